"""The end of the 53-bit recency stamp without a GPU: tests/stamp_end_cases.py — every pipeline, the cache operations, the one-launch path, fused
launches with an evaluation held back (where the CPU build can count the launches: k_evalpart_multi carried passes before and after each
renumbering), the front, moved-in buckets — on the CPU build of the engine (tests/hostsim/enginesim.cpp: host code and kernels compiled for the
host), in a process of its own with nothing preloaded.  The same paths under AddressSanitizer are the stand-alone program of
tests/test_stamp_end_asan_cpu.py; the GPU runs them in tests/test_gpu_stamp_end.py."""
import os
import subprocess
import sys

from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")


def test_stamp_end_cases_on_the_cpu_engine():
    subprocess.run(["make", "-s", "-C", HS, "enginesim_lib"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stamp_end_cases.py")], capture_output=True, text=True, timeout=1200,
                       env=dict(os.environ, GUBER_HIP_LIB=os.path.join(HS, "libenginesim.so")))
    assert p.returncode == 0 and "STAMP END CASES OK: 14 cases" in p.stdout, (p.stdout + p.stderr)[-3000:]
