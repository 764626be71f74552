"""The cache operations without a GPU: tests/cache_ops_cases.py — Add across workgroups, under colliding tags and into a binding cache, the
dump's buffer protocol, a restart through dump and load, device item columns, moves between tables — on the CPU build of the engine
(tests/hostsim/enginesim.cpp: host code and kernels compiled for the host), in a process of its own.  That build runs plain here, with nothing
preloaded; the same paths under AddressSanitizer are the stand-alone program of tests/test_cache_ops_asan_cpu.py.  The CPU build runs a
launch's workgroups one at a time: it checks the logic, the GPU tests (tests/test_gpu_cache_ops.py) the ordering between workgroups."""
import os
import subprocess
import sys

from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")


def test_cache_ops_cases_on_the_cpu_engine():
    subprocess.run(["make", "-s", "-C", HS, "enginesim_lib"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cache_ops_cases.py")], capture_output=True, text=True, timeout=1200,
                       env=dict(os.environ, GUBER_HIP_LIB=os.path.join(HS, "libenginesim.so")))
    assert p.returncode == 0 and "CACHE OPS CASES OK" in p.stdout, (p.stdout + p.stderr)[-3000:]
