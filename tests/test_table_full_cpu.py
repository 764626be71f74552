"""The table-full answer and the long-key arena without a GPU: tests/table_full_cases.py — churn over a small cache, a cache's worth of long
keys, the arena's refusal (GUBER_FLAG_TEST_FIXED_ARENA), the probe bound, a chain across the table's end, each on every pipeline — on the CPU
build of the engine (tests/hostsim/enginesim.cpp: host code and kernels compiled for the host), in a process of its own.  That build runs
plain here, with nothing preloaded; the arena's path under AddressSanitizer is the stand-alone program of tests/test_table_full_asan_cpu.py.
Reduced for the CPU (table_full_cases.CPU_CHAIN_BATCH): case 4 fills its chain of 4 096 keys in batches of 32 instead of 512 — n new keys under
ONE hash take about n rounds of up to n requests that each walk the chain; table_slots stays 8 192.  No case is dropped."""
import os
import subprocess
import sys

from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")


def test_table_full_cases_on_the_cpu_engine():
    subprocess.run(["make", "-s", "-C", HS, "enginesim_lib"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "table_full_cases.py")], capture_output=True, text=True, timeout=2400,
                       env=dict(os.environ, GUBER_HIP_LIB=os.path.join(HS, "libenginesim.so")))
    assert p.returncode == 0 and "TABLE FULL CASES OK" in p.stdout, (p.stdout + p.stderr)[-3000:]
