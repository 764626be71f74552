"""Memory safety of the renumbering at the end of the 53-bit recency stamp under AddressSanitizer: tests/hostsim/stamp_end_main.cpp — the engine's
host code and kernels compiled for the host against tests/hostsim/fakehip, with a main() of its own — drives, through the C ABI, the cache
operations' case of tests/stamp_end_cases.py (Add of 11 items into a cache of 10 with six stamps left, as one call and item by item, GetItem, one
more Add) and the cyclic scan of its pipelines' case (24 binding batches of 240, the renumbering before step 15) against a std::list model of
LRUCache.  k_lru_gather, the sort and k_lru_renumber work on buffers of live + 64 entries that are host allocations here.  A stand-alone
program: nothing is preloaded."""
import os
import subprocess

from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")


def test_the_renumbering_under_the_address_sanitizer(tmp_path):
    exe = str(tmp_path / "stamp_end_main")
    c = subprocess.run(["make", "-s", "-C", HS, "-f", "stamp_end.mk", "stamp_end_asan", "STAMP_END_OUT=" + exe], capture_output=True, text=True, timeout=900)
    assert c.returncode == 0, (c.stdout + c.stderr)[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0 and "STAMP END MAIN OK" in p.stdout, (p.stdout + p.stderr)[-3000:]
