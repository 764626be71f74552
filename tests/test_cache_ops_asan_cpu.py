"""Memory safety of the cache operations under AddressSanitizer: tests/hostsim/cache_ops_main.cpp — the engine's host code and kernels compiled
for the host against tests/hostsim/fakehip, with a main() of its own — drives, through the C ABI, case b of tests/cache_ops_cases.py (Add of long
keys and duplicates under the weak hash: the host's waves, each with a key buffer of its own), case f (guber_dump into buffers of exactly the
sizes it asks for, and one short) and case i (200 keys moved into a destination with a smaller max_key_bytes: staging rows padded by hand to
their stride, refused buckets restored).  State is compared with a std::map model.  A stand-alone program: nothing is preloaded."""
import os
import subprocess

from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")
CS = os.path.join(ROOT, "gubernator_amd", "csrc")


def test_add_dump_and_move_under_the_address_sanitizer(tmp_path):
    exe = str(tmp_path / "cache_ops_main")
    # (the command line of tests/test_table_full_asan_cpu.py)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fsanitize=address", "-Wno-attributes", "-Wno-unknown-pragmas",
           "-Wno-subobject-linkage", "-DGUBER_LAB", "-I", os.path.join(HS, "fakehip"), "-I", os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(HS, "cache_ops_main.cpp")] + [os.path.join(CS, f) for f in ("guber_host.cpp", "placement.cpp", "worker_pool.cpp", "wire.cpp")] + \
          ["-lpthread", "-ldl"]
    c = subprocess.run(cmd, capture_output=True, text=True, cwd=HS, timeout=900)
    assert c.returncode == 0, c.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0 and "CACHE OPS MAIN OK" in p.stdout, (p.stdout + p.stderr)[-3000:]
