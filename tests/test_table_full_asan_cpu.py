"""Memory safety of the long-key arena under AddressSanitizer: tests/hostsim/table_full_main.cpp — the engine's host code and kernels compiled
for the host against tests/hostsim/fakehip, with a main() of its own — drives cases 1, 2 and 3 of tests/table_full_cases.py through the C ABI,
once on the two-launch and once on the owner-partitioned pipeline: the arena's bound asks for rebuilds, the rebuilds copy the live keys from the
old arena into a new one — of another size once the arena grows: where an off-by-8 in that copy shows —, and with GUBER_FLAG_TEST_FIXED_ARENA the
arena runs full and refuses.  Answers are compared with a std::map model.  A stand-alone program: nothing is preloaded."""
import os
import subprocess

from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")
CS = os.path.join(ROOT, "gubernator_amd", "csrc")


def test_the_arena_fills_grows_and_refuses_under_the_address_sanitizer(tmp_path):
    exe = str(tmp_path / "table_full_main")
    # (the flags of tests/hostsim/Makefile's enginesim_san_lib rule, without -shared)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fsanitize=address", "-Wno-attributes", "-Wno-unknown-pragmas",
           "-Wno-subobject-linkage", "-DGUBER_LAB", "-I", os.path.join(HS, "fakehip"), "-I", os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(HS, "table_full_main.cpp")] + [os.path.join(CS, f) for f in ("guber_host.cpp", "placement.cpp", "worker_pool.cpp", "wire.cpp")] + \
          ["-lpthread", "-ldl"]
    c = subprocess.run(cmd, capture_output=True, text=True, cwd=HS, timeout=900)
    assert c.returncode == 0, c.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0 and "TABLE FULL MAIN OK" in p.stdout, (p.stdout + p.stderr)[-3000:]
