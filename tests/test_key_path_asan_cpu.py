"""Memory safety of the key path under AddressSanitizer: tests/hostsim/key_path_main.cpp — the engine's host code and kernels compiled for
the host against tests/hostsim/fakehip, with a main() of its own — sends generations of fixed-width keys (widths 1, 7, 8, 9, 15, 16, 17,
24, 25, 31, 32; 1, 1 024 and 1 025 requests) through guber_front_eval_dev on three engines whose shares go in two pieces, the key buffer an
allocation of exactly n x width + 8 bytes: the speculative key fetch (key_fetch_spec) and the copy of the keys into the shares may read the
8 bytes the API promises behind the last key and not one more.  Answers are compared with a std::map model.  A stand-alone program:
nothing is preloaded."""
import os
import subprocess

from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")
CS = os.path.join(ROOT, "gubernator_amd", "csrc")


def test_fixed_width_generations_under_the_address_sanitizer(tmp_path):
    exe = str(tmp_path / "key_path_main")
    # (the flags of tests/hostsim/Makefile's enginesim_san_lib rule, without -shared)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fsanitize=address", "-Wno-attributes", "-Wno-unknown-pragmas",
           "-Wno-subobject-linkage", "-DGUBER_LAB", "-I", os.path.join(HS, "fakehip"), "-I", os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(HS, "key_path_main.cpp")] + [os.path.join(CS, f) for f in ("guber_host.cpp", "placement.cpp", "worker_pool.cpp", "wire.cpp")] + \
          ["-lpthread", "-ldl"]
    c = subprocess.run(cmd, capture_output=True, text=True, cwd=HS, timeout=900)
    assert c.returncode == 0, c.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0 and "KEY PATH MAIN OK" in p.stdout, (p.stdout + p.stderr)[-3000:]
