"""Memory safety of the front's observation kernels under AddressSanitizer: tests/hostsim/front_observe_main.cpp — the engine's host code
and kernels compiled for the host against tests/hostsim/fakehip, with a main() of its own — runs k_fr_observe / k_fr_observe_top on
generations of 1, 64, 1 025 and 4 097 requests whose key buffers end exactly where they may be read (packed keys: 8 bytes behind the last
key; key rows with non-zero padding: with the last row), with and without the per-tile aggregation, and compares every window with a
std::map model.  A stand-alone program: nothing is preloaded."""
import os
import subprocess

from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")
CS = os.path.join(ROOT, "gubernator_amd", "csrc")


def test_observation_kernels_under_the_address_sanitizer(tmp_path):
    exe = str(tmp_path / "front_observe_main")
    # (the flags of tests/hostsim/Makefile's enginesim_san_lib rule, without -shared)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fsanitize=address", "-Wno-attributes", "-Wno-unknown-pragmas",
           "-Wno-subobject-linkage", "-DGUBER_LAB", "-I", os.path.join(HS, "fakehip"), "-I", os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(HS, "front_observe_main.cpp")] + [os.path.join(CS, f) for f in ("guber_host.cpp", "placement.cpp", "worker_pool.cpp", "wire.cpp")] + \
          ["-lpthread", "-ldl"]
    c = subprocess.run(cmd, capture_output=True, text=True, cwd=HS, timeout=900)
    assert c.returncode == 0, c.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0 and "FRONT OBSERVE MAIN OK" in p.stdout, (p.stdout + p.stderr)[-3000:]
