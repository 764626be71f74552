"""Memory safety of the mesh's one-launch path under AddressSanitizer: tests/hostsim/mesh_small_main.cpp — the engine's host code and
kernels compiled for the host against tests/hostsim/fakehip, with a main() of its own — drives guber_mesh_eval_small on three ranks of
two engines over totals of 1, 64, 256, 255 and 129 ragged keys (an empty and an over-long one among them), a refused call of 257 and a
share that falls back, every buffer an allocation of exactly its size, and compares the answers with a token-bucket model and the
forwarded count and the owner column with the host ring.  A stand-alone program: nothing is preloaded."""
import os
import subprocess

from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")
CS = os.path.join(ROOT, "gubernator_amd", "csrc")


def test_small_calls_on_a_mesh_of_three_ranks_under_the_address_sanitizer(tmp_path):
    exe = str(tmp_path / "mesh_small_main")
    # (the flags of tests/hostsim/Makefile's enginesim_san_lib rule, without -shared)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fsanitize=address", "-Wno-attributes", "-Wno-unknown-pragmas",
           "-Wno-subobject-linkage", "-DGUBER_LAB", "-I", os.path.join(HS, "fakehip"), "-I", os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(HS, "mesh_small_main.cpp")] + [os.path.join(CS, f) for f in ("guber_host.cpp", "placement.cpp", "worker_pool.cpp", "wire.cpp")] + \
          ["-lpthread", "-ldl"]
    c = subprocess.run(cmd, capture_output=True, text=True, cwd=HS, timeout=900)
    assert c.returncode == 0, c.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0 and "MESH SMALL MAIN OK" in p.stdout, (p.stdout + p.stderr)[-3000:]
