"""Memory safety of guber_wire_mesh_pool_* under AddressSanitizer: tests/hostsim/mesh_pool_main.cpp — the engine's host code and kernels compiled
for the host against tests/hostsim/fakehip, with a main() of its own — drives, through the C ABI, six caller threads over a mesh of three
ranks: every payload fills its stage's staging buffer to its last 16 bytes, every response buffer is an allocation of exactly
guber_wire_mesh_pool_response_bound bytes (cap = the bound), every second RPC is marshalled by its caller through the host transcoder, and
the "device" buffers of the decoders, the mesh and the encoder are host allocations: a byte behind any of them is a report.
A stand-alone program: nothing is preloaded."""
import os
import subprocess

from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")


def test_the_payload_stage_over_a_mesh_under_the_address_sanitizer(tmp_path):
    exe = str(tmp_path / "mesh_pool_main")
    c = subprocess.run(["make", "-s", "-C", HS, "-f", "mesh_pool.mk", "mesh_pool_asan", "MESH_POOL_ASAN_OUT=" + exe], capture_output=True, text=True, timeout=900)
    assert c.returncode == 0, (c.stdout + c.stderr)[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0 and "MESH POOL MAIN OK" in p.stdout, (p.stdout + p.stderr)[-3000:]
