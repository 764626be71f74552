"""Memory safety of guber_wire_dev_eval_mesh_enc under AddressSanitizer: tests/hostsim/mesh_enc_main.cpp — the engine's host code and kernels
compiled for the host against tests/hostsim/fakehip, with a main() of its own — drives, through the C ABI, the shape of
tests/mesh_enc_cases.py's case a (three ranks, RPCs of 0 .. 2 P + 1 items around the piece of k_wire_enc_owner, a rank without a decoder, a
decoder that decoded nothing, addresses of 11, 128 and 264 bytes).  Each buf, off, len and owner_rank is an allocation of exactly its required
size, and the "device" buffers of k_mx_count's item_owner[] and of the encoder are host allocations: a byte behind any of them is a report.
A stand-alone program: nothing is preloaded."""
import os
import subprocess

from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")


def test_the_mesh_encoder_under_the_address_sanitizer(tmp_path):
    exe = str(tmp_path / "mesh_enc_main")
    c = subprocess.run(["make", "-s", "-C", HS, "-f", "mesh_enc.mk", "mesh_enc_asan", "MESH_ENC_OUT=" + exe], capture_output=True, text=True, timeout=900)
    assert c.returncode == 0, (c.stdout + c.stderr)[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0 and "MESH ENC MAIN OK" in p.stdout, (p.stdout + p.stderr)[-3000:]
