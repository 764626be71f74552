"""The host protocol of guber_wire_mesh_pool_* under ThreadSanitizer: gubernator_amd/csrc/guber_wire_mesh_pool.h compiled on its own against
stand-ins for the device decoder and the mesh evaluation (tests/hostsim/mesh_pool_tsan.cpp: the host transcoder and one oracle, the decode
"collected" after a few polls, a mesh that refuses two sets at once, an uncollected decode or two instants in one set).  16 callers walking
three ranks, 4 000 RPCs; two sets with stages of two RPCs (callers seal full stages all the time), then three sets with stages of sixteen;
one RPC in sixteen carries an item error and is marshalled by its caller; per-key conservation over all answers; a pool destroyed without
ever seeing a caller.  A clean report is asserted.  (The real decoder, mesh and encoder run under AddressSanitizer:
tests/test_mesh_pool_asan_cpu.py; the fiber runtime of the CPU engine is not something ThreadSanitizer follows.)  A stand-alone program."""
import os
import subprocess

from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")


def test_the_mesh_pools_host_protocol_under_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "mesh_pool_tsan")
    c = subprocess.run(["make", "-s", "-C", HS, "-f", "mesh_pool.mk", "mesh_pool_tsan", "MESH_POOL_TSAN_OUT=" + exe], capture_output=True, text=True, timeout=900)
    assert c.returncode == 0, (c.stdout + c.stderr)[-3000:]
    for _ in range(2):
        p = subprocess.run([exe, "16", "250", "20"], capture_output=True, text=True, timeout=900)
        tail = (p.stdout + p.stderr)[-3000:]
        assert p.returncode == 0 and "MESH POOL TSAN OK" in p.stdout, tail
        assert "ThreadSanitizer" not in p.stderr, tail
