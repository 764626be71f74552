"""The host protocol of the payload stage over a mesh with lone small RPCs evaluated by their callers, under ThreadSanitizer:
tests/hostsim/mesh_pool_direct_tsan.cpp — guber_wire_mesh_pool.h and guber_wire_mesh_pool_direct.h against stand-ins, with its own main() —
runs direct callers and set callers at once while guber_wire_mesh_pool_set_direct is toggled, and checks per-key conservation over all
answers.  A stand-alone program: nothing is preloaded."""
import os
import subprocess

from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")


def test_direct_callers_and_set_callers_at_once_under_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "mesh_pool_direct_tsan")
    c = subprocess.run(["make", "-s", "-C", HS, "-f", "mesh_pool_direct.mk", "mesh_pool_direct_tsan", "MESH_POOL_DIRECT_TSAN_OUT=" + exe],
                       capture_output=True, text=True, timeout=900)
    assert c.returncode == 0, (c.stdout + c.stderr)[-3000:]
    p = subprocess.run([exe, "16", "400"], capture_output=True, text=True, timeout=900)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0 and "MESH POOL DIRECT TSAN OK" in p.stdout, tail
    assert "ThreadSanitizer" not in p.stderr, tail
