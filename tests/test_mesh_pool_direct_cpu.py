"""The payload stage over a mesh with lone small RPCs evaluated by their caller (guber_wire_mesh_pool_set_direct) on a machine without a
GPU: the cases of tests/mesh_pool_direct_cases.py against the CPU build of the engine (`make -C tests/hostsim enginesim_lib`), each in a
process of its own with GUBER_HIP_LIB pointing at it, nothing preloaded.  Test infrastructure only: the product library is hipcc's and
needs a device; the same cases run there in tests/test_gpu_mesh_pool_direct.py."""
import os
import subprocess
import sys

import pytest

from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")
LIB = os.path.join(HS, "libenginesim.so")


@pytest.fixture(scope="module")
def enginesim():
    subprocess.run(["make", "-s", "-C", HS, "enginesim_lib"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    return LIB


@pytest.mark.parametrize("letter", ["j0", "j1", "k", "l", "m"])
def test_mesh_pool_direct_case(enginesim, letter):
    """j one caller walking three ranks with set_direct(4, 8), every item class and error, bytes against the oracles (wrap_errors 0 and 1);
    k refusals with the path on; l 16 callers with set_direct(4, 2): conservation, both paths; m off by default and off again"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mesh_pool_direct_cases.py"), letter], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, GUBER_HIP_LIB=enginesim))
    assert p.returncode == 0 and f"MESH POOL DIRECT CASE OK {letter}" in p.stdout, (p.stdout + p.stderr)[-3000:]
