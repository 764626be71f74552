"""guber_wire_mesh_pool_* on a machine without a GPU: the cases of tests/mesh_pool_cases.py against the CPU build of the engine — host code
(guber_wire_mesh_pool.h, the split of guber_wire_dev_eval_mesh_enc) and kernels compiled against tests/hostsim/fakehip
(`make -C tests/hostsim enginesim_lib`) — each in a process of its own with GUBER_HIP_LIB pointing at it, nothing preloaded.  Test
infrastructure only: the product library is hipcc's and needs a device; the same cases run there in tests/test_gpu_mesh_pool.py."""
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


@pytest.mark.parametrize("letter", ["a", "b", "c12", "c24", "d", "e", "f1", "f8"])
def test_mesh_pool_case(enginesim, letter):
    """a one caller walking three ranks, every item class, bytes against the oracles; b the golden functional scenarios at W = 2; c 12 callers
    and three sets, 24 callers and two sets: conservation, owners' addresses, messages turned away; d stage limits; e refusals; f one rank
    against guber_wire_pool, eight ranks of which two receive nothing"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mesh_pool_cases.py"), letter], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, GUBER_HIP_LIB=enginesim))
    assert p.returncode == 0 and f"MESH POOL CASE OK {letter}" in p.stdout, (p.stdout + p.stderr)[-3000:]
