"""The mesh's one-launch path (guber_mesh_eval_small, gubernator_amd/csrc/guber_mesh.h; k_mx_small, guber_kernels_small.h) on a machine
without a GPU: the scenarios of tests/mesh_small_cases.py against the CPU build of the engine — host code and kernels compiled against
tests/hostsim/fakehip (`make -C tests/hostsim enginesim_lib`) — each in a process of its own with GUBER_HIP_LIB pointing at it.  Test
infrastructure only: the product library is hipcc's and needs a device."""
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


@pytest.mark.parametrize("letter", ["a", "b", "c", "d", "e", "f", "g", "h", "i"])
def test_mesh_small_scenario(enginesim, letter):
    """a sizes, the refusal of 257 and residency; b ragged, empty and over-long keys, ranks of 32 and 64 bytes; c the order across sources;
    d a share that falls back; e wholesale fall-backs; f mixing with guber_mesh_eval_dev; g the rule after a placement commit; h GLOBAL;
    i one rank and sixteen, both hashes"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mesh_small_cases.py"), letter], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, GUBER_HIP_LIB=enginesim))
    assert p.returncode == 0 and f"MESH SMALL CASE OK {letter}" in p.stdout, (p.stdout + p.stderr)[-3000:]
