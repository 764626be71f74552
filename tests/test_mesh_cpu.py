"""The mesh of fronts (guber_mesh_*, gubernator_amd/csrc/guber_mesh.h, guber_kernels_mesh.h) on a machine without a GPU: scenarios a - f
and h of tests/mesh_cases.py against the CPU build of the engine — host code and kernels compiled against tests/hostsim/fakehip
(`make -C tests/hostsim enginesim_lib`, the plain library) — each in a process of its own with GUBER_HIP_LIB pointing at it.  Test
infrastructure only: the product library is hipcc's and needs a device.  Scenario g (sixteen ranks) and the residency of GLOBAL engines
on a device run in tests/test_gpu_mesh.py."""
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


@pytest.mark.parametrize("letter", ["a", "b", "c", "d", "e", "f", "h"])
def test_mesh_scenario(enginesim, letter):
    """a sizes and empty generations (+ i residency), b ragged / empty / over-long keys (+ i), c the order across sources, d skew (fnv1 and
    fnv1a rings), e an inflow larger than the front's max_n, f GLOBAL requests stay, h one rank equals a plain front"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mesh_cases.py"), letter], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, GUBER_HIP_LIB=enginesim))
    assert p.returncode == 0 and f"MESH CASE OK {letter}" in p.stdout, (p.stdout + p.stderr)[-3000:]
