"""Key rows through the mesh of fronts (guber_mesh_eval_rows_dev, guber_wire_dev_eval_mesh) on a machine without a GPU: the cases of
tests/mesh_rows_cases.py against the CPU build of the engine — host code and kernels compiled against tests/hostsim/fakehip
(`make -C tests/hostsim enginesim_lib`, the plain library) — each in a process of its own with GUBER_HIP_LIB pointing at it.  Test
infrastructure only: the product library is hipcc's and needs a device.  Sixteen ranks run in tests/test_gpu_mesh_rows.py."""
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


@pytest.mark.parametrize("letter", ["a", "b", "c", "d", "e", "r", "f", "g", "h"])
def test_mesh_rows_case(enginesim, letter):
    """through the wire: a sizes and residency, b key widths at strides 24 and 72, c the order across sources, d GLOBAL, e an inflow larger
    than the front's max_n, r refusals; rows without the wire: f rows versus packed, g mixed forms in one call, h one rank"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mesh_rows_cases.py"), letter], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, GUBER_HIP_LIB=enginesim))
    assert p.returncode == 0 and f"MESH ROWS CASE OK {letter}" in p.stdout, (p.stdout + p.stderr)[-3000:]
