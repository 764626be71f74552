"""guber_wire_dev_eval_mesh_enc on a machine without a GPU: the cases of tests/mesh_enc_cases.py against the CPU build of the engine — host
code and kernels (k_mx_count's item_owner[], k_wire_enc_owner) compiled against tests/hostsim/fakehip (`make -C tests/hostsim enginesim_lib`)
— each in a process of its own with GUBER_HIP_LIB pointing at it.  Test infrastructure only: the product library is hipcc's and needs a
device; the same cases run there in tests/test_gpu_mesh_enc.py."""
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


@pytest.mark.parametrize("letter", ["a", "b", "c", "d", "e", "r", "h"])
def test_mesh_enc_case(enginesim, letter):
    """a sizes around the encoder's piece, a twin world through eval_mesh; b the eight address lengths at W = 8; c every class of item in one
    RPC; d item errors; e a malformed payload between two good ones, dead slots; r refusals; h one rank"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mesh_enc_cases.py"), letter], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, GUBER_HIP_LIB=enginesim))
    assert p.returncode == 0 and f"MESH ENC CASE OK {letter}" in p.stdout, (p.stdout + p.stderr)[-3000:]
