"""guber_mesh_eval_small's and guber_mesh_small_stats' argument checks on the product library: they come before any HIP call, so they
hold on a machine without a GPU (tests/test_mesh_abi_cpu.py for the mesh's other entry points)."""
import ctypes as C
import os

import pytest

import gubernator_amd as ga
from gubernator_amd import mesh as gm


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(ga.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    ga.lib()
    return gm._lib()


def test_the_small_call_and_its_statistics_reject_null(L):
    st = gm.MeshSmallStats()
    B, R = (ga.GuberBatch * 1)(), (ga.GuberResult * 1)()
    assert L.guber_mesh_eval_small(None, B, R, None) == ga.E_INVALID_ARG
    assert L.guber_mesh_small_stats(None, C.byref(st)) == ga.E_INVALID_ARG
    assert [f[0] for f in gm.MeshSmallStats._fields_] == ["calls", "launches", "wholesale_fallbacks", "share_fallbacks"]
    assert hasattr(gm.Mesh, "eval_small") and hasattr(gm.Mesh, "small_stats")
