"""guber_mesh_*'s argument checks on the product library: they run before any HIP call and before a front is looked into, so they hold on a
machine without a GPU (tests/test_abi_cpu.py::test_argument_checks_need_no_device for the other entry points)."""
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


def _fronts(*addresses):
    """an array of front handles nobody dereferences: every check below fails before a front is looked into"""
    return (C.c_void_p * len(addresses))(*addresses)


def test_create_rejects_malformed_calls_without_a_device(L):
    ring3 = ga.Ring(["gpu0", "gpu1", "gpu2"], 512)
    out = C.c_void_p()
    E = ga.E_INVALID_ARG
    assert L.guber_mesh_create_local(None, 3, ring3.h, 64, C.byref(out)) == E
    assert L.guber_mesh_create_local(_fronts(0x1000, 0x2000, 0x3000), 3, None, 64, C.byref(out)) == E
    assert L.guber_mesh_create_local(_fronts(0x1000, 0x2000, 0x3000), 3, ring3.h, 64, None) == E
    assert L.guber_mesh_create_local(_fronts(0x1000), 0, ring3.h, 64, C.byref(out)) == E and not out.value
    assert L.guber_mesh_create_local(_fronts(*range(0x1000, 0x1000 + 17 * 16, 16)), 17, ring3.h, 64, C.byref(out)) == E and not out.value
    # the ring's peers are the ranks
    assert L.guber_mesh_create_local(_fronts(0x1000, 0x2000), 2, ring3.h, 64, C.byref(out)) == E and not out.value
    assert b"peers" in L.guber_last_error()
    # one front twice, a null front
    assert L.guber_mesh_create_local(_fronts(0x1000, 0x2000, 0x1000), 3, ring3.h, 64, C.byref(out)) == E and not out.value
    assert b"twice" in L.guber_last_error()
    assert L.guber_mesh_create_local(_fronts(0x1000, None, 0x3000), 3, ring3.h, 64, C.byref(out)) == E and not out.value
    assert L.guber_mesh_create_local(_fronts(0x1000, 0x2000, 0x3000), 3, ring3.h, 0, C.byref(out)) != 0 and not out.value
    ring3.close()


def test_the_other_entry_points_reject_null(L):
    st = gm.MeshStats()
    assert L.guber_mesh_eval_dev(None, None, None) == ga.E_INVALID_ARG
    assert L.guber_mesh_synchronize(None) == ga.E_INVALID_ARG
    assert L.guber_mesh_stats(None, C.byref(st)) == ga.E_INVALID_ARG
    L.guber_mesh_destroy(None)
    with pytest.raises(ga.GuberError):
        gm.Mesh([], None, 64)
    assert ga.Mesh is gm.Mesh
