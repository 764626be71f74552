"""The argument checks of guber_mesh_eval_rows_dev and guber_wire_dev_eval_mesh on the product library: they run before any HIP call and
before a mesh, a front or a decoder is looked into, so they hold on a machine without a GPU (tests/test_mesh_abi_cpu.py for the mesh's
other entry points).  A mesh of one rank needs no device to exist: guber_mesh_create_local looks at its front's fields only, which are
those of a block of zeroed memory here — no check below gets as far as using it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gubernator_amd as ga
import support
from gubernator_amd import mesh as gm
from gubernator_amd import wire as gw


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(ga.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    ga.lib()
    gw._lib()
    return gm._lib()


def test_both_symbols_are_declared_listed_and_exported(L):
    """guber_mesh_eval_rows_dev belongs to include/guber_gpu.h and ABI_SYMBOLS; guber_wire_dev_eval_mesh is declared in include/guber_wire.h,
    whose symbols the package lists as wire.WIRE_SYMBOLS (ABI_SYMBOLS is, symbol for symbol, what guber_gpu.h declares:
    tests/test_abi_cpu.py)"""
    gpu_h = open(os.path.join(support.ROOT, "include", "guber_gpu.h")).read()
    wire_h = open(os.path.join(support.ROOT, "include", "guber_wire.h")).read()
    assert re.search(r"\bint guber_mesh_eval_rows_dev\s*\(", gpu_h) and "guber_mesh_rows_t" in gpu_h
    assert re.search(r"\bint guber_wire_dev_eval_mesh\s*\(", wire_h)
    assert "guber_mesh_eval_rows_dev" in ga.ABI_SYMBOLS and "guber_wire_dev_eval_mesh" in gw.WIRE_SYMBOLS
    assert hasattr(L, "guber_mesh_eval_rows_dev") and hasattr(L, "guber_wire_dev_eval_mesh")
    assert ga.MeshRows is gm.MeshRows and C.sizeof(gm.MeshRows) == 16


def test_null_arguments_of_both_entry_points(L):
    L.guber_wire_dev_eval_mesh.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(ga.GuberResult)]
    E = ga.E_INVALID_ARG
    B, R, RW = (ga.GuberBatch * 1)(), (ga.GuberResult * 1)(), (gm.MeshRows * 1)()
    decs = (C.c_void_p * 1)(None)
    assert L.guber_mesh_eval_rows_dev(None, B, RW, R) == E
    assert L.guber_mesh_eval_rows_dev(C.c_void_p(0x1000), None, RW, R) == E
    assert L.guber_mesh_eval_rows_dev(C.c_void_p(0x1000), B, RW, None) == E
    assert L.guber_wire_dev_eval_mesh(None, C.c_void_p(0x1000), R) == E
    assert L.guber_wire_dev_eval_mesh(decs, None, R) == E
    assert L.guber_wire_dev_eval_mesh(decs, C.c_void_p(0x1000), None) == E


@pytest.fixture()
def mesh1(L):
    """a mesh of one rank over a front nobody dereferences usefully: zeroed memory of ample size (see the module's docstring)"""
    ring = ga.Ring(["gpu0"], 512)
    blob = (C.c_uint8 * (1 << 16))()
    fronts = (C.c_void_p * 1)(C.addressof(blob))
    h = C.c_void_p()
    assert L.guber_mesh_create_local(fronts, 1, ring.h, 1 << 22, C.byref(h)) == 0, L.guber_last_error()
    yield h
    L.guber_mesh_destroy(h)
    ring.close()


def test_row_arguments_are_checked_before_any_hip_call(L, mesh1):
    n = 4
    col = np.zeros(n, np.int64)
    out8, out64 = np.zeros(n, np.uint8), np.zeros(n, np.int64)
    klen = np.zeros(n, np.uint32)
    rows = np.zeros(n * 24, np.uint8)

    def call(n=n, stride=24, key_len=klen.ctypes.data, key_off=None):
        B = (ga.GuberBatch * 1)(ga.GuberBatch(n, 0, rows.ctypes.data, key_off, col.ctypes.data, col.ctypes.data, col.ctypes.data, None, None, None, None,
                                              None, None, None, 1_700_000_000_000))
        R = (ga.GuberResult * 1)(ga.GuberResult(out8.ctypes.data, out64.ctypes.data, out64.ctypes.data, out64.ctypes.data, out8.ctypes.data, 0, 0, 0, 0, 0))
        RW = (gm.MeshRows * 1)(gm.MeshRows(stride, key_len))
        return L.guber_mesh_eval_rows_dev(mesh1, B, RW, R)

    assert call(stride=20) == ga.E_INVALID_ARG and b"multiple of 8" in L.guber_last_error()
    assert call(key_off=klen.ctypes.data) == ga.E_INVALID_ARG and b"key_off" in L.guber_last_error()
    assert call(key_len=None) == ga.E_INVALID_ARG and b"key_len" in L.guber_last_error()
    # n x key_stride past 32 bits: 2^22 rows (the mesh's max_n) of 1 024 bytes
    assert call(n=1 << 22, stride=1024) == ga.E_BATCH_TOO_LARGE and b"4 GB" in L.guber_last_error()
    # more rows than the mesh was created for
    assert call(n=(1 << 22) + 1, stride=8) == ga.E_BATCH_TOO_LARGE
