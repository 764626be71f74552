"""ctypes binding of the mesh of fronts (include/guber_gpu.h: guber_mesh_*; implementation gubernator_amd/csrc/guber_mesh.h,
kernels guber_kernels_mesh.h): rank r is peer r of a Ring and owns one Front; a call takes the generation that arrived at every
rank, evaluates every request on the rank the ring names (gubernator.go:236-283) and answers it, in arrival order, where it arrived."""
import ctypes as C

from . import GuberBatch, GuberError, GuberResult, lib


class MeshStats(C.Structure):
    _fields_ = [("calls", C.c_uint64), ("requests", C.c_uint64), ("forwarded", C.c_uint64), ("bytes_moved", C.c_uint64),
                ("inflow_pieces", C.c_uint64), ("ms", C.c_double)]


class MeshSmallStats(C.Structure):
    _fields_ = [("calls", C.c_uint64), ("launches", C.c_uint64), ("wholesale_fallbacks", C.c_uint64), ("share_fallbacks", C.c_uint64)]


class MeshRows(C.Structure):
    """guber_mesh_rows_t: key_stride 0 = the rank's generation is packed; otherwise its keys lie in rows key_stride bytes apart (a
    multiple of 8) and key_len is a device array of the keys' lengths"""
    _fields_ = [("key_stride", C.c_uint32), ("key_len", C.c_void_p)]


_bound = False


def _lib():
    global _bound
    L = lib()
    if not _bound:
        L.guber_mesh_create_local.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.guber_mesh_eval_dev.argtypes = [C.c_void_p, C.POINTER(GuberBatch), C.POINTER(GuberResult)]
        L.guber_mesh_eval_rows_dev.argtypes = [C.c_void_p, C.POINTER(GuberBatch), C.POINTER(MeshRows), C.POINTER(GuberResult)]
        L.guber_mesh_eval_small.argtypes = [C.c_void_p, C.POINTER(GuberBatch), C.POINTER(GuberResult), C.POINTER(C.c_void_p)]
        L.guber_mesh_small_stats.argtypes = [C.c_void_p, C.POINTER(MeshSmallStats)]
        L.guber_mesh_synchronize.argtypes = [C.c_void_p]
        L.guber_mesh_stats.argtypes = [C.c_void_p, C.POINTER(MeshStats)]
        L.guber_mesh_destroy.argtypes = [C.c_void_p]
        L.guber_mesh_destroy.restype = None
        _bound = True
    return L


def _check(rc):
    if rc != 0:
        L = lib()
        raise GuberError(rc, f"{L.guber_strerror(rc).decode()} ({L.guber_last_error().decode()})")


class Mesh:
    """guber_mesh_t over fronts[r] = rank r = peer r of `ring`; max_n: the largest generation per rank and call.  Every rank lives in
    this process (guber_mesh_create_local); the ranks' fronts may share a device."""

    def __init__(self, fronts, ring, max_n):
        self.fronts, self.ring = list(fronts), ring
        arr = (C.c_void_p * max(len(self.fronts), 1))(*[f.h for f in self.fronts])
        self.h = C.c_void_p()
        _check(_lib().guber_mesh_create_local(arr, len(self.fronts), ring.h if ring is not None else None, max_n, C.byref(self.h)))

    def eval_dev(self, gens, results):
        """ctypes arrays of len(fronts) GuberBatch / GuberResult (device pointers on each rank's device, arrival order); asynchronous"""
        _check(_lib().guber_mesh_eval_dev(self.h, gens, results))

    def eval_rows_dev(self, gens, rows, results):
        """eval_dev for generations whose keys lie in rows: `rows` a ctypes array of len(fronts) MeshRows (None: every rank packed); rank
        r with rows[r].key_stride != 0 has gens[r].key_bytes = its first row and gens[r].key_off = None"""
        _check(_lib().guber_mesh_eval_rows_dev(self.h, gens, rows, results))

    def eval_small(self, gens, results, owner_rank=None):
        """the one-launch path for a call of at most 256 requests over all ranks (guber_mesh_eval_small): ctypes arrays of len(fronts)
        GuberBatch / GuberResult of HOST pointers; owner_rank: None, or a ctypes array of len(fronts) c_void_p (None, or gens[r].n bytes
        that receive the ring's owner of every item, 0xFF = none).  Synchronous: the answers are complete on return"""
        _check(_lib().guber_mesh_eval_small(self.h, gens, results, owner_rank))

    def small_stats(self):
        st = MeshSmallStats()
        _check(_lib().guber_mesh_small_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in MeshSmallStats._fields_}

    def synchronize(self):
        _check(_lib().guber_mesh_synchronize(self.h))

    def stats(self):
        st = MeshStats()
        _check(_lib().guber_mesh_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in MeshStats._fields_}

    def close(self):
        if getattr(self, "h", None):
            _lib().guber_mesh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001
            pass
