"""Recency stamps around 2^52 through the KERNEL SOURCE on the CPU (tests/hostsim/devsim.cpp, as tests/test_kernels_devsim.py runs it): after
ds_set_seq(2^52 - k) the batch pipelines, the eviction pre-pass and the cache-operation kernels write, read, compare and sort stamps whose
high 21 bits (Rec::meta >> 11) are set and change — rec_set_stamp / rec_stamp, the REC_META_MASK masking of rec_meta / rec_eq, k_lru_keys,
k_lru_win_flag, k_lru_gather, k_lru_risk's search, k_items_commit, k_item_lookup.  The driver and the positioning arithmetic are
tests/late_counters.py's; the GPU twin (the product library, the 53-bit device sort, the engine's host side) is tests/test_gpu_late_counters.py."""
import ctypes as C
import os
import subprocess

import pytest

import late_counters as lc
import scenarios
import streams
import support
from gubernator_amd.abi import GuberItem, item_dict
from support import GuberBatch, GuberResult, HostBatch, Oracle, assert_results_equal
from test_kernels_devsim import HS, Sim


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", HS, "devsim_lib"], check=True)
    L = C.CDLL(os.path.join(HS, "libdevsim.so"))
    L.ds_create_bounded.restype = C.c_void_p
    L.ds_create_bounded.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_uint64]
    L.ds_destroy.argtypes = [C.c_void_p]
    L.ds_eval.argtypes = [C.c_void_p, C.POINTER(GuberBatch), C.POINTER(GuberResult), C.c_int, C.c_int]
    L.ds_counters.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    L.ds_lru_stats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    L.ds_part_forms.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_ulonglong)]
    L.ds_set_seq.argtypes = [C.c_void_p, C.c_uint64]
    L.ds_seq.argtypes = [C.c_void_p]
    L.ds_seq.restype = C.c_uint64
    L.ds_add_items.argtypes = [C.c_void_p, C.POINTER(GuberItem), C.c_uint32, C.POINTER(C.c_uint8), C.c_int64]
    L.ds_item_lookup.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_int64, C.c_int, C.POINTER(GuberItem), C.POINTER(C.c_int)]
    L.owner_bits = 0
    return L


class SimBackend:
    """tests/late_counters.py's backend over a devsim table whose next stamp is the mirror's"""

    def __init__(self, lib, mirror, cache_size, pipeline=1, slots=1 << 13, max_batch=2048):
        self.sim = Sim(lib, slots=slots, max_batch=max_batch, pipeline=pipeline, cache_size=cache_size)
        self.lib, self.mirror = lib, mirror
        lib.ds_set_seq(self.sim.h, mirror.seq)

    def eval(self, b):
        return self.sim.eval(b)

    def totals(self):
        c = self.sim.counters()
        return (c[0], c[1], c[2], self.sim.lru_stats()["unexpired_evictions"], c[3])

    def add_items(self, items, now_ms):
        arr, ex = (GuberItem * len(items))(*items), (C.c_uint8 * len(items))()
        assert self.lib.ds_add_items(self.sim.h, arr, len(items), ex, now_ms) == 0
        return [bool(x) for x in ex]

    def _lookup(self, key, now_ms, mode):
        kb = key if isinstance(key, bytes) else key.encode()
        out, found = GuberItem(), C.c_int(0)
        assert self.lib.ds_item_lookup(self.sim.h, kb, len(kb), now_ms, mode, C.byref(out), C.byref(found)) == 0
        return item_dict(out, kb) if found.value else None

    def get_item(self, key, now_ms):
        return self._lookup(key, now_ms, 0)

    def remove_item(self, key):
        self._lookup(key, 0, 1)

    def rebuilds(self):
        return self.sim.lru_stats()["rebuilds"]

    def close(self):
        assert self.lib.ds_seq(self.sim.h) == self.mirror.seq, "the test's count of the stamps is not the table's"
        self.sim.close()


def test_the_mirror_holds_the_headers_values():
    """tests/late_counters.py's constants are gubernator_amd/csrc/guber_test_flags.h's (what guber_engine_create starts a flagged engine with)"""
    h = lc.header_values()
    assert (h["GUBER_FLAG_TEST_LATE_COUNTERS"], h["GUBER_TEST_LATE_SEQ_NEXT"], h["GUBER_TEST_LATE_EPOCH"], h["GUBER_TEST_LATE_EPOCH16"], h["GUBER_TEST_LATE_RB_SEQ"]) == \
        (lc.FLAG, lc.SEQ_NEXT, lc.EPOCH, lc.EPOCH16, lc.RB_SEQ) == (256, 2 ** 52 - 4096, 0x7fffffff - 12, 0xffff - 12, 0xffffffff - 8)
    import gubernator_amd as ga
    assert ga.FLAG_TEST_LATE_COUNTERS == lc.FLAG
    m = lc.Mirror()
    assert [m.batch(1)[1] for _ in range(13)] == [False] * 11 + [True, False] and m.epoch == 2          # the 12th batch wraps the directory epoch
    m = lc.Mirror()
    assert [m.batch(1)[2] for _ in range(14)] == [False] * 12 + [True, False] and m.epoch16 == 2        # the 13th the claim epoch
    m = lc.Mirror()
    assert [m.snapshot() for _ in range(10)] == [False] * 8 + [True, False] and m.rb_seq == 2           # the 9th snapshot skips 0


@pytest.mark.parametrize("pipeline", [1, 0])
@pytest.mark.parametrize("workload", lc.WORKLOADS)
def test_the_bounded_cache_keeps_the_reference_order_across_stamp_2_52(lib, pipeline, workload):
    """a cache of 300 under 400 keys, batches of 230 keys + 10 touched by every batch, 24 steps, k_part / k_own / k_eval3 (1) and k_front /
    k_eval2 (0): the table's next stamp set so that stamp 2^52 is request 100 of step 15 (Zipf fills the cache in step 9) — the tail list is rebuilt on both sides and its
    windows hold stamps from both.  Answers, counters, the size after every batch and the unexpired evictions equal the bounded-LRU oracle."""
    cs, n = 300, 240
    mirror = lc.Mirror(lc.CROSSING - (15 * n + 100))
    be, orc = SimBackend(lib, mirror, cs, pipeline), Oracle(cache_size=cs)
    trace = lc.run_bounded(be, orc, mirror, cs, lc.bounded_batches(workload, 400, 230, 10, 24), f"{workload} pipeline {pipeline}", per_batch_counters=False)
    k, before, after = lc.assert_crossing_inside(trace, cs, what=workload)
    assert k == 15 and trace[k][0] + 100 == lc.CROSSING and trace[k][2]
    lc.assert_rebuilds_on_both_sides(trace, k)
    st = be.sim.lru_stats()
    assert st["applied"] >= 10 and st["rebuilds"] >= 2, st
    be.close()


@pytest.mark.parametrize("one_call", [True, False], ids=["one_add_of_eleven", "item_by_item"])
def test_cache_operations_pick_the_reference_victims_across_stamp_2_52(lib, one_call):
    """tests/late_counters.py cache_sequence on the kernel source: Add of 11 into a cache of 10 with stamp 2^52 among the eleven, GetItem on the
    oldest survivor, Add of one more"""
    mirror = lc.Mirror(lc.CROSSING - 6)
    be, orc = SimBackend(lib, mirror, 10, slots=1 << 10, max_batch=256), Oracle(cache_size=10)
    lc.cache_sequence(be, orc, mirror, one_call)
    be.close()


def test_the_lrucache_vectors_across_stamp_2_52(lib):
    """tests/golden/cache_vectors.json (lrucache_test.go TestLRUCache, the two eviction cases included) on tables whose second operation takes
    stamp 2^52 - 1: the crossing is inside every case (asserted when the case closes its cache)"""
    def make(cs):
        mirror = lc.Mirror(lc.CROSSING - 2)
        be = SimBackend(lib, mirror, cs or 4096, slots=1 << 14, max_batch=256)
        return lc.CountingCache(be, mirror, on_close=be.close)
    assert scenarios.run_cache_vectors(make, evicting=True) > 3000


def test_a_removed_bucket_that_keeps_late_stamp_bits_is_still_an_empty_bucket(lib):
    """REC_META_MASK: kind, status and algorithm are Rec::meta's low 11 bits, the rest is the stamp.  A TOKEN_BUCKET RESET_REMAINING removes
    the item (algorithms.go:78-90) and the bucket it leaves — kind absent — still gets the request's stamp: at late stamps its meta word is
    not 0.  k_own asks "is this bucket empty?" through rec_meta before it answers a key with the 32-byte record, and the run shortcuts compare
    states through rec_eq: 100 keys created (stamps below 2^52, the high bits 0xfffff), removed (stamp 2^52 among them) and asked for again —
    the oracle's answers, and every key of the last batch served by the short record (an unmasked compare sends all of them the long way)."""
    mirror = lc.Mirror(lc.CROSSING - 150)
    be, orc = SimBackend(lib, mirror, 0, pipeline=1), Oracle(cache_size=1 << 12)
    keys = [f"gone_{i}" for i in range(100)]
    for step, (hits, behavior) in enumerate([(1, 0), (1, support.RESET_REMAINING), (2, 0)]):
        b = HostBatch(keys, hits, 10, 60_000, streams.NOW0 + step, behavior=behavior)
        first = mirror.batch(b.n)[0]
        assert_results_equal(be.eval(b), orc.eval(b), f"step {step} (stamps {first - lc.CROSSING:+d} ..)")
        assert be.totals()[:3] == lc.oracle_totals(orc)[:3] and be.totals()[4] == orc.size() == (0 if step == 1 else 100)
    groups, short_recs, _ = be.sim.part_forms(100)
    assert groups == short_recs == 100, (groups, short_recs)
    be.close()
