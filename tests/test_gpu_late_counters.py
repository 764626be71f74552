"""Engines created with FLAG_TEST_LATE_COUNTERS (gubernator_amd/csrc/guber_test_flags.h): the counters start where production is after
seconds to days — the next recency stamp 4 096 below 2^52 (Rec::pad about to go from 0xffffffff to 0, the high 21 bits in Rec::meta all
about to change), the directory's 31-bit epoch and the claim table's 16-bit epoch 12 below their wraps, the snapshot ring's sequence 8 below
its own.  Every test puts ITS crossing inside its run by arithmetic of its own (tests/late_counters.py: Mirror, advance) and asserts that it
is there; every comparison is exact equality with the bounded-LRU oracle — answers, per-batch aggregates, counters, size, unexpired
evictions.  The CPU twin of the stamp tests (the kernel source on the host) is tests/test_late_counters_cpu.py; the engine's host side —
guber_engine_create's start values, batch_prelude's wrap and defer_hard, the ring's sequence — runs here only.

"Device" memory is torch's; against the CPU build of the engine (GUBER_HIP_LIB = tests/hostsim/libenginesim.so, as
tests/test_enginesim_cpu.py runs other `gpu` files) it is numpy's."""
import ctypes as C

import numpy as np
import pytest

import front_edges as fe
import front_runs as frn
import gubernator_amd as ga
import late_counters as lc
import scenarios
import streams
import support
from support import HostBatch, Oracle

pytestmark = pytest.mark.gpu

LATE = ga.FLAG_TEST_LATE_COUNTERS
ON_CPU_ENGINE = "enginesim" in ga.LIB_PATH


class EngineBackend:
    """tests/late_counters.py's backend over a ga.Engine"""

    def __init__(self, **kw):
        self.e = ga.Engine(**kw)

    def eval(self, b):
        return self.e.eval(b)

    def totals(self):
        return tuple(int(x) for x in self.e.counters())

    def batches(self):
        return self.e.stats()["batches"]

    def rebuilds(self):
        return self.e.stats()["tail_rebuilds"]

    def add_items(self, items, now_ms):
        if now_ms:
            self.e.set_clock(now_ms)
        return self.e.add_items(items)

    def get_item(self, key, now_ms):
        return self.e.get_item(key, now_ms)

    def remove_item(self, key):
        self.e.remove_item(key)

    def close(self):
        assert self.e.stats()["retries"] == 0          # (a retry round would have taken stamps the mirror does not know of)
        self.e.close()


class Device:
    """request columns and result arrays where the kernels read and write them"""

    def __init__(self):
        if ON_CPU_ENGINE:
            self.torch = None
        else:
            import torch
            self.torch, self.dev = torch, torch.device("cuda", 0)

    def put(self, a):
        a = np.ascontiguousarray(a)
        if self.torch is None:
            return a, a.ctypes.data
        t = self.torch.from_numpy(a).to(self.dev)
        return t, t.data_ptr()

    def get(self, t):
        return t if self.torch is None else t.cpu().numpy()

    def synchronize(self):
        if self.torch is not None:
            self.torch.cuda.synchronize(self.dev)

    def batch(self, hb, r=None, full=False):
        """-> (guber_batch_t, guber_result_t, keep-alive): hb's columns (burst / created_at / is_owner when full), result arrays r (numpy:
        copied over) or fresh ones of hb.n"""
        cols = [hb.key_bytes, hb.key_off.view(np.int32), hb.hits, hb.limit, hb.duration, hb.algorithm, hb.behavior.view(np.int32)] + ([hb.burst, hb.created_at, hb.is_owner] if full else [])
        held = [self.put(c) for c in cols]
        p = [h[1] for h in held] + ([] if full else [None, None, None])
        if r is None:
            r = dict(status=np.zeros(hb.n, np.uint8), err=np.zeros(hb.n, np.uint8), limit=np.zeros(hb.n, np.int64), remaining=np.zeros(hb.n, np.int64), reset_time=np.zeros(hb.n, np.int64))
        rt = {k: self.put(v) for k, v in r.items()}
        b = ga.GuberBatch(hb.n, 0, p[0], p[1], p[2], p[3], p[4], p[7], p[8], p[5], p[6], p[9], None, None, hb.now_ms)
        res = ga.GuberResult(rt["status"][1], rt["limit"][1], rt["remaining"][1], rt["reset_time"][1], rt["err"][1], 0, 0, 0, 0, 0)
        return b, res, (held, rt)

    def results(self, keep):
        return {k: self.get(v[0]) for k, v in keep[1].items()}

    def host_result(self, keep, n):
        got = ga.HostResult(n)
        for name, a in self.results(keep).items():
            getattr(got, name)[:] = a[:n]
        return got


# ---- the recency stamp across 2^52 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 32, 2, 64], ids=["default", "two_launch", "radix", "owner_partitioned"])
def test_stamp_2_52_inside_a_small_binding_run_on_every_pipeline(flags):
    """a cache of 300 under 400 keys, batches of 230 keys + 10 touched by every batch (240 requests), 24 steps, the four workloads of
    test_evicted_keys_that_return_meet_the_reference_list with both algorithms: the engine is advanced so that stamp 2^52 is request 100 of
    step 15 (Zipf fills the cache in step 9) — the pre-pass binds on both sides, rebuilds its tail list on both sides of the crossing and holds stamps from
    both sides in one window.  flags 0: a batch whose cache may bind leaves the one-launch path, so this is k_front / k_eval2 over
    host-resident columns (k_small at late stamps: test_the_one_launch_path_stamps_across_2_52); 32: the same pipeline with the one-launch
    path off; 2: the radix pipeline; 64: k_part / k_own / k_eval3."""
    cs, n = 300, 240
    for name in lc.WORKLOADS:
        mirror, orc = lc.Mirror(), Oracle(cache_size=cs)
        be = EngineBackend(cache_size=cs, max_batch=1024, flags=flags | LATE)
        lc.advance(be, mirror, lc.stamps_to_put_crossing_in(mirror, 15, n, 100), streams.NOW0)
        trace = lc.run_bounded(be, orc, mirror, cs, lc.bounded_batches(name, 400, 230, 10, 24), f"flags {flags} {name}")
        k, before, after = lc.assert_crossing_inside(trace, cs, what=name)
        assert k == 15 and trace[k][0] + 100 == lc.CROSSING and trace[k][2]
        lc.assert_rebuilds_on_both_sides(trace, k)
        st = be.e.stats()
        print(f"flags {flags} {name}: crossing in step {k}, binding batches before / after {before} / {after}, eviction passes {st['eviction_passes']}, tail rebuilds {st['tail_rebuilds']}")
        assert st["unexpired_evictions"] == orc.counters()[3] and st["eviction_passes"] >= 10 and st["tail_rebuilds"] >= 1, st
        be.close()


@pytest.mark.parametrize("name", ["cyclic scan", "random walk", "expiring"])
def test_stamp_2_52_inside_the_full_shape(name):
    """the shape of test_evicted_keys_that_return_meet_the_reference_list — a cache of 2 000 under 2 600 keys, batches of 1 550 — with the
    flag alone: the window grows (LRU_MORE) and the device sorts thousands of stamps that lie on both sides of 2^52.  Where the crossing
    can be is arithmetic: the engine starts 4 096 stamps below it and a cache of 2 000 binds only after 2 000 of them, so stamp 2^52 is
    request 996 of step 2, and five binding batches of 1 550 before it would need 2 000 + 5 x 1 550 stamps — the cache binds from the
    crossing on (the cyclic scan: from step 1), the first victims being the items with the stamps below 2^52; the small shape above has its
    five batches on both sides.  (Three of that test's four workloads, 12 steps each: Zipf over 2 600 keys does not fill this cache in the
    stamps there are.)"""
    cs, n = 2000, 1550
    mirror, orc = lc.Mirror(), Oracle(cache_size=cs)
    be = EngineBackend(cache_size=cs, max_batch=2048, flags=LATE)
    trace = lc.run_bounded(be, orc, mirror, cs, lc.bounded_batches(name, 2600, 1500, 50, 12, seed=5), f"full shape {name}", witness="list" if name == "expiring" else "unexpired")
    k, before, after = lc.assert_crossing_inside(trace, cs, each_side=0, what=name)
    assert k == 2 and trace[k][0] + 996 == lc.CROSSING and after >= 9 and trace[k][2], (k, before, after, trace[k])
    st = be.e.stats()
    print(f"full shape {name}: binding batches before / after {before} / {after}, eviction passes {st['eviction_passes']}, tail rebuilds {st['tail_rebuilds']}")
    assert st["unexpired_evictions"] == orc.counters()[3] and st["eviction_passes"] >= 9 and st["tail_rebuilds"] >= 1, st
    be.close()


def test_the_one_launch_path_stamps_across_2_52():
    """k_small writes the stamps: five batches of 50 new keys into a cache of 300 that they cannot make bind — the one-launch path, asserted
    from small_batches — with stamp 2^52 request 20 of the third; then batches of 120 new keys bind and the victims are those keys in the
    order k_small stamped them, element-wise the oracle's."""
    cs = 300
    mirror, orc = lc.Mirror(), Oracle(cache_size=cs)
    be = EngineBackend(cache_size=cs, max_batch=1024, flags=LATE)
    lc.advance(be, mirror, lc.stamps_to_put_crossing_in(mirror, 2, 50, 20), streams.NOW0)
    small0 = be.e.stats()["small_batches"]                        # (stats: the host's bound of the size is exact again)
    now = streams.NOW0
    fill = [HostBatch([f"one_{s}_{i}" for i in range(50)][::-1], 1, 100, 3_600_000, now + s, algorithm=np.arange(50) & 1) for s in range(5)]
    trace = lc.run_bounded(be, orc, mirror, cs, fill, "one-launch fill")
    assert lc.crossing_step(trace) == 2 and trace[2][0] + 20 == lc.CROSSING
    assert be.e.stats()["small_batches"] == small0 + 5
    more = [HostBatch([f"more_{s}_{i}" for i in range(120)], 1, 100, 3_600_000, now + 10 + s) for s in range(3)]
    lc.run_bounded(be, orc, mirror, cs, more, "binding after the one-launch fill")
    probe = HostBatch([f"one_{s}_{i}" for s in range(5) for i in range(50)], 0, 100, 3_600_000, now + 20)
    support.assert_results_equal(be.eval(probe), orc.eval(probe), "who is left")
    assert be.totals() == lc.oracle_totals(orc) and orc.counters()[3] >= 250
    be.close()


def test_an_invalid_algorithm_request_does_not_refresh_recency_at_late_stamps():
    """test_an_invalid_algorithm_request_does_not_refresh_recency's batches (a third of the requests with an algorithm the reference rejects
    before GetItem, whole keys' runs among them: the bucket keeps the stamp of its last VALID request) through k_part / k_own / k_eval3 with
    stamp 2^52 request 50 of step 8 of 20 — batches of 500 requests, not that test's 700: the cache binds from step 2 on, and two batches
    that fill it and five of 700 that bind do not fit into the 4 096 stamps below the crossing"""
    cs, n = 600, 500
    mirror, orc = lc.Mirror(), Oracle(cache_size=cs)
    be = EngineBackend(cache_size=cs, max_batch=2048, flags=64 | LATE)
    lc.advance(be, mirror, lc.stamps_to_put_crossing_in(mirror, 8, n, 50), streams.NOW0)
    rng = np.random.default_rng(21)

    def batches():
        now = streams.NOW0
        for step in range(20):
            ids = rng.integers(0, 900, n)
            algo = (ids & 1).astype(np.uint8)
            bad = rng.random(n) < 0.3
            if step % 4 == 1:
                bad |= ids % 3 == 0
            algo[bad] = lc.INVALID_ALGORITHM
            yield HostBatch([f"inv_{int(i)}" for i in ids], 1, 40, 3_600_000, now, algorithm=algo)
            now += 500
    trace = lc.run_bounded(be, orc, mirror, cs, batches(), "invalid algorithm")
    k, before, after = lc.assert_crossing_inside(trace, cs)
    assert k == 8
    assert be.e.stats()["unexpired_evictions"] == orc.counters()[3] > 0
    be.close()


# ---- cache operations --------------------------------------------------------------------------------------------------------------
def test_lrucache_vectors_across_stamp_2_52():
    """tests/golden/cache_vectors.json (lrucache_test.go TestLRUCache, the eviction cases included) through guber_add_items / guber_get_item /
    guber_remove_item on engines advanced to two stamps below 2^52: the crossing is inside every case (asserted when the case closes)"""
    def make(cs):
        mirror = lc.Mirror()
        be = EngineBackend(cache_size=cs or 4096, max_batch=1024, flags=LATE)
        lc.advance(be, mirror, lc.CROSSING - 2 - mirror.seq, streams.NOW0, chunk=1024 if not cs else cs // 2, exact=False)     # (half the cache per batch: no pieces)
        return lc.CountingCache(be, mirror, on_close=be.close)
    assert scenarios.run_cache_vectors(make, evicting=True) > 3000


@pytest.mark.parametrize("one_call", [True, False], ids=["one_add_of_eleven", "item_by_item"])
def test_add_and_get_pick_the_reference_victims_across_stamp_2_52(one_call):
    """tests/late_counters.py cache_sequence: Add of 11 items into a cache of 10 with stamp 2^52 among the eleven (the host's rec_set_stamp,
    k_items_commit, the pre-pass without requests), GetItem on the oldest survivor (k_item_lookup), Add of one more — the victims are the
    reference's"""
    mirror, orc = lc.Mirror(), Oracle(cache_size=10)
    be = EngineBackend(cache_size=10, max_batch=1024, flags=LATE)
    lc.advance(be, mirror, lc.CROSSING - 6 - mirror.seq, streams.NOW0, chunk=1024, exact=False)
    lc.cache_sequence(be, orc, mirror, one_call)
    be.close()


class Plain:
    """tests/late_counters.py advance's backend over an engine somebody else owns"""

    def __init__(self, e):
        self.eval, self.totals, self.batches = e.eval, lambda: tuple(e.counters()), lambda: e.stats()["batches"]


# ---- the epochs ----------------------------------------------------------------------------------------------------------------------
def check_keys(e, orc, keys, now):
    for k in keys:
        a, g = orc.get_item(k, now), e.get_item(k, now)
        assert a is not None and g is not None and (a["remaining"], a["remaining_f"], a["status"]) == (g["remaining"], g["remaining_f"], g["status"]), (k, a, g)


def wrap_index(flags_per_batch):
    """the one batch that wrapped, with at least five batches on each side of it"""
    at = [i for i, w in enumerate(flags_per_batch) if w]
    assert len(at) == 1 and at[0] >= 5 and len(flags_per_batch) - 1 - at[0] >= 5, at
    return at[0]


def test_the_directory_epoch_wraps_under_the_radix_pipeline():
    """batch_prelude: the 12th batch of a flagged engine takes the directory's 31-bit epoch over 0x7fffffff — k_clear_claims runs and the
    epoch restarts at 1.  40 batches of 300 requests over 40 keys (duplicates in every batch) through k_resolve / k_scatter / k_heads /
    k_eval, the cache not binding: keys inserted before the wrap are found after it (k_clear_claims keeps META_READY), and the wrap batch
    itself — dense ids claimed under epoch 1 over entries last claimed near 2^31 — groups every key's requests right."""
    mirror, orc = lc.Mirror(), Oracle(cache_size=1 << 12)
    e = ga.Engine(cache_size=1 << 12, max_batch=1024, flags=2 | LATE)
    wrapped = []
    for s, b in enumerate(lc.duplicate_batches(40, 300, 40, seed=31)):
        wrapped.append(mirror.batch(b.n)[1])
        got, want = e.eval(b), orc.eval(b)
        support.assert_results_equal(got, want, f"batch {s}" + (" (the wrap)" if wrapped[-1] else ""))
        assert got.counters() == want.counters(), (s, got.counters(), want.counters())
    assert wrap_index(wrapped) == 11
    st = e.stats()
    assert st["batches"] == 40 and st["retries"] == 0 and st["small_batches"] == 0, st      # one epoch per batch: the mirror's arithmetic is the engine's
    check_keys(e, orc, [b"wrap_%d" % i for i in range(40)], streams.NOW0 + 40 * 50)
    assert e.size() == orc.size() == 40
    e.close()


def test_a_fused_group_lets_go_of_its_held_back_evaluation_at_the_epoch_wrap():
    """defer_hard: three engines on one stream, 20 rounds of one batch each — 60 routed batches — (1 024 .. 1 300 requests: the owner-partitioned pipeline, fused)
    in ONE guber_eval_batches_routed_dev call.  From the second round on the group's k_eval3 is held back for the next round's k_part
    (k_evalpart_multi); the prelude that would wrap the directory epoch has a launch to enqueue (k_clear_claims), so it says defer and the
    held-back evaluation is launched first.  Engine 2 has taken five batches more, so the wraps come in rounds 6 (engine 2) and 11 (engines
    0, 1).  Every batch equals its engine's oracle; nothing retried; the groups were fused.  What this test can and cannot see: it RUNS the
    wrap under fused groups with an evaluation held back, and fails if that corrupts an answer, a counter or the directory.  It cannot tell
    whether the detour was taken: no statistic says so, and only the radix kernels read the directory epoch, so k_clear_claims ahead of a
    held-back k_eval3 changes nothing that the owner-partitioned kernels read — without the defer_hard check the answers are the same."""
    dv = Device()
    n_engines, rounds, K = 3, 20, 800
    e0 = ga.Engine(cache_size=1 << 16, max_batch=4096, flags=LATE)
    engs = [e0] + [ga.Engine(cache_size=1 << 16, max_batch=4096, stream=e0.stream_handle(), flags=LATE) for _ in range(n_engines - 1)]
    orcs = [Oracle(cache_size=1 << 16) for _ in engs]
    mirrors = [lc.Mirror() for _ in engs]

    assert lc.advance(Plain(engs[2]), mirrors[2], 5 * 300, streams.NOW0, chunk=300, epochs=True) == 5
    rng = np.random.default_rng(13)
    zs = [streams.ZipfSampler(K, seed=200 + j) for j in range(n_engines)]
    which, hbs, keep, cb, cr, wrapped = [], [], [], [], [], [[] for _ in engs]
    for r in range(rounds):
        for j in range(n_engines):
            n = 1024 + int(rng.integers(0, 277))
            ids = zs[j].draw(n)
            hb = HostBatch([b"dh%d_%d" % (j, int(i)) for i in ids], rng.integers(0, 3, n), 60, 4000, streams.NOW0 + r * 700, algorithm=(ids & 1).astype(np.uint8))
            b, res, k = dv.batch(hb)
            which.append(j); hbs.append(hb); keep.append(k); cb.append(b); cr.append(res)
            wrapped[j].append(mirrors[j].batch(n)[1])
    assert [wrap_index(w) for w in wrapped] == [11, 11, 6]
    dv.synchronize()
    N = len(which)
    ga.Engine.eval_routed_dev(engs, (C.c_uint32 * N)(*which), (ga.GuberBatch * N)(*cb), (ga.GuberResult * N)(*cr), N)
    for e in engs:
        e.synchronize()
    sums = [[0, 0, 0] for _ in engs]
    for s in range(N):
        want = orcs[which[s]].eval(hbs[s])
        support.assert_results_equal(dv.host_result(keep[s], hbs[s].n), want, f"round {s // n_engines} engine {which[s]}")
        for q in range(3):
            sums[which[s]][q] += want.counters()[q]
    stats = [e.stats() for e in engs]
    assert sum(st["fused_batches"] for st in stats) > 0 and all(st["retries"] == 0 for st in stats), stats
    assert [st["batches"] for st in stats] == [rounds, rounds, rounds + 5], stats              # one epoch per batch: the mirror's arithmetic is the engine's
    for j, (e, o) in enumerate(zip(engs, orcs)):
        assert list(e.counters()[:3]) == sums[j] and e.size() == o.size(), (j, e.counters(), sums[j])
    for e in reversed(engs):
        e.close()


@pytest.mark.parametrize("entry", ["eval", "stages", "routed"])
def test_the_claim_epoch_wraps_on_every_way_into_the_two_launch_pipeline(entry):
    """plan_fast: the 13th two-launch batch of a flagged engine takes the claim table's 16-bit epoch over 0xffff — the table and the segment
    records' epoch-tagged flag words are wiped and the epoch restarts at 1.  40 batches of 300 requests over 40 keys per engine with the
    one-launch path off (flags 32): through guber_eval_batch; through guber_stages_submit with two stages in flight; through
    guber_eval_batches_routed_dev on two engines of one stream (k_front_multi / k_eval2_multi).  The cheap complement of
    test_claim_table_epoch_wraps' 66 500 batches, and the wrap's only run under stage and routed submissions."""
    n_engines = 2 if entry == "routed" else 1
    e0 = ga.Engine(cache_size=1 << 12, max_batch=1024, flags=32 | LATE)
    engs = [e0] + [ga.Engine(cache_size=1 << 12, max_batch=1024, stream=e0.stream_handle(), flags=32 | LATE) for _ in range(n_engines - 1)]
    orcs, mirrors = [Oracle(cache_size=1 << 12) for _ in engs], [lc.Mirror() for _ in engs]
    runs = [list(lc.duplicate_batches(40, 300, 40, seed=41 + j, prefix=b"claim%d" % j)) for j in range(n_engines)]
    wrapped = [[mirrors[j].batch(b.n)[2] for b in runs[j]] for j in range(n_engines)]
    assert [wrap_index(w) for w in wrapped] == [12] * n_engines
    if entry == "eval":
        for s, b in enumerate(runs[0]):
            got, want = e0.eval(b), orcs[0].eval(b)
            support.assert_results_equal(got, want, f"batch {s}")
            assert got.counters() == want.counters(), (s, got.counters(), want.counters())
    elif entry == "stages":
        stages = [ga.Stage(e0, 1024, key_bytes_cap=1024 * 24) for _ in range(2)]
        pending = None
        for s, b in enumerate(runs[0] + [None]):
            if b is not None:
                stages[s % 2].fill(b)
                assert ga.Stage.submit_many([stages[s % 2]]) == 1                           # guber_stages_submit; the previous stage is still in flight
            if pending is not None:
                pst, phb, ps = pending
                pst.wait()
                support.assert_results_equal(pst.result(), orcs[0].eval(phb), f"stage batch {ps}")
            pending = (stages[s % 2], b, s) if b is not None else None
        for st in stages:
            st.close()
    else:
        dv = Device()
        which, hbs, keep, cb, cr = [], [], [], [], []
        for s in range(40):
            for j in range(n_engines):
                b, res, k = dv.batch(runs[j][s])
                which.append(j); hbs.append(runs[j][s]); keep.append(k); cb.append(b); cr.append(res)
        dv.synchronize()
        N = len(which)
        ga.Engine.eval_routed_dev(engs, (C.c_uint32 * N)(*which), (ga.GuberBatch * N)(*cb), (ga.GuberResult * N)(*cr), N)
        for e in engs:
            e.synchronize()
        for s in range(N):
            support.assert_results_equal(dv.host_result(keep[s], hbs[s].n), orcs[which[s]].eval(hbs[s]), f"round {s // n_engines} engine {which[s]}")
        assert sum(e.stats()["fused_batches"] for e in engs) > 0
    for j, e in enumerate(engs):
        st = e.stats()
        assert st["batches"] == 40 and st["retries"] == 0 and st["small_batches"] == 0 and st["cache_size"] == orcs[j].size() == 40, st
        assert tuple(e.counters()[:3]) == tuple(orcs[j].counters()[:3])
        check_keys(e, orcs[j], [b"claim%d_%d" % (j, i) for i in range(40)], streams.NOW0 + 40 * 50)
    for e in reversed(engs):
        e.close()


@pytest.mark.timeout(30)
def test_the_snapshot_rings_sequence_wraps_under_synchronous_snapshots():
    """rb_seq under the snapshots of the RESERVED slot only (the host synchronises and never looks at their number: this test runs the wrap's
    expression and the counters around it, it cannot fail on the number — test_the_rings_sequence_wraps_on_an_armed_slot can): every counter
    snapshot takes the next 32-bit sequence number — 0 means "none", so the wrap skips it.  40 batches over a cache that is nowhere near binding, 200 requests (the
    one-launch path: no snapshot) and 300 (the host entry's read-back: one) in turn, and ONE guber_stats per batch (one more): by that
    arithmetic the 9th snapshot — the wrap — is taken in batch 5.  counters() and the size equal the oracle's after every batch, and no
    call waits for a number that never comes (the test's time limit; a hang here is a finding)."""
    mirror, orc = lc.Mirror(), Oracle(cache_size=1 << 12)
    e = ga.Engine(cache_size=1 << 12, max_batch=1024, flags=LATE)
    rng = np.random.default_rng(51)
    keys = [b"ring_%d" % i for i in range(40)]
    wrapped = []
    for s in range(40):
        n = 300 if s % 2 else 200
        ids = rng.integers(0, 40, n)
        hits = rng.integers(0, 3, n) if n > 256 else 1                  # (the one-launch path declines requests of one key that differ)
        b = HostBatch([keys[i] for i in ids], hits, 400, 3_600_000, streams.NOW0 + s * 50, algorithm=(ids & 1).astype(np.uint8))
        w = [mirror.snapshot() for _ in range((1 if n > 256 else 0) + 1)]
        wrapped.append(any(w))
        got, want = e.eval(b), orc.eval(b)
        support.assert_results_equal(got, want, f"batch {s}")
        st = e.stats()
        assert (st["over_limit_count"], st["cache_hits"], st["cache_misses"], st["unexpired_evictions"], st["cache_size"]) == lc.oracle_totals(orc), (s, st, lc.oracle_totals(orc))
    assert wrap_index(wrapped) == 5
    assert st["small_batches"] == 20 and st["batches"] == 40 and st["retries"] == 0, st       # (which path each batch took: the arithmetic's premise)
    e.close()


@pytest.mark.timeout(30)
@pytest.mark.parametrize("entry", ["riding", "launched"])
def test_the_rings_sequence_wraps_on_an_armed_slot(entry):
    """rb_seq on a RING slot: the host knows that a snapshot is complete by finding the slot's sequence number in host memory, and 0 means
    "none" — to the kernels (Work::snap_seq) and to memory nobody has written yet.  So the wrap must skip 0, and here it lands on a slot
    the host is going to believe: a cache of 1 000 filled to 800 by 80 one-launch batches of 10 new keys (never near the size: no snapshot),
    eight guber_stats (eight snapshots into the reserved slot), and then the batch W of 20 requests for resident keys — near the size but
    not binding, so maintain() arms the FIRST ring slot ever, with the 9th sequence number, the wrap.  riding: W is device-resident and
    k_front carries the snapshot; launched: W takes the one-launch path and the snapshot is a launch of its own ahead of it.  The next
    batch X (250 new keys, then the 150 oldest) binds only if the host's bound still knows about the 800 items: a slot that read as complete
    without having been written would put the bound at 20, X would skip the eviction pre-pass and the oldest keys would be hits where the
    reference has evicted them.  Six more binding batches follow; answers, counters and size equal the oracle's; nothing waits for a
    number that never comes (the time limit)."""
    cs, now = 1000, streams.NOW0
    dv = Device() if entry == "riding" else None
    mirror, orc = lc.Mirror(), Oracle(cache_size=cs)
    e = ga.Engine(cache_size=cs, max_batch=1024, flags=LATE)

    def run(b, what):
        want = orc.eval(b)
        if dv is None:
            got = e.eval(b)
            assert got.counters() == want.counters(), (what, got.counters(), want.counters())
        else:
            cb, cr, keep = dv.batch(b)
            dv.synchronize()
            e.eval_dev(cb, cr)
            e.synchronize()
            got = dv.host_result(keep, b.n)
        support.assert_results_equal(got, want, what)
    for s in range(80):                                               # 800 items, no snapshot: 16 x 10 + 10 + what is there never reaches 1 000
        b = HostBatch([f"ring_{s * 10 + i}" for i in range(10)], 1, 50, 3_600_000, now + s)
        support.assert_results_equal(e.eval(b), orc.eval(b), f"fill {s}")
    wrapped = []
    for _ in range(8):
        st = e.stats()
        wrapped.append(mirror.snapshot())
    assert st["small_batches"] == st["batches"] == 80 and st["cache_size"] == 800, st     # (the fill took the one-launch path: the arithmetic's premise)
    # W: 800 + 20 + min(16 x 20, 500) > 1 000 is near, 800 + 20 is not binding: one ring slot armed
    wrapped.append(mirror.snapshot())
    assert wrapped == [False] * 8 + [True]
    run(HostBatch([f"ring_{780 + i}" for i in range(20)], 1, 50, 3_600_000, now + 100), "W (the wrap's snapshot)")
    pos = 0
    for s in range(7):                                                # X and six more: 250 new keys, then the 150 oldest left
        keys = [f"late_{s}_{i}" for i in range(250)] + [f"ring_{(pos + i) % 800}" for i in range(150)]
        pos += 150
        run(HostBatch(keys, 1, 50, 3_600_000, now + 200 + s), f"binding batch {s} after the wrap")
    assert tuple(int(x) for x in e.counters()) == lc.oracle_totals(orc) and orc.size() == cs and orc.counters()[3] >= 7 * 250 - 200
    assert e.stats()["retries"] == 0 and e.stats()["eviction_passes"] >= 7
    e.close()


# ---- the front ---------------------------------------------------------------------------------------------------------------------------
def test_the_fronts_runs_over_engines_past_stamp_2_52():
    """tests/front_runs.py's generations of up to three tiles (every plan and key width at sizes 1 .. 2 049: 64 of its 72; the largest size runs
    in tests/test_gpu_front_runs.py) through a front of four flagged engines over caches of 96 items
    that bind, against ONE oracle with four workers.  An engine's share of a generation takes as many stamps as it has requests — counted
    here from the plans — so every engine hands out stamp 2^52 inside the run (the generations' sizes grow, so an engine that would not have crossed by
    generation 44 is advanced first and crosses with its first request after that; the others cross earlier by themselves).  Binding on both
    sides is counted per engine from guber_stats_t.eviction_passes, sampled whenever the driver asks for the next generation: at least five
    eviction pre-passes that applied evictions before the generation with the crossing is handed in, and five after it has been answered."""
    dv = Device()
    n_engines = 4
    rng = np.random.default_rng(2604)
    place = ga.Placement(n_engines)
    e0 = ga.Engine(cache_size=frn.CACHE_PER_ENGINE, max_batch=8192, flags=LATE)
    e2 = ga.Engine(cache_size=frn.CACHE_PER_ENGINE, max_batch=8192, flags=LATE)
    engs = [e0, ga.Engine(cache_size=frn.CACHE_PER_ENGINE, max_batch=8192, stream=e0.stream_handle(), flags=LATE),
            e2, ga.Engine(cache_size=frn.CACHE_PER_ENGINE, max_batch=8192, stream=e2.stream_handle(), flags=LATE)]       # two streams, as test_gpu_front_runs has them
    fr = ga.Front(engs, place, max_n=max(frn.SIZES), depth=3)
    orc = Oracle(cache_size=frn.CACHE_PER_ENGINE * n_engines, workers=n_engines)
    route = lambda keys: place.route_keys(*fe.pack(keys))[0]
    gens = [g for g in frn.generations(n_engines, route, rng, depth=3) if g[1].n <= 2049]      # (every plan at the sizes up to three tiles: 64 generations)
    shares = np.array([np.bincount(engines, minlength=n_engines) for _, _, _, engines in gens])     # the stamps every engine takes per generation
    mirrors = [lc.Mirror() for _ in engs]
    T = 44                                                             # (the sizes grow: the first 44 generations hold a quarter of the requests)
    for j, e in enumerate(engs):                                       # an engine that has not crossed by generation T does so with its first request after it
        lc.advance(Plain(e), mirrors[j], max(0, lc.CROSSING - 1 - int(shares[:T, j].sum()) - mirrors[j].seq), streams.NOW0, chunk=64)

    def device_side(hb, full, r):
        b, res, keep = dv.batch(hb, r, full)
        dv.synchronize()
        return b, res, keep
    passes = []                                                        # passes[t][j]: engine j's eviction passes when generation t is asked for (those before it: answered or not yet handed in)

    def sampled():
        for gen in gens:
            passes.append([e.stats()["eviction_passes"] for e in engs])
            yield gen
    count = frn.drive(engs, fr, orc, sampled(), device_side, dv.results)
    assert count == len(gens) == 8 * (1 + len(frn.PLANS))
    passes.append([e.stats()["eviction_passes"] for e in engs])
    for j in range(n_engines):
        taken = mirrors[j].seq + np.cumsum(shares[:, j])               # engine j's next stamp after every generation
        g = int(np.searchsorted(taken, lc.CROSSING, side="right"))     # the generation in which it hands out stamp 2^52
        assert 0 < g < count - 5, (j, g)
        before = passes[g][j]                                          # applied by generations before g (a call holds at most depth + 1 = 4 generations:
        after = passes[count][j] - passes[g + 4][j]                    #  when generation g + 4 is asked for, g has been answered)
        print(f"front engine {j}: stamp 2^52 in generation {g} of {count}, eviction passes before / after {before} / {after}")
        assert before >= 5 and after >= 5, (j, g, before, after)
    fr.close()
    for e in (engs[1], engs[3], e0, e2):
        e.close()
    place.close()
    orc.close()
