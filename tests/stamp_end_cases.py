"""The END of the 53-bit recency stamp (GUBER_FLAG_TEST_LAST_STAMPS, gubernator_amd/csrc/guber_test_flags.h): an engine created with the flag
starts 4 096 stamps below 2^53, and the call that would hand out a stamp above 2^53 - 1 first renumbers the live items' stamps 1..live in
their order (engine_batch.inl stamps_ensure, k_lru_renumber) — without it stamp 2^53 is written as 0, the newest item looks like the oldest
and the wrong items are evicted.  The driver of tests/test_gpu_stamp_end.py (the product library on a GPU) and tests/test_stamp_end_cpu.py
(the CPU build of the engine, tests/hostsim/enginesim.cpp: this file run as a script); numpy only — the GPU test brings torch's memory.

Every comparison is exact equality with the bounded-LRU oracle (support.Oracle): answers, per-batch aggregates, totals, the size after
every batch.  Every case POSITIONS its renumbering by arithmetic of its own (late_counters.Mirror counts what the engine hands out) and
asserts through Engine.recency_info() that it happened where intended: renumbers 0 before the call and 1 after it, and after that call
next_stamp = the live items before the call + 1 + the stamps the call took.

  pipelines      every batch pipeline (flags 0, 32, 2, 64): a cache of 300 under 400 keys, batches of 240, the call of step 15 of 24 is the
                 first whose stamps do not fit; the reference evicts in at least five batches on both sides; tail_rebuilds rises by one
  cache ops      Add of 11 into a cache of 10 in one call and item by item, GetItem, one more Add: the reference's victims;
                 guber_add_items_dev, guber_get_item and guber_remove_item as the call that renumbers
  one launch     k_small: the renumbering call is a batch of 50 on the one-launch path; an empty table
  fused          guber_eval_batches_routed_dev over four engines of one stream, GUBER_FUSE_EP: two engines reach the end in different rounds
                 inside ONE call (defer_hard: the evaluation held back is launched first)
  front          guber_front_eval_dev, four tables, one call of six generations of 1 024: the end inside the call for two tables
  moved in       65 buckets moved from another engine, then the destination driven over the end: every live item kept, Each() the oracle's"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)                          # (run as a script: the package is importable from the repository tree)

import cache_ops_cases as co
import front_edges as fe
import late_counters as lc
import streams
import support
from late_counters import Mirror, WORKLOADS, advance, bounded_batches, recency_items, run_bounded
from support import HostBatch, Oracle

FLAG = 1024                                  # gubernator_amd.FLAG_TEST_LAST_STAMPS
END = 1 << 53                                # one past the last stamp (REC_STAMP_MASK + 1)
SEQ_NEXT = END - 4096                        # GUBER_TEST_LAST_SEQ_NEXT
PIPELINES = ((0, "default"), (32, "two_launch"), (2, "radix"), (64, "owner_partitioned"))
NOW = streams.NOW0


def _ga():
    import gubernator_amd as ga
    return ga


def header_values():
    """the flag and the start value as gubernator_amd/csrc/guber_test_flags.h spells them"""
    import re
    text = open(os.path.join(support.ROOT, "gubernator_amd", "csrc", "guber_test_flags.h")).read()
    out = {}
    for name in ("GUBER_FLAG_TEST_LAST_STAMPS", "GUBER_TEST_LAST_SEQ_NEXT"):
        expr = re.search(r"^#define %s\s+(.+?)\s*(?:/\*|$)" % name, text, re.M).group(1)
        assert re.fullmatch(r"[0-9a-fxulUL()<\-+ ]+", expr), expr
        out[name] = eval(re.sub(r"(?<=[0-9a-f])(?:ull|u)\b", "", expr, flags=re.I))
    return out


class EngineBackend:
    """late_counters.py's backend over a gubernator_amd.Engine, with the engine's place in its stamps"""

    def __init__(self, **kw):
        self.e = _ga().Engine(**kw)

    def eval(self, b):
        return self.e.eval(b)

    def totals(self):
        return tuple(int(x) for x in self.e.counters())

    def batches(self):
        return self.e.stats()["batches"]

    def rebuilds(self):
        return self.e.stats()["tail_rebuilds"]

    def size(self):
        return self.e.size()

    def recency(self):
        return self.e.recency_info()

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


class Plain:
    """advance's backend over an engine somebody else owns"""

    def __init__(self, e):
        self.eval, self.totals, self.batches = e.eval, lambda: tuple(e.counters()), lambda: e.stats()["batches"]


class Device:
    """request columns and result arrays where the kernels read and write them: numpy's memory for the CPU build of the engine, otherwise
    what the caller brings (put(array) -> (keep-alive, pointer), get(keep-alive) -> array, synchronize())"""

    def put(self, a):
        a = np.ascontiguousarray(a)
        return a, a.ctypes.data

    def get(self, t):
        return t

    def synchronize(self):
        pass

    def batch(self, hb, full=False):
        ga = _ga()
        cols = [hb.key_bytes, hb.key_off.view(np.int32), hb.hits, hb.limit, hb.duration, hb.algorithm, hb.behavior.view(np.int32)] + ([hb.burst, hb.created_at, hb.is_owner] if full else [])
        held = [self.put(c) for c in cols]
        p = [h[1] for h in held] + ([] if full else [None, None, None])
        r = dict(status=np.zeros(hb.n, np.uint8), err=np.zeros(hb.n, np.uint8), limit=np.zeros(hb.n, np.int64), remaining=np.zeros(hb.n, np.int64), reset_time=np.zeros(hb.n, np.int64))
        rt = {k: self.put(v) for k, v in r.items()}
        b = ga.GuberBatch(hb.n, 0, p[0], p[1], p[2], p[3], p[4], p[7], p[8], p[5], p[6], p[9], None, None, hb.now_ms)
        res = ga.GuberResult(rt["status"][1], rt["limit"][1], rt["remaining"][1], rt["reset_time"][1], rt["err"][1], 0, 0, 0, 0, 0)
        return b, res, (held, rt)

    def host_result(self, keep, n):
        got = _ga().HostResult(n)
        for name, v in keep[1].items():
            getattr(got, name)[:] = np.asarray(self.get(v[0]))[:n]
        return got


# ---- positioning ---------------------------------------------------------------------------------------------------------------------
def advance_to(be, mirror, seq, chunk=200, exact=True):
    """hand out stamps (and nothing else) until the engine's next stamp is `seq`; the engine agrees with the mirror"""
    advance(be, mirror, seq - mirror.seq, NOW, chunk=chunk, exact=exact)
    assert mirror.seq == seq


class Renumbering:
    """the assertions around the ONE call that renumbers: before(n) right before a call that takes n stamps, after() right behind it"""

    def __init__(self, recency, size, what):
        self.recency, self.size, self.what = recency, size, what

    def fits(self, n):
        """a call before the end: its n stamps fit and nothing has been renumbered"""
        r = self.recency()
        assert r["renumbers"] == 0 and r["next_stamp"] + n <= END, (self.what, r, n)

    def before(self, n, next_stamp=None):
        r = self.recency()
        assert r["renumbers"] == 0 and r["next_stamp"] <= END < r["next_stamp"] + n, (self.what, r, n)
        if next_stamp is not None:
            assert r["next_stamp"] == next_stamp, (self.what, r, next_stamp - END)
        self.live, self.n = self.size(), n

    def after(self):
        r = self.recency()
        assert r["renumbers"] == 1 and r["last_live"] == self.live and r["next_stamp"] == self.live + 1 + self.n, (self.what, r, self.live, self.n)
        return r


def watched(batches, rn, mirror, k, entry=None):
    """the batches of a run with the renumbering's assertions around batch k (the one after it asks for: batch k + 1, or the run's end)"""
    for step, b in enumerate(batches):
        if step < k:
            rn.fits(b.n)
        elif step == k:
            rn.before(b.n, entry)
        elif step == k + 1:
            mirror.seq = rn.after()["next_stamp"]
        yield b
    if step == k:
        mirror.seq = rn.after()["next_stamp"]


# ---- 1 and 7: every pipeline; the binding run goes on over the list the renumbering left ---------------------------------------------------
def case_pipeline(flags, names=WORKLOADS, make=EngineBackend):
    """a cache of 300 under 400 keys, batches of 230 keys + 10 touched by every batch (240 requests), 24 steps, the four workloads with both
    algorithms — the shapes tests/test_gpu_late_counters.py runs across 2^52.  The engine is advanced so that its next stamp is 100 below
    2^53 when step 15 is called: the first call whose 240 stamps do not fit.  The reference evicts in at least five batches before that step
    and five after it (evicted_unasked); the triggering call builds the tail list once — the renumbering's — and its own pre-pass uses it."""
    cs, n, k = 300, 240, 15
    for name in names:
        mirror, orc = Mirror(seq=SEQ_NEXT), Oracle(cache_size=cs)
        be = make(cache_size=cs, max_batch=1024, flags=flags | FLAG)
        advance_to(be, mirror, END - 100 - k * n)
        rn = Renumbering(be.recency, be.size, f"flags {flags} {name}")
        trace = run_bounded(be, orc, mirror, cs, watched(bounded_batches(name, 400, 230, 10, 24), rn, mirror, k, END - 100), f"flags {flags} {name}")
        binds = [t[2] for t in trace]
        assert trace[k][0] == END - 100 and sum(binds[:k]) >= 5 and sum(binds[k + 1:]) >= 5 and binds[k], (name, binds)
        assert trace[k][3] - trace[k - 1][3] == 1, (name, [t[3] for t in trace])       # one rebuild for the renumbering AND the call's pre-pass
        st = be.e.stats()
        print(f"flags {flags} {name}: renumbered before step {k} ({rn.live} live), binding batches before / after {sum(binds[:k])} / {sum(binds[k + 1:])}, eviction passes {st['eviction_passes']}, tail rebuilds {st['tail_rebuilds']}")
        assert st["unexpired_evictions"] == orc.counters()[3] and st["eviction_passes"] >= 10, st
        assert be.recency()["renumbers"] == 1
        be.close()
        orc.close()


# ---- 2: cache operations ---------------------------------------------------------------------------------------------------------------
def cache_engine(cs, seq, make=EngineBackend):
    mirror, orc = Mirror(seq=SEQ_NEXT), Oracle(cache_size=cs)
    be = make(cache_size=cs, max_batch=1024, flags=FLAG)
    advance_to(be, mirror, seq, chunk=1024, exact=False)                             # (pieces or not: they take the batch's stamps, no more)
    return be, orc, mirror


def survivors(be, orc, names, now):
    """GetItem on every name, in the same order on both sides (it moves what it finds) -> the names that are left"""
    left = []
    for k in names:
        a, g = orc.get_item(k, now), be.get_item(k, now)
        assert (a is None) == (g is None), (k, a, g)
        if a is not None:
            assert (a["remaining"], a["algorithm"], a["status"]) == (g["remaining"], g["algorithm"], g["status"]), (k, a, g)
            left.append(k)
    return left


def case_cache_sequence(one_call, make=EngineBackend):
    """late_counters.cache_sequence's shape at the end of the stamps: Add of 11 items into a cache of 10 with the engine's next stamp 2^53 - 6
    on entry.  One call of 11 renumbers before the call (an empty table: the eleven get 1..11); item by item the seventh Add renumbers (six live
    items get 1..6, the seventh 7).  The victims are the reference's: item 0, and after GetItem on item 1 and one more Add, item 2."""
    be, orc, mirror = cache_engine(10, END - 6, make)
    rn = Renumbering(be.recency, be.size, f"cache sequence one_call={one_call}")
    names = [f"seq_{i}" for i in range(12)]
    items = recency_items(names, NOW)
    for it in items[:11]:
        orc.add_item(it, NOW)
    if one_call:
        rn.before(11, END - 6)
        assert be.add_items(items[:11], NOW) == [False] * 11
        assert rn.live == 0
        rn.after()
    else:
        for i, it in enumerate(items[:11]):
            if i < 6:
                rn.fits(1)
            elif i == 6:
                rn.before(1, END)
                assert rn.live == 6
            assert be.add_items([it], NOW) == [False]
            if i == 6:
                rn.after()
    assert be.totals() == lc.oracle_totals(orc) and orc.size() == 10 and orc.counters()[3] == 1
    a, g = orc.get_item(names[1], NOW), be.get_item(names[1], NOW)                   # the oldest item left: to the front (lrucache.go:123)
    assert a is not None and g is not None and a["remaining"] == g["remaining"], (a, g)
    orc.add_item(items[11], NOW)
    assert be.add_items([items[11]], NOW) == [False]
    assert be.totals() == lc.oracle_totals(orc) and orc.counters()[3] == 2
    assert survivors(be, orc, names, NOW) == [names[1]] + names[3:]
    assert be.totals() == lc.oracle_totals(orc) and be.recency()["renumbers"] == 1
    be.close()
    orc.close()


def case_lookup_triggers(remove, make=EngineBackend):
    """guber_get_item / guber_remove_item as the call that renumbers (they take a stamp without passing through maintain()): three items with the
    last three stamps, then the lookup of item 0 — GetItem moves it to the front with stamp 4 of the new numbering, Remove takes it out —, then
    Adds until the cache of 10 has evicted: the victim is item 1, the oldest that is left"""
    be, orc, mirror = cache_engine(10, END - 3, make)
    rn = Renumbering(be.recency, be.size, f"lookup remove={remove}")
    names = [f"lk_{i}" for i in range(12)]
    items = recency_items(names, NOW)
    for it in items[:3]:
        rn.fits(1)
        orc.add_item(it, NOW)
        assert be.add_items([it], NOW) == [False]
    rn.before(1, END)
    if remove:
        orc.remove_item(names[0])
        be.remove_item(names[0])
    else:
        a, g = orc.get_item(names[0], NOW), be.get_item(names[0], NOW)
        assert a is not None and g is not None and a["remaining"] == g["remaining"], (a, g)
    assert rn.live == 3
    rn.after()
    more = items[3:12] if remove else items[3:11]                                     # up to 11 items: one eviction
    for it in more:
        orc.add_item(it, NOW)
        assert be.add_items([it], NOW) == [False]
    assert be.totals() == lc.oracle_totals(orc) and orc.size() == 10 and orc.counters()[3] == 1
    want = [n for n in names[:3 + len(more)] if n != names[1] and not (remove and n == names[0])]
    assert survivors(be, orc, names, NOW) == want
    be.close()
    orc.close()


def case_add_items_dev(dv=None, make=EngineBackend):
    """guber_add_items_dev as the call that renumbers: five items by guber_add_items (stamps 2^53 - 6 .. 2^53 - 2), then five device rows whose
    stamps do not fit (one is left) — the five live items get 1..5, the rows 6..10 —, then one more Add: eleven items in a cache of ten, and the
    victim is item 0"""
    dv = dv or Device()
    be, orc, mirror = cache_engine(10, END - 6, make)
    rn = Renumbering(be.recency, be.size, "add_items_dev")
    names = [b"dv_%d" % i for i in range(11)]
    specs = [dict(key=k, algorithm=0, limit=10, duration=3_600_000, remaining=9 - i % 7, stamp=NOW, expire_at=NOW + 3_600_000) for i, k in enumerate(names)]
    for s in specs[:5]:
        rn.fits(1)
        orc.add_item(co.mk(s), NOW)
        assert be.add_items([co.mk(s)], NOW) == [False]
    rn.before(5, END - 1)
    want = np.array([orc.add_item(co.mk(s), NOW) for s in specs[5:10]], np.uint8)
    got = co.add_dev(be.e, specs[5:10], NOW, False, dv.put, dv.get)
    assert np.array_equal(got, want), (got, want)
    assert rn.live == 5
    rn.after()
    orc.add_item(co.mk(specs[10]), NOW)
    assert be.add_items([co.mk(specs[10])], NOW) == [False]
    assert be.totals() == lc.oracle_totals(orc) and orc.size() == 10 and orc.counters()[3] == 1
    assert survivors(be, orc, names, NOW) == names[1:]
    be.close()
    orc.close()


# ---- 3: the one-launch path ------------------------------------------------------------------------------------------------------------
def case_one_launch(make=EngineBackend):
    """k_small writes the stamps: five batches of 50 new keys into a cache of 300 that they cannot make bind — the one-launch path, asserted
    from small_batches —, the third being the call that renumbers (20 stamps are left); then batches of 120 new keys bind and the victims are
    those keys in the order k_small stamped them on both sides of the renumbering, element-wise the oracle's"""
    cs = 300
    mirror, orc = Mirror(seq=SEQ_NEXT), Oracle(cache_size=cs)
    be = make(cache_size=cs, max_batch=1024, flags=FLAG)
    advance_to(be, mirror, END - 20 - 2 * 50)
    small0 = be.e.stats()["small_batches"]
    rn = Renumbering(be.recency, be.size, "one launch")
    fill = [HostBatch([f"one_{s}_{i}" for i in range(50)][::-1], 1, 100, 3_600_000, NOW + s, algorithm=np.arange(50) & 1) for s in range(5)]
    run_bounded(be, orc, mirror, cs, watched(fill, rn, mirror, 2, END - 20), "one-launch fill")
    assert rn.live == 100 and be.e.stats()["small_batches"] == small0 + 5
    more = [HostBatch([f"more_{s}_{i}" for i in range(120)], 1, 100, 3_600_000, NOW + 10 + s) for s in range(3)]
    run_bounded(be, orc, mirror, cs, more, "binding after the one-launch fill")
    probe = HostBatch([f"one_{s}_{i}" for s in range(5) for i in range(50)], 0, 100, 3_600_000, NOW + 20)
    support.assert_results_equal(be.eval(probe), orc.eval(probe), "who is left")
    assert be.totals() == lc.oracle_totals(orc) and orc.counters()[3] >= 250 and be.recency()["renumbers"] == 1
    be.close()
    orc.close()


def case_empty_table(make=EngineBackend):
    """an engine that holds nothing when its stamps end: nothing to number, the call's n stamps are 1..n"""
    mirror, orc = Mirror(seq=SEQ_NEXT), Oracle(cache_size=300)
    be = make(cache_size=300, max_batch=1024, flags=FLAG)
    advance_to(be, mirror, END - 20)
    rn = Renumbering(be.recency, be.size, "empty table")
    b = HostBatch([f"empty_{i}" for i in range(50)], 1, 100, 3_600_000, NOW)
    rn.before(50, END - 20)
    support.assert_results_equal(be.eval(b), orc.eval(b), "the first items of an empty table")
    assert rn.live == 0 and rn.after()["next_stamp"] == 1 + 50
    assert be.totals() == lc.oracle_totals(orc)
    be.close()
    orc.close()


# ---- 4: fused launches -----------------------------------------------------------------------------------------------------------------
def case_fused(dv=None, count_launches=False):
    """guber_eval_batches_routed_dev over four engines of one stream, the owner-partitioned pipeline (flags 64, so that batches of 300 take it),
    GUBER_FUSE_EP as it is by default: eight rounds of 300 requests per table in ONE call.  Engine 1 is advanced so that its stamps end in round
    3, engine 2 in round 5; engines 0 and 3 stay 4 096 below the end.  From the second round on the group's k_eval3 is held back for the next
    round's k_part (k_evalpart_multi); the prelude that has to renumber says defer, the held-back evaluation is launched, and the prelude comes
    again.  All four engines equal their oracles; count_launches (the CPU build, where every launch is countable): k_evalpart_multi carried
    every pass that could be joined — rounds 1, 2, 4, 6, 7: before, between and after the two renumberings."""
    ga = _ga()
    dv = dv or Device()
    n_engines, rounds, n, K = 4, 8, 300, 500
    at = {1: 3, 2: 5}                                                     # engine -> the round whose batch renumbers
    e0 = ga.Engine(cache_size=1 << 14, max_batch=1024, flags=64 | FLAG)
    engs = [e0] + [ga.Engine(cache_size=1 << 14, max_batch=1024, stream=e0.stream_handle(), flags=64 | FLAG) for _ in range(n_engines - 1)]
    orcs = [Oracle(cache_size=1 << 14) for _ in engs]
    mirrors = [Mirror(seq=SEQ_NEXT) for _ in engs]
    for j, r in at.items():
        advance_to(Plain(engs[j]), mirrors[j], END - 150 - r * n, chunk=300)
    if count_launches:
        for e in engs:
            e.profile(True)
    rng = np.random.default_rng(17)
    zs = [streams.ZipfSampler(K, seed=400 + j) for j in range(n_engines)]
    which, hbs, keep, cb, cr = [], [], [], [], []
    for r in range(rounds):
        for j in range(n_engines):
            ids = zs[j].draw(n)
            hb = HostBatch([b"fz%d_%d" % (j, int(i)) for i in ids], rng.integers(0, 3, n), 60, 4000, NOW + r * 700, algorithm=(ids & 1).astype(np.uint8))
            b, res, k = dv.batch(hb)
            which.append(j); hbs.append(hb); keep.append(k); cb.append(b); cr.append(res)
    for j, e in enumerate(engs):
        info = e.recency_info()
        assert info["renumbers"] == 0 and info["next_stamp"] == mirrors[j].seq, (j, info)
        for r in range(rounds):                                           # the arithmetic: which round's 300 stamps do not fit
            assert (mirrors[j].seq + r * n + n > END) == (j in at and r >= at[j]), (j, r)
    dv.synchronize()
    N = len(which)
    ga.Engine.eval_routed_dev(engs, (C.c_uint32 * N)(*which), (ga.GuberBatch * N)(*cb), (ga.GuberResult * N)(*cr), N)
    for e in engs:
        e.synchronize()
    live_at = {}
    for s in range(N):
        j, r = which[s], s // n_engines
        if at.get(j) == r:
            live_at[j] = orcs[j].size()
        support.assert_results_equal(dv.host_result(keep[s], hbs[s].n), orcs[j].eval(hbs[s]), f"round {r} engine {j}")
    for j, (e, o) in enumerate(zip(engs, orcs)):
        info, st = e.recency_info(), e.stats()
        assert e.size() == o.size() and st["retries"] == 0 and st["batches"] >= rounds, (j, st)
        assert tuple(e.counters()[:3]) == tuple(o.counters()[:3]), (j, e.counters(), o.counters())
        if j in at:
            assert info["renumbers"] == 1 and info["last_live"] == live_at[j] and info["next_stamp"] == live_at[j] + 1 + (rounds - at[j]) * n, (j, info, live_at[j])
        else:
            assert info["renumbers"] == 0 and info["next_stamp"] == SEQ_NEXT + rounds * n, (j, info)
    assert sum(e.stats()["fused_batches"] for e in engs) > 0
    if count_launches:
        launches = {}
        for e in engs:
            for k, v in e.profile_read().items():
                launches[k] = launches.get(k, 0) + v[0]
        print("fused launches", {k: v for k, v in launches.items() if v})
        # one k_own_multi per round; a round's k_eval3 rides on the next round's k_part unless that round renumbers (3 and 5) or is the last
        assert launches.get("k_own_multi", 0) == rounds and launches.get("k_evalpart_multi", 0) == rounds - 1 - len(at), launches
        assert launches.get("k_eval3_multi", 0) == 1 + len(at) and launches.get("k_part_multi", 0) == 1 + len(at), launches
    for e in reversed(engs):
        e.close()
    for o in orcs:
        o.close()


# ---- 5: the front ----------------------------------------------------------------------------------------------------------------------
def case_front(dv=None):
    """guber_front_eval_dev: four tables (two streams), ONE call of six generations of 1 024 requests over 600 keys, caches of 96 items that bind
    (every share is larger than its cache: evaluated in pieces).  An engine's share of a generation takes as many stamps as it has requests —
    counted here from the placement's host rule —; engine 0 is advanced so that 10 stamps are left when generation 2 reaches it, engine 2 likewise
    for generation 4.  Answers are in arrival order and equal the oracle's with four workers."""
    ga = _ga()
    dv = dv or Device()
    n_engines, gens_n, n, per = 4, 6, 1024, 96
    at = {0: 2, 2: 4}
    place = ga.Placement(n_engines)
    e0 = ga.Engine(cache_size=per, max_batch=8192, flags=FLAG)
    e2 = ga.Engine(cache_size=per, max_batch=8192, flags=FLAG)
    engs = [e0, ga.Engine(cache_size=per, max_batch=8192, stream=e0.stream_handle(), flags=FLAG),
            e2, ga.Engine(cache_size=per, max_batch=8192, stream=e2.stream_handle(), flags=FLAG)]
    fr = ga.Front(engs, place, max_n=n, depth=8)
    orc = Oracle(cache_size=per * n_engines, workers=n_engines)
    rng = np.random.default_rng(2607)
    hbs, shares = [], []
    for g in range(gens_n):
        ids = rng.integers(0, 600, n)
        keys = [b"fr_%05d" % int(i) for i in ids]
        hbs.append(HostBatch(keys, rng.integers(0, 3, n), 50, 3_600_000, NOW + g * 100, algorithm=(ids & 1).astype(np.uint8)))
        shares.append(np.bincount(place.route_keys(*fe.pack(keys))[0], minlength=n_engines))
    shares = np.array(shares)
    assert (shares > per).all(), shares
    mirrors = [Mirror(seq=SEQ_NEXT) for _ in engs]
    for j, g in at.items():
        advance_to(Plain(engs[j]), mirrors[j], END - 10 - int(shares[:g, j].sum()), chunk=per // 2, exact=False)
    for j, e in enumerate(engs):
        info = e.recency_info()
        assert info["renumbers"] == 0 and info["next_stamp"] == mirrors[j].seq, (j, info)
        for g in range(gens_n):
            assert (mirrors[j].seq + int(shares[:g + 1, j].sum()) > END) == (j in at and g >= at[j]), (j, g)
    sides = [dv.batch(hb) for hb in hbs]
    dv.synchronize()
    assert fr.eval_dev((ga.GuberBatch * gens_n)(*[s[0] for s in sides]), (ga.GuberResult * gens_n)(*[s[1] for s in sides]), gens_n) == gens_n
    fr.synchronize()
    for g, hb in enumerate(hbs):
        support.assert_results_equal(dv.host_result(sides[g][2], hb.n), orc.eval(hb), f"generation {g}")
    assert sum(e.size() for e in engs) == orc.size() and sum(e.stats()["retries"] for e in engs) == 0
    assert sum(e.stats()["unexpired_evictions"] for e in engs) == orc.counters()[3] > 0
    for j, e in enumerate(engs):
        info = e.recency_info()
        if j in at:                                                        # (the live items at that moment: a cache that has been binding is full)
            assert info["renumbers"] == 1 and info["last_live"] == per and info["next_stamp"] == per + 1 + int(shares[at[j]:, j].sum()), (j, info, shares[:, j])
        else:
            assert info["renumbers"] == 0 and info["next_stamp"] == SEQ_NEXT + int(shares[:, j].sum()), (j, info)
    fr.close()
    for e in (engs[1], engs[3], e0, e2):
        e.close()
    place.close()
    orc.close()


# ---- 6: moved-in buckets -----------------------------------------------------------------------------------------------------------------
def case_moved_in():
    """two engines with the flag: A has handed out 2 000 stamps more than B when 65 of its buckets move into B (the destination numbers what
    it takes over: 65 stamps of B's, in the order of the hashes), then B is driven over the end by a batch of 30 resident and 30 new keys with
    30 stamps left.  Every live item is kept — 100 of B's own, the 65, the 30 new — and Each() sorted by key equals the oracle's; next_stamp =
    live + 1 + n can only hold if no stamp is left above it.  Three batches of 60 new keys then bind the cache of 200: the victims are the
    oldest by the order that was kept."""
    ga = _ga()
    cs = 200
    A = ga.Engine(cache_size=1024, max_batch=1024, flags=FLAG)
    B = EngineBackend(cache_size=cs, max_batch=1024, flags=FLAG, stream=A.stream_handle())
    ma, mb, orc = Mirror(seq=SEQ_NEXT), Mirror(seq=SEQ_NEXT), Oracle(cache_size=cs)
    advance(Plain(A), ma, 2000, NOW)
    a_items = recency_items([f"mva_{i}" for i in range(100)], NOW)
    b_items = recency_items([f"mvb_{i}" for i in range(100)], NOW)
    assert A.add_items(a_items) == [False] * 100
    assert B.add_items(b_items, NOW) == [False] * 100
    mb.stamps(100)
    for it in b_items:
        orc.add_item(it, NOW)
    assert A.recency_info()["next_stamp"] - 100 > B.recency()["next_stamp"]          # every stamp of A's items is above B's next
    moved = list(range(3, 68))                                                        # 65 hashes: more than one wavefront
    B.e.set_clock(NOW)
    assert A.move_items_to(B.e, [co.xxh(b"mva_%d" % i) for i in moved]) == 65
    mb.stamps(65)
    for i in moved:
        assert orc.add_item(a_items[i], NOW) is False
    assert A.size() == 35 and B.size() == 165 and B.recency()["next_stamp"] == mb.seq
    co.assert_same_items(B.e, orc, "after the move")
    advance_to(B, mb, END - 30, chunk=cs // 2, exact=False)
    rn = Renumbering(B.recency, B.size, "moved in")
    keys = [f"mvb_{i}" for i in range(15)] + [f"mva_{i}" for i in moved[:15]] + [f"mvn_{i}" for i in range(30)]
    b = HostBatch(keys, 1, 10, 3_600_000, NOW + 1)
    rn.before(60, END - 30)
    support.assert_results_equal(B.eval(b), orc.eval(b), "the batch that renumbers")
    assert rn.live == 165 and rn.after()["next_stamp"] == 165 + 1 + 60
    assert B.size() == orc.size() == 195 and orc.counters()[3] == 0                   # every live item is kept
    co.assert_same_items(B.e, orc, "after the renumbering")
    for s in range(3):
        b = HostBatch([f"mvx_{s}_{i}" for i in range(60)], 1, 10, 3_600_000, NOW + 2 + s)
        support.assert_results_equal(B.eval(b), orc.eval(b), f"binding batch {s} after the renumbering")
        assert B.totals() == lc.oracle_totals(orc), (s, B.totals(), lc.oracle_totals(orc))
    assert orc.size() == cs and orc.counters()[3] == 175
    co.assert_same_items(B.e, orc, "after the binding batches")
    B.close()
    A.close()
    orc.close()


def main():
    ga = _ga()
    assert "enginesim" in ga.LIB_PATH, "run as a script these cases are for the CPU build of the engine (GUBER_HIP_LIB)"
    hv = header_values()
    assert hv["GUBER_FLAG_TEST_LAST_STAMPS"] == FLAG == ga.FLAG_TEST_LAST_STAMPS and hv["GUBER_TEST_LAST_SEQ_NEXT"] == SEQ_NEXT, hv
    only = sys.argv[1:]
    cases = [(f"pipeline {label}", lambda f=f: case_pipeline(f)) for f, label in PIPELINES] + [
        ("cache sequence, one call", lambda: case_cache_sequence(True)), ("cache sequence, item by item", lambda: case_cache_sequence(False)),
        ("get_item renumbers", lambda: case_lookup_triggers(False)), ("remove_item renumbers", lambda: case_lookup_triggers(True)),
        ("add_items_dev renumbers", case_add_items_dev), ("one launch", case_one_launch), ("empty table", case_empty_table),
        ("fused", lambda: case_fused(count_launches=True)), ("front", case_front), ("moved in", case_moved_in)]
    ran = 0
    for name, fn in cases:
        if only and not any(o in name for o in only):
            continue
        fn()
        print("ok:", name, flush=True)
        ran += 1
    print(f"STAMP END CASES OK: {ran} cases")


if __name__ == "__main__":
    main()
