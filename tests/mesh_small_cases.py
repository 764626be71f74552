"""Scenarios for the mesh's one-launch path (guber_mesh_eval_small, gubernator_amd/csrc/guber_mesh.h; the kernel: k_mx_small,
guber_kernels_small.h) and the checks that go with them; shared by tests/test_gpu_mesh_small.py (the product library on a GPU, every rank
a logical rank of device 0) and tests/test_mesh_small_cpu.py (the same host code and kernels compiled for the CPU).  Built on
mesh_cases.World: one oracle per rank fed what the order rule says, the host ring and the ranks' placements for residency.

A small call hands over HOST arrays and is synchronous.  Every call here checks: the answers against the world's oracles, nothing written
behind n (answers and owner column), `calls` / `requests` / `forwarded` of guber_mesh_stats as guber_mesh_eval_dev moves them, the owner
column against the host ring (0xFF where the ring places no key).

The letters are the issue's: a sizes; b keys; c order across sources; d share fall-back; e wholesale fall-back; f mixing with the
general path; g the rule is the device's; h GLOBAL; i shapes of W."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):         # (run as a script by tests/test_mesh_small_cpu.py)
    if _p not in sys.path:
        sys.path.insert(0, _p)
import mesh_cases as mc
from mesh_cases import BEHAVIOR_GLOBAL, LONG_MS, MAX_KEY, NOW0, POP, SENTINEL_I64, SENTINEL_U8, STEP_MS, TAIL, Gen, by_ids, draw, population
from gubernator_amd.abi import GuberBatch, GuberResult, HostResult, assert_results_equal

OWNER_SENTINEL = 0x77
NAMES = ("status", "limit", "remaining", "reset_time", "err")
STAT_KEYS = ("over_limit_count", "cache_hits", "cache_misses", "cache_size")


def raw_small(w, gens):
    """one guber_mesh_eval_small over gens (host arrays of exactly n + TAIL sentinels) -> (answers per rank as dicts, owner column per rank)"""
    W = w.W
    B, R, OW, keep = (GuberBatch * W)(), (GuberResult * W)(), (C.c_void_p * W)(), []
    for r, g in enumerate(gens):
        ra = mc.result_arrays(g.n)
        ow = np.full(g.n + TAIL, OWNER_SENTINEL, np.uint8)
        p = dict(key_bytes=None, key_off=None, hits=None, limit=None, duration=None, burst=None, created_at=None, algorithm=None, behavior=None)
        src = {}
        if g.n:
            kb, off = g.packed()
            src = dict(key_bytes=kb, key_off=off, hits=g.hits, limit=g.limit, duration=g.duration, burst=g.burst, created_at=g.created_at,
                       algorithm=g.algorithm, behavior=g.behavior)
            src = {k: np.ascontiguousarray(v) for k, v in src.items() if v is not None}
            p.update({k: v.ctypes.data for k, v in src.items()})
        B[r] = GuberBatch(g.n, 0, p["key_bytes"], p["key_off"], p["hits"], p["limit"], p["duration"], p["burst"], p["created_at"], p["algorithm"],
                          p["behavior"], None, None, None, g.now)
        R[r] = GuberResult(ra["status"].ctypes.data, ra["limit"].ctypes.data, ra["remaining"].ctypes.data, ra["reset_time"].ctypes.data,
                           ra["err"].ctypes.data, 0, 0, 0, 0, 0)
        OW[r] = ow.ctypes.data
        keep.append((src, ra, ow))
    w.mesh.eval_small(B, R, OW)
    return [k[1] for k in keep], [k[2] for k in keep]


def check_tails(gens, answers, owners, label):
    for r, g in enumerate(gens):
        for name, a in answers[r].items():
            s = SENTINEL_U8 if a.dtype == np.uint8 else SENTINEL_I64
            assert (a[g.n:] == s).all(), f"{label}: rank {r}: {name} was written behind its {g.n} answers"
        assert (owners[r][g.n:] == OWNER_SENTINEL).all(), f"{label}: rank {r}: the owner column was written behind its {g.n} items"


def small_call(w, gens, label):
    """raw_small + every check of the module's docstring; -> answers per rank (HostResult)"""
    now = next(g.now for g in gens if g is not None)
    gens = [g if g is not None else Gen([], now) for g in gens]
    before = w.mesh.stats()
    answers, owners = raw_small(w, gens)
    after = w.mesh.stats()
    check_tails(gens, answers, owners, label)
    want, forwarded = w.expected(gens)
    got_all = []
    for r, g in enumerate(gens):
        got, exp = HostResult(g.n), HostResult(g.n)
        for name in NAMES:
            getattr(got, name)[:g.n] = answers[r][name][:g.n]
            getattr(exp, name)[:g.n] = want[r][name]
        assert_results_equal(got, exp, f"{label}: rank {r} (n={g.n})")
        got_all.append(got)
        if g.n:
            owner, _, kind = w.route(g)
            assert np.array_equal(owners[r][:g.n], np.where(kind != 0, 0xFF, owner).astype(np.uint8)), (label, r)
    assert after["calls"] - before["calls"] == 1 and after["requests"] - before["requests"] == sum(g.n for g in gens), (label, before, after)
    assert after["forwarded"] - before["forwarded"] == forwarded, (label, after["forwarded"] - before["forwarded"], forwarded)
    w.calls += 1
    return got_all


def engine_state(w):
    return [[(e.stats(), e.size()) for e in engs] for engs in w.engs]


def summed_stats(w):
    return {k: sum(e.stats()[k] for engs in w.engs for e in engs) for k in STAT_KEYS}


def with_global(ids, g, every=5):
    """a key is GLOBAL always or never: those whose number is a multiple of `every`"""
    g.behavior[:] = np.where(np.asarray(ids) % every == 0, BEHAVIOR_GLOBAL, 0)
    return g


SIZES_A = [(0, 0, 0), (0, 1, 0), (1, 0, 1), (0, 0, 63), (30, 0, 34), (65, 0, 0), (100, 55, 100), (1, 200, 55), (0, 0, 256), (128, 64, 64), (7, 9, 5),
           (85, 86, 85)]


def scenario_a(make_world):
    """sizes: W = 3, two plain engines and a GLOBAL engine per rank; totals of 0, 1, 2, 63, 64, 65, 255 and 256 spread unevenly (one rank
    empty, all but one empty, everything at the last rank), a dozen calls over one population with the clock advancing, token and leaky
    mixed by key, burst / created_at given in one call and NULL in the next; 257 is refused and leaves every engine as it was; residency"""
    w = make_world(W=3, n_engines=2, max_n=256, with_global=True)
    pop, rng = population(), np.random.default_rng(41)
    launches = 0
    for c, sizes in enumerate(SIZES_A):
        now = NOW0 + c * STEP_MS
        gens = []
        for r, n in enumerate(sizes):
            ids = draw(rng, n, POP)
            gens.append(with_global(ids, by_ids(pop, ids, now, c, full=c % 2 == 1, rng=rng)) if n else Gen([], now))
        small_call(w, gens, f"a call {c} sizes {sizes}")
        launches += 3 if sum(sizes) else 0
    st = w.mesh.small_stats()
    assert st["launches"] == launches and st["wholesale_fallbacks"] == 0 and st["calls"] == len(SIZES_A) - 1, st
    w.assert_every_pair_used("a")
    # 257 requests in all: refused before anything is enqueued
    state, mstat = engine_state(w), w.mesh.stats()
    now = NOW0 + len(SIZES_A) * STEP_MS
    try:
        raw_small(w, [by_ids(pop, draw(rng, n, POP), now, 0) for n in (100, 100, 57)])
        raise AssertionError("a: 257 requests were taken")
    except w.ga.GuberError as e:
        assert e.code == w.ga.E_BATCH_TOO_LARGE, e
    assert engine_state(w) == state and w.mesh.stats()["requests"] == mstat["requests"] and w.mesh.small_stats() == st
    w.check_residency("a")
    n = w.calls
    w.close()
    return n


def scenario_b(make_world):
    """keys: widths 1, 8, 31, 32, 33 and max_key_bytes ragged in one call, the empty key and an over-long one; `forwarded` as a twin world
    counts it through guber_mesh_eval_dev; then ranks with different max_key_bytes (32 and 64) and a 40-byte key"""
    w, twin = make_world(W=3, n_engines=2, max_n=256), make_world(W=3, n_engines=2, max_n=256)
    rng = np.random.default_rng(42)
    allw = [bytes([97 + i]) for i in range(26)] + sum((mc.keys_of_width(x, 30) for x in (8, 31, 32, 33, MAX_KEY)), [])
    for c in range(3):
        now = NOW0 + c * STEP_MS
        gens = []
        for r in range(3):
            n = (40, 77, 90)[(r + c) % 3]
            g = by_ids(allw, rng.integers(0, len(allw), n), now, c)
            for odd, key in ((int(rng.integers(0, n)), b""), (int(rng.integers(0, n)), b"\x21" * (MAX_KEY + 1))):
                g.keys[odd] = key
                g.hits[odd], g.limit[odd], g.duration[odd], g.algorithm[odd] = 1, 10, LONG_MS, 0    # (the request of World.errors)
            gens.append(g)
        f0, t0 = w.mesh.stats()["forwarded"], twin.mesh.stats()["forwarded"]
        got = small_call(w, gens, f"b call {c}")
        ref = twin.call(gens, f"b twin call {c}")
        assert w.mesh.stats()["forwarded"] - f0 == twin.mesh.stats()["forwarded"] - t0
        for r in range(3):
            assert_results_equal(got[r], ref[r], f"b call {c}: rank {r} against guber_mesh_eval_dev")
            assert (got[r].err[:got[r].n] == 4).sum() >= 1 and (got[r].err[:got[r].n] == 7).sum() >= 1
    w.check_residency("b")
    w.close(); twin.close()

    # rank 0 takes keys up to 32 bytes, rank 1 up to 64; a 40-byte key
    def tweak(rank, flags, kw):
        kw["max_key_bytes"] = 32 if rank == 0 else 64
        return flags, kw
    w, twin = make_world(W=2, n_engines=2, max_n=256, tweak=tweak), make_world(W=2, n_engines=2, max_n=256, tweak=tweak)
    cand = [b"%010d" % (i * 104729) + b"_forty_bytes_in_all_xxxxxxxxxxx" [:30] for i in range(64)]     # (fnv1 spreads keys that differ early)
    assert all(len(k) == 40 for k in cand)
    owner = w.ring.route(Gen(cand, NOW0).packed())
    k_of0, k_of1 = cand[int(np.nonzero(owner == 0)[0][0])], cand[int(np.nonzero(owner == 1)[0][0])]
    short = [b"s_%04d" % i for i in range(20)]
    gens = [Gen([k_of0, k_of1] + short[:10], NOW0), Gen([k_of0, k_of1] + short[10:], NOW0)]
    f0 = w.mesh.stats()["forwarded"]
    answers, owners = raw_small(w, gens)
    check_tails(gens, answers, owners, "b 32 / 64")
    ref = dev_call(twin, gens)
    for r in range(2):
        for name in NAMES:
            assert np.array_equal(answers[r][name][:gens[r].n], ref[r][name][:gens[r].n]), ("b 32 / 64", r, name)
    # arriving at the 32 rank: both stay and earn its item error, the ring names nobody
    assert answers[0]["err"][:2].tolist() == [7, 7] and owners[0][:2].tolist() == [0xFF, 0xFF]
    # arriving at the 64 rank: the one rank 0 owns is forwarded and gets the owner's item error, the other is evaluated here
    assert answers[1]["err"][:2].tolist() == [7, 0] and owners[1][:2].tolist() == [0, 1] and answers[1]["status"][1] == 0
    short_owner = [w.ring.route(g.packed())[2:] for g in gens]
    fwd = 1 + int((short_owner[0] != 0).sum()) + int((short_owner[1] != 1).sum())
    assert w.mesh.stats()["forwarded"] - f0 == fwd == twin.mesh.stats()["forwarded"]
    assert sum(e.size() for engs in w.engs for e in engs) == 21 == sum(e.size() for engs in twin.engs for e in engs)
    w.close(); twin.close()


def dev_call(w, gens):
    """one guber_mesh_eval_dev over gens without an oracle -> the answers per rank as dicts"""
    W = w.W
    B, R, keep = (GuberBatch * W)(), (GuberResult * W)(), []
    for r, g in enumerate(gens):
        rh = {k: w.upload(v) for k, v in mc.result_arrays(g.n).items()}
        p = dict(key_bytes=None, key_off=None, hits=None, limit=None, duration=None, burst=None, created_at=None, algorithm=None, behavior=None)
        h = {}
        if g.n:
            kb, off = g.packed()
            src = dict(key_bytes=kb, key_off=off.view(np.int32), hits=g.hits, limit=g.limit, duration=g.duration, burst=g.burst, created_at=g.created_at,
                       algorithm=g.algorithm, behavior=g.behavior.view(np.int32))
            h = {k: w.upload(np.ascontiguousarray(v)) for k, v in src.items() if v is not None}
            p.update({k: v[1] for k, v in h.items()})
        B[r] = GuberBatch(g.n, 0, p["key_bytes"], p["key_off"], p["hits"], p["limit"], p["duration"], p["burst"], p["created_at"], p["algorithm"],
                          p["behavior"], None, None, None, g.now)
        R[r] = GuberResult(rh["status"][1], rh["limit"][1], rh["remaining"][1], rh["reset_time"][1], rh["err"][1], 0, 0, 0, 0, 0)
        keep.append((h, rh))
    w.mesh.eval_dev(B, R)
    w.mesh.synchronize()
    return [{k: np.asarray(w.download(v[0])) for k, v in keep[r][1].items()} for r in range(W)]


def scenario_c(make_world):
    """order across sources: one hot token key from every rank in one call turns OVER_LIMIT exactly where source 0, 1, 2 in turn exhaust
    it; then 256 requests of one key from three sources"""
    W, limit = 3, 30
    w = make_world(W=W, n_engines=2, max_n=256)
    pop, rng = population(), np.random.default_rng(43)
    hot, per = b"k_hot_key", 2 * limit // W
    pos, gens = [], []
    for r in range(W):
        g = by_ids(pop, rng.integers(0, POP, 80), NOW0, 0)
        at = np.sort(rng.choice(80, per, replace=False))
        for i in at:
            g.keys[i] = hot
            g.hits[i], g.limit[i], g.duration[i], g.algorithm[i] = 1, limit, LONG_MS, 0
        pos.append(at); gens.append(g)
    got = small_call(w, gens, "c the hot key from every rank")
    seq = np.concatenate([got[r].status[pos[r]] for r in range(W)])
    assert (seq[:limit] == 0).all() and (seq[limit:] == 1).all(), seq
    assert got[1].status[pos[1]].tolist() == [0] * (limit - per) + [1] * (2 * per - limit)
    one = b"k_the_one"
    gens = [Gen([one] * n, NOW0 + STEP_MS, limit=150) for n in (100, 100, 56)]
    got = small_call(w, gens, "c 256 requests of one key")
    seq = np.concatenate([got[r].status[:got[r].n] for r in range(W)])
    assert (seq[:150] == 0).all() and (seq[150:] == 1).all(), seq
    st = w.mesh.small_stats()
    assert st["share_fallbacks"] == 0 and st["wholesale_fallbacks"] == 0 and st["launches"] == 6, st
    w.close()


def scenario_d(make_world):
    """share fall-back: one key whose requests differ in hits and limit within a call — its share is re-run through the general pipeline,
    the others stand; guber_mesh_small_stats counts it"""
    w = make_world(W=3, n_engines=2, max_n=256)
    pop, rng = population(), np.random.default_rng(44)
    for c in range(3):
        now = NOW0 + c * STEP_MS
        gens = [by_ids(pop, draw(rng, 60, POP), now, c) for _ in range(3)]
        odd = b"k_odd_one"
        for r in range(3):
            for j, i in enumerate((3, 17, 40)):
                gens[r].keys[i] = odd
                gens[r].hits[i], gens[r].limit[i], gens[r].duration[i], gens[r].algorithm[i] = 1 + (j + r) % 3, 40 + j, LONG_MS, 0
        before = w.mesh.small_stats()
        small_call(w, gens, f"d call {c}")
        after = w.mesh.small_stats()
        assert after["share_fallbacks"] - before["share_fallbacks"] == 1 and after["launches"] - before["launches"] == 3, (before, after)
        assert after["wholesale_fallbacks"] == 0
    w.check_residency("d")
    w.close()


def scenario_e(make_world):
    """wholesale fall-back: engines whose cache may bind for the call's total, and an engine in careful mode: no small launch, the
    oracles' answers; then a population larger than the caches — the evicted keys behave as through guber_mesh_eval_dev on a twin world"""
    def tight(rank, flags, kw):
        if kw["cache_size"] == 1 << 14:
            kw["cache_size"] = 40
        return flags, kw

    def careful(rank, flags, kw):
        if rank == 1 and kw["cache_size"] == 1 << 14:
            flags[1] |= w_ga.FLAG_TEST_CAREFUL
        return flags, kw
    rng = np.random.default_rng(45)
    pop = population(30)
    for name, tweak in (("a cache that may bind", tight), ("a careful engine", careful)):
        w = make_world(W=3, n_engines=2, max_n=256, tweak=tweak)
        for c in range(3):
            small_call(w, [by_ids(pop, rng.integers(0, 30, 16), NOW0 + c * STEP_MS, c) for _ in range(3)], f"e {name}: call {c}")
        st = w.mesh.small_stats()
        assert st["launches"] == 0 and st["wholesale_fallbacks"] == 3 and st["calls"] == 3, (name, st)
        w.check_residency(f"e {name}")
        w.close()
    w, twin = make_world(W=2, n_engines=1, max_n=256, tweak=tight), make_world(W=2, n_engines=1, max_n=256, tweak=tight)
    pop = population(400)
    for c in range(5):
        gens = [by_ids(pop, rng.integers(0, 400, 100), NOW0 + c * STEP_MS, c) for _ in range(2)]
        answers, owners = raw_small(w, gens)
        check_tails(gens, answers, owners, f"e evictions: call {c}")
        ref = dev_call(twin, gens)
        for r in range(2):
            for nm in NAMES:
                assert np.array_equal(answers[r][nm][:100], ref[r][nm][:100]), (c, r, nm)
    assert w.mesh.small_stats()["launches"] == 0
    assert [e.size() for engs in w.engs for e in engs] == [e.size() for engs in twin.engs for e in engs]
    assert sum(e.stats()["unexpired_evictions"] for engs in w.engs for e in engs) == sum(e.stats()["unexpired_evictions"] for engs in twin.engs for e in engs) > 0
    w.close(); twin.close()


w_ga = None                                           # (the gubernator_amd module, set by the drivers' make_world: scenario_e's flags)


def scenario_f(make_world):
    """mixing with the general path: guber_mesh_eval_small and guber_mesh_eval_dev alternate over one population and one advancing clock:
    every answer equals one world of oracles, and the summed guber_stats deltas equal a twin world's fed the same stream through
    guber_mesh_eval_dev only"""
    w, twin = make_world(W=3, n_engines=2, max_n=256), make_world(W=3, n_engines=2, max_n=256)
    pop, rng = population(), np.random.default_rng(46)
    s0, t0 = summed_stats(w), summed_stats(twin)
    for c in range(8):
        now = NOW0 + c * STEP_MS
        gens = [by_ids(pop, draw(rng, n, POP), now, c) for n in ((50, 90, 70), (256, 1, 200))[c % 4 == 3]]
        if c % 2 == 0 and sum(g.n for g in gens) <= 256:
            small_call(w, gens, f"f call {c} (small)")
        else:
            w.call(gens, f"f call {c} (general)")
        twin.call(gens, f"f twin call {c}")
    s1, t1 = summed_stats(w), summed_stats(twin)
    assert {k: s1[k] - s0[k] for k in STAT_KEYS} == {k: t1[k] - t0[k] for k in STAT_KEYS}, (s0, s1, t0, t1)
    assert w.mesh.small_stats()["launches"] == 4 * 3
    w.check_residency("f")
    w.close(); twin.close()


def scenario_g(make_world):
    """the rule is the device's: after a placement pass that pins hot keys to other engines of their rank, the buckets moved and
    guber_front_set_rule, a small call finds the moved keys where the general path left them"""
    w = make_world(W=2, n_engines=4, max_n=256)
    pop, rng = population(200), np.random.default_rng(47)
    hot_ids = [3, 11, 19, 42, 57, 91]
    for c in range(2):
        ids = [np.concatenate([rng.integers(0, 200, 80), np.repeat(hot_ids, 4)]) for _ in range(2)]
        w.call([by_ids(pop, x, NOW0 + c * STEP_MS, c) for x in ids], f"g general call {c}")
    moved = 0
    for r in range(2):
        place = w.places[r]
        obs = Gen([pop[i] for i in np.concatenate([np.repeat(hot_ids, 3000), rng.integers(0, 200, 6000)])], NOW0)
        place.observe_keys(*obs.packed())
        moves = place.rebalance(0.125, False)
        for h, frm, to in moves:
            moved += w.engs[r][frm].move_items_to(w.engs[r][to], [h])
        rule = place.export(global_engine=-1)
        assert w.ga.lib().guber_front_set_rule(w.fronts[r].h, C.byref(rule)) == 0
    assert moved >= 1, "g: the placement pass moved no resident key"
    for c in range(2, 5):
        ids = [np.concatenate([rng.integers(0, 200, 60), np.repeat(hot_ids, 3)]) for _ in range(2)]
        small_call(w, [by_ids(pop, x, NOW0 + c * STEP_MS, c) for x in ids], f"g small call {c}")
    st = w.mesh.small_stats()
    assert st["launches"] == 6 and st["wholesale_fallbacks"] == 0, st
    w.check_residency("g")
    w.close()


def scenario_h(make_world):
    """GLOBAL requests at their owner and at a non-owner, with and without a global_engine in the rule: none is forwarded (small_call
    compares `forwarded` with the plain requests other ranks own), is_owner follows the ring (the oracles are fed it), and with a
    global_engine the buckets sit in the arrival rank's GLOBAL engine"""
    for glob in (True, False):
        w = make_world(W=2, n_engines=2, max_n=256, with_global=glob)
        pop, rng = mc.spread_population(w.ring, 2, per_owner=150), np.random.default_rng(48)
        for c in range(4):
            gens = []
            for r in range(2):
                ids = draw(rng, 110, 300)
                gens.append(with_global(ids, by_ids(pop, ids, NOW0 + c * STEP_MS, c), every=3))   # (the population alternates owners: every third key has both)
            small_call(w, gens, f"h global_engine {glob}: call {c}")
        for r in range(2):
            owner = w.ring.route(Gen(sorted(k for k, gl in w.seen[r].items() if gl), NOW0).packed())
            assert (owner == r).any() and (owner != r).any(), "h: GLOBAL keys at their owner and at a non-owner"
        st = w.mesh.small_stats()
        assert st["launches"] == 8 and st["wholesale_fallbacks"] == 0 and st["share_fallbacks"] == 0, st
        if glob:
            for r in range(2):
                assert w.engs[r][2].size() == sum(1 for gl in w.seen[r].values() if gl) > 0
            w.check_residency("h")
        else:
            assert sum(e.size() for engs in w.engs for e in engs) == sum(o.size() for o in w.oracles)
        w.close()


def scenario_i(make_world, plain_front):
    """shapes of W: one rank — the answers of a plain front; sixteen ranks of one engine each — 16 requests, one per rank, then 256; rings
    of both hash kinds"""
    w = make_world(W=1, n_engines=2, max_n=256)
    ref_eval, ref_close = plain_front(2, 256)
    pop, rng = population(), np.random.default_rng(49)
    for c, n in enumerate((1, 256, 65, 0)):
        now = NOW0 + c * STEP_MS
        g = by_ids(pop, draw(rng, n, POP), now, c) if n else Gen([], now)
        got = small_call(w, [g], f"i one rank: call {c}")[0]
        if n:
            ref = ref_eval(g)
            for name in NAMES:
                assert np.array_equal(getattr(got, name)[:n], ref[name][:n]), (c, name)
    st = w.mesh.small_stats()
    assert st["launches"] == 3 and st["wholesale_fallbacks"] == 0 and w.mesh.stats()["forwarded"] == 0, st
    ref_close()
    w.check_residency("i one rank")
    w.close()
    for kind in ("fnv1", "fnv1a"):
        w = make_world(W=16, n_engines=1, max_n=256, hash_kind=kind)
        pop = mc.spread_population(w.ring, 16, per_owner=20)
        rng = np.random.default_rng(50)
        small_call(w, [by_ids(pop, rng.integers(0, len(pop), 1), NOW0, 0) for _ in range(16)], f"i sixteen ranks ({kind}): one request per rank")
        small_call(w, [by_ids(pop, draw(rng, 16, len(pop)), NOW0 + STEP_MS, 1) for _ in range(16)], f"i sixteen ranks ({kind}): 256 requests")
        small_call(w, [by_ids(pop, np.arange(r * 16, r * 16 + 16), NOW0 + 2 * STEP_MS, 2) for r in range(16)], f"i sixteen ranks ({kind}): 256 keys")
        w.assert_every_pair_used(f"i {kind}")
        st = w.mesh.small_stats()
        assert st["launches"] == 48 and st["wholesale_fallbacks"] == 0, st
        w.check_residency(f"i sixteen ranks ({kind})")
        w.close()


def wrap_world(ga, support, new_engines, upload, download):
    """-> make_world(tweak=None, **kw): mesh_cases.World whose engines' flags and settings tweak(rank, flags, kw) may change"""
    global w_ga
    w_ga = ga

    def make_world(tweak=None, **kw):
        def ne(rank, flags, ekw):
            if tweak is not None:
                flags, ekw = tweak(rank, list(flags), dict(ekw))
            return new_engines(rank, flags, ekw)
        return mc.World(ga, support, new_engines=ne, upload=upload, download=download, **kw)
    return make_world


LETTERS = ("a", "b", "c", "d", "e", "f", "g", "h", "i")


def run(letter, make_world, plain_front):
    if letter == "i":
        return scenario_i(make_world, plain_front)
    return globals()["scenario_" + letter](make_world)


# ---- on the CPU build of the engine (tests/test_mesh_small_cpu.py): GUBER_HIP_LIB=tests/hostsim/libenginesim.so python tests/mesh_small_cases.py <letter>
def _cpu_main(letter):
    import gubernator_amd as ga
    import support
    from gubernator_amd.abi import HostBatch
    assert "enginesim" in ga.LIB_PATH, "this entry is for the CPU build of the engine (GUBER_HIP_LIB)"

    def new_engines(rank, flags, kw):
        e0 = ga.Engine(flags=flags[0], **kw)
        return [e0] + [ga.Engine(flags=f, stream=e0.stream_handle(), **kw) for f in flags[1:]]

    def plain_front(n_engines, max_n):
        engs = new_engines(0, [0] * n_engines, dict(cache_size=1 << 14, max_batch=4096, max_key_bytes=MAX_KEY))
        place = ga.Placement(n_engines)
        fr = ga.Front(engs, place, max_n=max_n, depth=3)

        def run_gen(g):
            kb, off = g.packed()
            hb = HostBatch((kb, off), g.hits, g.limit, g.duration, g.now, burst=g.burst, created_at=g.created_at, algorithm=g.algorithm, behavior=g.behavior)
            r = mc.result_arrays(g.n)
            res = GuberResult(r["status"].ctypes.data, r["limit"].ctypes.data, r["remaining"].ctypes.data, r["reset_time"].ctypes.data, r["err"].ctypes.data, 0, 0, 0, 0, 0)
            assert fr.eval_dev((GuberBatch * 1)(hb.c), (GuberResult * 1)(res), 1) == 1
            fr.synchronize()
            return r

        def close():
            fr.close()
            for e in engs:
                e.close()
            place.close()
        return run_gen, close

    run(letter, wrap_world(ga, support, new_engines, lambda a: (a, a.ctypes.data), lambda a: a), plain_front)
    print("MESH SMALL CASE OK", letter)


if __name__ == "__main__":
    _cpu_main(sys.argv[1])
