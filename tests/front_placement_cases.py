"""Cases for a front that observes its own traffic and runs placement passes (guber_front_observe / guber_front_observation /
guber_front_rebalance, gubernator_amd/csrc/guber_front.h; the kernels: guber_kernels_front_observe.h); shared by
tests/test_gpu_front_placement.py (the product library on a GPU) and tests/test_front_placement_cpu.py (the same host code and kernels
compiled for the CPU, at the same sizes but for case g, whose owner-partitioned shares the fiber emulation takes seconds for).
    GUBER_HIP_LIB=tests/hostsim/libenginesim.so python tests/front_placement_cases.py <case>

An Env hands in what differs between the two: upload(array) -> (handle, device pointer), download(handle) -> numpy array,
new_engines(n_engines, n_streams, **kw) -> engines (engine j on stream j * n_streams // n_engines), small: case g's reduced size.
Every answer is compared with ONE support.Oracle that knows nothing of placement, element-wise.  What the window counted is compared with
numpy: hashes from Placement.route_keys (the host's XXH64), slots from the numbers of Placement.export() (slots_of below:
guber_placement_impl.h slot_of in Python integers)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gubernator_amd as ga
import front_edges as fe
import support
from gubernator_amd.abi import GuberBatch, GuberResult, HostBatch, HostResult, assert_results_equal

NOW0 = 1_700_000_000_000
HOUR = 3_600_000
GLOBAL = 2
PAD = 0xA5                                            # every byte of a key row behind its key
NEW_KERNELS = ("k_fr_observe", "k_fr_observe_top")
NAMES = ("status", "limit", "remaining", "reset_time", "err")


class Env:
    def __init__(self, upload, download, new_engines, small):
        self.upload, self.download, self.new_engines, self.small = upload, download, new_engines, small


def slots_of(place, hashes):
    """the placement slot of every hash: guber_placement::slot_of with the exported numbers"""
    r = place.export()
    out = np.zeros(len(hashes), np.int64)
    for k, h in enumerate(hashes):
        h63 = int(h) >> 1
        w = (h63 * r.inv_step) >> 64
        if (w + 1) * r.step <= h63:
            w += 1
        w = min(w, r.n_shards - 1)
        out[k] = w * r.per + min(((h63 - w * r.step) * r.inv_sub) >> 64, r.per - 1)
    return out


class Rig:
    """engines, placement, front, oracle; run(): generations through ONE eval_dev call, each compared with the oracle"""

    def __init__(self, env, n_engines, n_streams=1, max_n=4096, global_engine=-1, profile=False, max_key_bytes=0, flags=None, cache_size=1 << 14, max_batch=4096):
        self.env, self.n_engines, self.global_engine = env, n_engines, global_engine
        self.place = ga.Placement(n_engines)
        self.engs = env.new_engines(n_engines, n_streams, cache_size=cache_size, max_batch=max_batch, max_key_bytes=max_key_bytes, flags=flags)
        if profile:
            self.engs[0].profile(True)
        self.front = ga.Front(self.engs, self.place, max_n=max_n, depth=3, global_engine=global_engine)
        self.orc = support.Oracle(cache_size=1 << 20)
        self.max_key = max_key_bytes or 1024
        self.max_n, self.ring, self.mesh = max_n, None, None

    def device_side(self, hb):
        cols = dict(key_bytes=hb.key_bytes, key_off=hb.key_off, hits=hb.hits, limit=hb.limit, duration=hb.duration, algorithm=hb.algorithm, behavior=hb.behavior)
        up = {k: self.env.upload(np.ascontiguousarray(v)) for k, v in cols.items()}
        res = {k: self.env.upload(v) for k, v in fe.result_arrays(hb.n).items()}
        p = {k: v[1] for k, v in up.items()}
        b = GuberBatch(hb.n, 0, p["key_bytes"], p["key_off"], p["hits"], p["limit"], p["duration"], None, None, p["algorithm"], p["behavior"], None, None, None, hb.now_ms)
        r = GuberResult(res["status"][1], res["limit"][1], res["remaining"][1], res["reset_time"][1], res["err"][1], 0, 0, 0, 0, 0)
        return b, r, (up, res)

    def fetch(self, hb, side):
        got = HostResult(hb.n)
        for name, (handle, _) in side[1].items():
            a = self.env.download(handle)
            s = fe.SENTINEL_U8 if a.dtype == np.uint8 else fe.SENTINEL_I64
            assert (a[hb.n:] == s).all(), f"{name} written behind the generation's end"
            getattr(got, name)[:hb.n] = a[:hb.n]
        return got

    def run(self, gens, label, check=True):
        sides = [self.device_side(hb) for hb in gens]
        N = len(gens)
        assert self.front.eval_dev((GuberBatch * N)(*[s[0] for s in sides]), (GuberResult * N)(*[s[1] for s in sides]), N) == N
        self.front.synchronize()
        out = []
        for k, (hb, s) in enumerate(zip(gens, sides)):
            got = self.fetch(hb, s[2])
            if check:
                assert_results_equal(got, self.orc.eval(hb), f"{label} generation {k}")
            out.append(got)
        return out

    def run_rows(self, hb, keys, stride, label):
        """the generation hb with its keys in ROWS `stride` bytes apart (every byte behind a key is PAD, the buffer ends with the last row),
        handed to the front as a mesh of one rank hands it over (guber_mesh_eval_rows_dev: the caller's rows go to the front as they lie)"""
        from gubernator_amd.mesh import Mesh, MeshRows
        if self.mesh is None:
            self.ring = ga.Ring(["gpu0"], 512, "fnv1")
            self.mesh = Mesh([self.front], self.ring, self.max_n)
        rows = np.full(hb.n * stride, PAD, np.uint8)
        for i, k in enumerate(keys):
            assert 0 < len(k) <= stride
            rows[i * stride:i * stride + len(k)] = np.frombuffer(k, np.uint8)
        cols = dict(key_bytes=rows, key_len=np.array([len(k) for k in keys], np.uint32), hits=hb.hits, limit=hb.limit, duration=hb.duration,
                    algorithm=hb.algorithm, behavior=hb.behavior)
        up = {k: self.env.upload(np.ascontiguousarray(v)) for k, v in cols.items()}
        res = {k: self.env.upload(v) for k, v in fe.result_arrays(hb.n).items()}
        p = {k: v[1] for k, v in up.items()}
        b = GuberBatch(hb.n, 0, p["key_bytes"], None, p["hits"], p["limit"], p["duration"], None, None, p["algorithm"], p["behavior"], None, None, None, hb.now_ms)
        r = GuberResult(res["status"][1], res["limit"][1], res["remaining"][1], res["reset_time"][1], res["err"][1], 0, 0, 0, 0, 0)
        self.mesh.eval_rows_dev((GuberBatch * 1)(b), (MeshRows * 1)(MeshRows(stride, p["key_len"])), (GuberResult * 1)(r))
        self.mesh.synchronize()
        assert_results_equal(self.fetch(hb, (up, res)), self.orc.eval(hb), label)

    def launches(self):
        return {k: v[0] for k, v in self.engs[0].profile_read().items() if v[0]}

    def handled(self):
        """requests every engine has evaluated so far (its cache hits + misses)"""
        out = []
        for e in self.engs:
            st = e.stats()
            out.append(st["cache_hits"] + st["cache_misses"])
        return np.array(out, np.int64)

    def close(self):
        if self.mesh is not None:
            self.mesh.close()
            self.ring.close()
        self.front.close()
        for e in reversed(self.engs):                 # (an engine that owns a stream goes after the ones it lent it to)
            e.close()
        self.place.close()
        self.orc.close()


def gen_of(keys, now, behavior=0, limit=1_000_000, algorithm=None, seed=0):
    """a generation over `keys` (bytes): hits 1, limits high enough that `remaining` keeps changing, token and leaky mixed by key; the key
    buffer ends exactly 8 bytes behind the last key"""
    if algorithm is None:
        algorithm = np.array([(k[-1] if k else 0) & 1 for k in keys], np.uint8)
    return HostBatch(fe.pack(keys), 1, limit, HOUR, now, algorithm=algorithm, behavior=behavior)


def expected_window(rig, gens):
    """what a window over `gens` must hold: (observed, skipped, slot_w, {hash: count})"""
    n_slots = rig.place.n_slots()
    slot_w, counts, observed, skipped = np.zeros(n_slots, np.int64), {}, 0, 0
    for hb in gens:
        _, hh = rig.place.route_keys(hb.key_bytes, hb.key_off)
        lens = np.diff(hb.key_off.astype(np.int64))
        seen = (lens != 0) & (lens <= rig.max_key)
        if rig.global_engine >= 0:
            seen &= (hb.behavior & GLOBAL) == 0
        observed += int(seen.sum()); skipped += int((~seen).sum())
        u, c = np.unique(hh[seen], return_counts=True)
        slot_w += np.bincount(slots_of(rig.place, u), weights=c, minlength=n_slots).astype(np.int64)
        for h, k in zip(u.tolist(), c.tolist()):
            counts[h] = counts.get(h, 0) + k
    return observed, skipped, slot_w, counts


def check_window(rig, gens, label):
    obs = rig.front.observation()
    observed, skipped, slot_w, counts = expected_window(rig, gens)
    n = sum(hb.n for hb in gens)
    assert obs["observed"] == observed and obs["skipped"] == skipped and obs["observed"] + obs["skipped"] == n, (label, obs["observed"], obs["skipped"], observed, skipped, n)
    assert obs["dropped"] == 0 and obs["generations"] == len(gens), (label, obs["dropped"], obs["generations"])
    assert np.array_equal(obs["slot_w"].astype(np.int64), slot_w), f"{label}: slot_w differs in {int((obs['slot_w'] != slot_w).sum())} slots"
    bar = max(1, observed // (rig.n_engines * 64))
    assert obs["threshold"] == bar, (label, obs["threshold"], bar)
    got = dict(obs["candidates"])
    assert len(got) == len(obs["candidates"]), f"{label}: a key was reported twice"
    want = {h: c for h, c in counts.items() if c >= bar}
    assert got == want, f"{label}: {len(got)} candidates reported, {len(want)} expected at a bar of {bar}; e.g. {sorted(set(got.items()) ^ set(want.items()))[:4]}"
    return obs


SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4097)


ROW_STRIDE = {"rows16": 16, "rows40": 40}


def keys_kind(kind, rng, count=300):
    """a population: one width of 16 bytes (the speculative fetch is taken), ragged, above 32 bytes (one width of 40, and ragged 33 .. 70); for
    key rows 16 and 40 bytes apart: ragged lengths up to the row's width, some keys filling their row (the first of them: the kernel's guess)"""
    if kind in ROW_STRIDE:
        w = ROW_STRIDE[kind]
        return [k[:w - 5 if i % 4 == 0 else int(rng.integers(1, w - 4))] + b"_%04d" % i for i, k in enumerate(fe.keys_of_width(w, count, rng))]
    if kind == "w16":
        return fe.keys_of_width(16, count, rng)
    if kind == "ragged":
        return [k[:int(rng.integers(1, 31))] + b"_%04d" % i for i, k in enumerate(fe.keys_of_width(30, count, rng))]
    if kind == "w40":
        return fe.keys_of_width(40, count, rng)
    assert kind == "long_ragged"
    return [k[:int(rng.integers(33, 70))] + b"_%04d" % i for i, k in enumerate(fe.keys_of_width(70, count, rng))]


def counts_exact(env, n_engines):
    """a. every = 1: every generation's window equals numpy — packed keys, and key rows with 0xA5 behind every key; a window over three
    generations adds up; the window after one is empty"""
    rig = Rig(env, n_engines, max_n=40_000)
    rig.front.observe(1)
    rng = np.random.default_rng(100 + n_engines)
    now = NOW0
    kinds = ("w16", "ragged", "w40", "long_ragged", "rows16", "rows40")
    for kind in kinds:
        pop = keys_kind(kind, rng)
        for n in SIZES:
            ids = np.minimum(rng.zipf(1.3, n) - 1, len(pop) - 1)
            keys = [pop[i] for i in ids]
            hb = gen_of(keys, now)
            if kind in ROW_STRIDE:
                rig.run_rows(hb, keys, ROW_STRIDE[kind], f"a {kind} n={n}")
            else:
                rig.run([hb], f"a {kind} n={n}")
            check_window(rig, [hb], f"a {n_engines} engines {kind} n={n}")
            now += 500
    # one key is half of a large generation
    pop = keys_kind("w16", rng)
    n = 40_000
    ids = np.where(np.arange(n) % 2 == 0, 7, rng.integers(0, len(pop), n))
    hb = gen_of([pop[i] for i in ids], now)
    rig.run([hb], "a one key is half")
    obs = check_window(rig, [hb], "a one key is half")
    assert max(c for _, c in obs["candidates"]) >= n // 2
    # three generations, one window; then nothing
    gens = []
    for k, kind in enumerate(("w16", "ragged", "w40")):
        pop = keys_kind(kind, rng)
        ids = np.minimum(rng.zipf(1.3, 1500) - 1, len(pop) - 1)
        gens.append(gen_of([pop[i] for i in ids], now + 500 * (k + 1)))
    rig.run(gens, "a three generations")
    check_window(rig, gens, "a window over three generations")
    obs = check_window(rig, [], "a the window after one")
    assert obs["observed"] == 0 and not obs["slot_w"].any() and not obs["candidates"]
    rig.close()


def not_observed(env):
    """b. with a global_engine in the rule, GLOBAL requests, empty keys and over-long keys are skipped — and answered as they are today;
    without one, GLOBAL requests are observed"""
    MAXK = 64
    scratch = env.new_engines(1, 1, cache_size=64, max_batch=256, max_key_bytes=MAXK)[0]
    errors = fe.error_answers(scratch, max_key_bytes=MAXK)
    scratch.close()
    rng = np.random.default_rng(7)
    pop = fe.keys_of_width(12, 40, rng)
    for global_engine in (2, -1):
        rig = Rig(env, 3, global_engine=global_engine, max_key_bytes=MAXK)
        rig.front.observe(1)
        n = 1100
        what = np.arange(n) % 3                       # 0: GLOBAL, 1: empty, 2: over-long
        keys = [pop[i % len(pop)] if what[i] == 0 else (b"" if what[i] == 1 else b"\x21" * (MAXK + 1)) for i in range(n)]
        hb = HostBatch(fe.pack(keys), 1, 10, HOUR, NOW0, algorithm=0, behavior=np.where(what == 0, GLOBAL, 0))
        got = rig.run([hb], "b", check=False)[0]
        sel = np.nonzero(what == 0)[0]
        want = rig.orc.eval(HostBatch([keys[i] for i in sel], 1, 10, HOUR, NOW0, algorithm=0, behavior=GLOBAL))
        for name in NAMES:
            assert np.array_equal(getattr(got, name)[sel], getattr(want, name)[:len(sel)]), f"b global_engine={global_engine}: {name} of the GLOBAL requests"
        rows = got.rows()
        for i in range(n):
            if what[i]:
                assert rows[i] == errors["empty" if what[i] == 1 else "too_long"], (i, rows[i])
        obs = check_window(rig, [hb], f"b global_engine={global_engine}")
        if global_engine >= 0:
            assert obs["observed"] == 0 and obs["skipped"] == n and not obs["slot_w"].any() and not obs["candidates"], obs
        else:
            assert obs["observed"] == len(sel) and obs["skipped"] == n - len(sel), obs
        rig.close()


def off_means_untouched(env):
    """c. a front that never observed, and one that turned it off again, launch none of the new kernels; every = 4 observes two of eight"""
    rng = np.random.default_rng(3)
    pop = fe.keys_of_width(16, 200, rng)

    def gens(count, now):
        return [gen_of([pop[i] for i in rng.integers(0, len(pop), 300)], now + 500 * k) for k in range(count)]
    for prelude in (None, (1, 0)):
        rig = Rig(env, 4, profile=True)
        for every in prelude or ():
            rig.front.observe(every)
        rig.run(gens(3, NOW0), "c off")
        ran = rig.launches()
        assert not any(k in ran for k in NEW_KERNELS) and ran.get("k_fr_count") == 3, ran
        rig.close()
    rig = Rig(env, 4, profile=True)
    rig.front.observe(4)
    g8 = gens(8, NOW0)
    rig.run(g8[:5], "c every 4")
    rig.run(g8[5:], "c every 4")
    ran = rig.launches()
    assert ran.get("k_fr_observe") == 2 and ran.get("k_fr_count") == 8 and "k_fr_observe_top" not in ran, ran
    check_window(rig, [g8[3], g8[7]], "c every 4: the fourth and the eighth generation")
    ran = rig.launches()
    assert ran.get("k_fr_observe_top") == 2 and "k_fr_observe" not in ran, ran      # (its two phases)
    rig.close()


class HotSet:
    """d's traffic: three keys that follow slots of engine 0, a tenth of every generation each; the rest uniform over 2 000 keys (all of
    11 bytes: a packed generation, unless hot_len says otherwise)"""

    def __init__(self, rig, n, hot_len=None, seed=11):
        self.rig, self.n, self.rng = rig, n, np.random.default_rng(seed)
        self.cold = [b"cold_%06d" % i for i in range(2000)]
        cand = [(b"hot_%06d" % i).ljust(hot_len or 11, b"h") for i in range(400)]
        sh, hh = rig.place.route_keys(*fe.pack(cand))
        pick = np.nonzero(sh == 0)[0][:3]
        assert len(pick) == 3
        self.hot = [cand[i] for i in pick]
        self.hot_hash = [int(hh[i]) for i in pick]
        self.now = NOW0

    def gen(self, with_hot=True):
        n, tenth = self.n, self.n // 10
        keys = [self.cold[i] for i in self.rng.integers(0, len(self.cold), n)]
        if with_hot:
            at = self.rng.permutation(n)[:3 * tenth]
            for q in range(3):
                for i in at[q * tenth:(q + 1) * tenth]:
                    keys[i] = self.hot[q]
        self.now += 500
        return gen_of(keys, self.now)

    def share_of_engine0(self, gens, label):
        before = self.rig.handled()
        self.rig.run(gens, label)
        d = self.rig.handled() - before
        assert d.sum() == sum(g.n for g in gens), (label, d)
        return d[0] / d.sum()

    def check_homes(self, label):
        """every hot key's bucket is in the engine the placement names, and in no other"""
        for k, h in zip(self.hot, self.hot_hash):
            home = self.rig.place.shard(h)
            held = [j for j, e in enumerate(self.rig.engs) if e.get_item(k, self.now) is not None]
            assert held == [home], f"{label}: {k!r} is held by engines {held}, the placement names {home}"


def pass_moves_hot_buckets(env, aging=True):
    """d. a pass moves hot buckets and answers stay exact; e. three passes without the hot keys take the pins back and move the buckets home"""
    n = 8192
    rig = Rig(env, 4, max_n=n)
    t = HotSet(rig, n)
    rig.front.observe(1)
    before = t.share_of_engine0([t.gen(), t.gen()], "d before the pass")
    t.check_homes("d before the pass")
    sizes = sum(e.size() for e in rig.engs)
    st = rig.front.rebalance(rig.place)
    print("d pass:", st, "engine 0's share before", round(before, 3))
    assert st["observed"] == 2 * n and st["dropped"] == 0, st
    # (with equal base loads the planner may pin the first key where it is — plan_locked: `if (j == from) continue` —; the other two leave)
    assert st["moves_planned"] >= 2 and st["cancelled"] == 0 and st["buckets_moved"] == st["moves_planned"] - st["cancelled"], st
    assert st["n_hot"] == 3 == rig.place.n_hot(), st
    assert sum(e.size() for e in rig.engs) == sizes == rig.orc.size()
    t.check_homes("d after the pass")
    assert sum(rig.place.shard(h) != 0 for h in t.hot_hash) == st["moves_planned"]
    after = t.share_of_engine0([t.gen(), t.gen()], "d after the pass")
    print("d engine 0's share after", round(after, 3))
    assert after < before and before > 0.42 and after < 0.33, (before, after)     # (by construction 47.5 % -> at most 27.5 %, the noise under 1 %)
    if aging:
        rig.front.observation()                       # (the two generations above held the hot keys: their window is not e's)
        per_pass = max(2, -(-4096 // n))              # (each pass over at least kMinWindow = 4 096 observed requests)
        for k in range(3):
            rig.run([t.gen(with_hot=False) for _ in range(per_pass)], f"e window {k}")
            last = rig.front.rebalance(rig.place)
            print("e pass", k, last)
            assert last["observed"] == per_pass * n, last
            if k < 2:
                assert last["moves_planned"] == 0 and last["n_hot"] == 3, last
        assert last["n_hot"] == 0 == rig.place.n_hot() and last["moves_planned"] == st["moves_planned"] == last["buckets_moved"] and last["cancelled"] == 0, last
        assert all(rig.place.shard(h) == 0 for h in t.hot_hash)
        t.check_homes("e after the third pass")
        back = t.share_of_engine0([t.gen()], "e the hot keys again")           # (their state survived both moves: exact against the oracle)
        assert back > 0.42, back
        assert sum(e.size() for e in rig.engs) == rig.orc.size()
    rig.close()


def refused_move_is_cancelled(env):
    """f. the destinations refuse: engines 1 .. 3 are created with FLAG_TEST_FIXED_ARENA and their long-key arenas (1 MiB) are full, the hot
    keys are long (100 bytes: above what a bucket's cell holds).  guber_move_items_by_hash gives the bucket back with GUBER_E_TABLE_FULL."""
    n, MAXK = 2048, 16384
    F = ga.FLAG_TEST_FIXED_ARENA
    rig = Rig(env, 4, max_n=n, max_key_bytes=MAXK, flags=[0, F, F, F], max_batch=4096)
    for j in (1, 2, 3):                               # keys of 16 384 bytes until the arena (16 bytes per table slot) refuses one, which nobody minds
        for rnd in range(8):
            res = rig.engs[j].eval(HostBatch([b"fill_%d_%03d_" % (j, rnd * 70 + i) + b"f" * (MAXK - 11) for i in range(70)], 1, 10, HOUR, NOW0))
            if (res.err[:70] == 6).any():             # GUBER_ITEM_E_TABLE_FULL
                break
        else:
            raise AssertionError("the arena of a destination is not full")
    filler = sum(e.size() for e in rig.engs)
    t = HotSet(rig, n, hot_len=100)
    rig.front.observe(1)
    before = t.share_of_engine0([t.gen(), t.gen()], "f before the pass")
    st = rig.front.rebalance(rig.place)
    print("f pass:", st)
    assert st["moves_planned"] >= 2 and st["cancelled"] == st["moves_planned"] and st["buckets_moved"] == 0, st
    assert all(rig.place.shard(h) == 0 for h in t.hot_hash), "a key whose move was cancelled follows its slot"
    t.check_homes("f after the pass")
    assert sum(e.size() for e in rig.engs) - filler == rig.orc.size()
    after = t.share_of_engine0([t.gen(), t.gen()], "f after the pass")
    assert abs(after - before) < 0.03, (before, after)
    rig.close()


def in_flight_and_pieces(env, n_streams):
    """g. three generations in one call on a front of depth 3, a pass, three more — over three streams (owner-partitioned pipeline, shares in
    pieces) and over one (one pair of launches for all tables); then a pass right after a probe whose generation nobody evaluated"""
    n = 1536 if env.small else 6000
    kw = dict(flags=[ga.FLAG_TEST_FORCE_PART] * 6, max_batch=512) if n_streams > 1 else dict(flags=[0] * 6)
    rig = Rig(env, 6, n_streams=n_streams, max_n=n, **kw)
    t = HotSet(rig, n)
    rig.front.observe(1)
    rig.run([t.gen() for _ in range(3)], f"g {n_streams} streams, before")
    st = rig.front.rebalance(rig.place)
    print("g pass:", st)
    assert st["observed"] == 3 * n and st["moves_planned"] >= 2 and st["cancelled"] == 0, st
    t.check_homes("g after the pass")
    rig.run([t.gen() for _ in range(3)], f"g {n_streams} streams, after")
    # a probed generation is dropped by the pass, as by any other front call: the call that evaluates it routes it afresh, by the new rule
    hb = t.gen()
    b, r, side = rig.device_side(hb)
    rig.front.probe_missing_dev(b)
    st = rig.front.rebalance(rig.place)
    assert st["observed"] == 3 * n, st                # (a store generation is not observed)
    assert rig.front.eval_dev((GuberBatch * 1)(b), (GuberResult * 1)(r), 1) == 1
    rig.front.synchronize()
    assert_results_equal(rig.fetch(hb, side), rig.orc.eval(hb), "g the generation a pass dropped")
    t.check_homes("g at the end")
    assert sum(e.size() for e in rig.engs) == rig.orc.size()
    rig.close()


def under_a_mesh(make_world):
    """h. W = 2, two engines per rank: a mesh call, a pass on rank 0's front with one hot key that rank 1 forwards, a mesh call, a one-launch
    call — mesh_cases' oracle arrangement"""
    import mesh_cases as mc
    import mesh_small_cases as ms
    w = make_world(W=2, n_engines=2, max_n=2049)
    pop = mc.population()
    owner = w.ring.route(mc.Gen(pop, NOW0).packed())
    sh, hh = w.places[0].route_keys(*mc.Gen(pop, NOW0).packed())
    mine = [i for i in range(len(pop)) if owner[i] == 0]
    hot = mine[0]
    rng = np.random.default_rng(5)
    w.fronts[0].observe(1)

    def gens(call, n):
        out = []
        for r in range(2):
            ids = rng.integers(0, len(pop), n)
            if r == 1:
                ids[rng.permutation(n)[:n // 3]] = hot            # a third of what arrives at rank 1 is rank 0's hot key
            out.append(mc.by_ids(pop, ids, NOW0 + call * mc.STEP_MS, call))
        return out
    w.call(gens(0, 1500), "h before the pass")
    st = w.fronts[0].rebalance(w.places[0])
    print("h pass:", st)
    assert st["observed"] > 0 and st["n_hot"] == 1 and st["cancelled"] == 0, st
    assert w.places[0].n_hot() == 1 and w.places[1].n_hot() == 0
    w.call(gens(1, 1500), "h after the pass")
    ms.small_call(w, gens(2, 100), "h one launch after the pass")
    w.check_residency("h")
    held = [j for j, e in enumerate(w.engs[0]) if pop[hot] in set(it["key"] for it in e.each())]
    assert held == [w.places[0].shard(int(hh[hot]))], held
    w.close()


def placement_feed():
    """i. (no device) observe_aggregate against observe called `count` times per key: the same pins, the same moves; a wrong n_slots"""
    rng = np.random.default_rng(9)
    keys = [b"feed_%05d" % i for i in range(3000)]
    counts = rng.integers(1, 6, len(keys))
    counts[:5] = (4000, 2500, 1800, 900, 40)
    a, b = ga.Placement(4), ga.Placement(4)
    _, hh = a.route_keys(*fe.pack(keys))
    for rnd in range(2):
        for h, c in zip(hh.tolist(), counts.tolist()):
            for _ in range(c):
                a.observe(h, 1)
        slot_w = np.bincount(slots_of(b, hh), weights=counts, minlength=b.n_slots()).astype(np.uint32)
        b.observe_aggregate(slot_w, hh, counts.astype(np.uint32))     # (every key a candidate, in the same order: the sketches see the same)
        ma, mb = a.plan(), b.plan()
        assert ma == mb and len(ma) >= 1, (rnd, ma, mb)
        a.commit(); b.commit()
        assert a.n_hot() == b.n_hot() >= 4, (a.n_hot(), b.n_hot())
        assert np.array_equal(a.route_keys(*fe.pack(keys))[0], b.route_keys(*fe.pack(keys))[0])
        counts = np.roll(counts, 7)                   # the hot set drifts: the second round plans moves both ways
    try:
        b.observe_aggregate(np.zeros(b.n_slots() - 1, np.uint32))
        raise AssertionError("a wrong n_slots was taken")
    except ga.GuberError as e:
        assert e.code == ga.E_INVALID_ARG
    a.close(); b.close()


def refusals(env):
    """j. (with a device) a one-engine front, a front without a rule, a placement with another shard count, a window never turned on"""
    def refused(f, *a):
        try:
            f(*a)
        except ga.GuberError as e:
            assert e.code == ga.E_INVALID_ARG, e
            return True
        return False
    e1 = env.new_engines(1, 1, cache_size=1024, max_batch=256)
    f1 = ga.Front(e1, None, max_n=256, depth=3)       # (one engine: no rule either)
    assert refused(f1.observe, 1) and refused(f1.observation)
    p2 = ga.Placement(2)
    assert refused(f1.rebalance, p2)
    f1.observe(0)                                     # (off is always taken)
    f1.close(); e1[0].close()
    rig = Rig(env, 4)
    assert refused(rig.front.observation) and refused(rig.front.rebalance, rig.place), "a window that was never turned on"
    rig.front.observe(1)
    p3, p4 = ga.Placement(3), ga.Placement(4, n_slots=1024)
    assert refused(rig.front.rebalance, p3) and refused(rig.front.rebalance, p4) and refused(rig.front.rebalance, p2)
    st = rig.front.rebalance(rig.place)               # (an empty window: nothing planned, nothing changes)
    assert st == dict(observed=0, dropped=0, moves_planned=0, buckets_moved=0, cancelled=0, n_hot=0), st
    for p in (p2, p3, p4):
        p.close()
    rig.close()


CASES = {
    "counts4": lambda env: counts_exact(env, 4),
    "counts16": lambda env: counts_exact(env, 16),
    "not_observed": not_observed,
    "off": off_means_untouched,
    "pass_and_aging": pass_moves_hot_buckets,
    "refused_move": refused_move_is_cancelled,
    "in_flight_3_streams": lambda env: in_flight_and_pieces(env, 3),
    "in_flight_1_stream": lambda env: in_flight_and_pieces(env, 1),
    "refusals": refusals,
}


# ---- on the CPU build of the engine (tests/test_front_placement_cpu.py) ---------------------------------------------------------------
def _cpu_env():
    assert "enginesim" in ga.LIB_PATH, "this entry is for the CPU build of the engine (GUBER_HIP_LIB)"

    def new_engines(n_engines, n_streams, flags=None, **kw):
        engs = []
        for j in range(n_engines):
            sj = j * n_streams // n_engines
            first = next((q for q in range(j) if q * n_streams // n_engines == sj), None)
            engs.append(ga.Engine(flags=(flags[j] if flags else 0), stream=None if first is None else engs[first].stream_handle(), **kw))
        return engs
    return Env(lambda a: (a, a.ctypes.data), lambda a: a, new_engines, small=True)


def _cpu_main(case):
    env = _cpu_env()
    if case == "mesh":
        import mesh_small_cases as ms

        def ne(rank, flags, kw):
            e0 = ga.Engine(flags=flags[0], **kw)
            return [e0] + [ga.Engine(flags=f, stream=e0.stream_handle(), **kw) for f in flags[1:]]
        under_a_mesh(ms.wrap_world(ga, support, ne, env.upload, env.download))
    elif case == "placement_feed":
        placement_feed()
    else:
        CASES[case](env)
    print("FRONT PLACEMENT CASE OK", case)


if __name__ == "__main__":
    _cpu_main(sys.argv[1])
