"""Scenarios for the mesh of fronts (guber_mesh_*, gubernator_amd/csrc/guber_mesh.h and guber_kernels_mesh.h) and the checks that go with
them; shared by tests/test_gpu_mesh.py (the product library on a GPU, every rank a logical rank of device 0) and tests/test_mesh_cpu.py
(the same host code and kernels compiled for the CPU).  numpy only: engines and the device's side of an array are handed in by the caller.

The expected answers come from ONE support.Oracle per rank.  Per call the owners are computed with the host ring (ga.Ring.route); oracle
o is fed the concatenation, over sources s = 0 .. W-1, of source s's requests whose destination is o, in arrival order — the order rule of
guber_mesh.h — and its answers are scattered back to (source, index).  A plain request's destination is its owner and it is evaluated
with IsOwner 1; a GLOBAL request stays on its arrival rank with is_owner = (owner == rank) (the recipe of enginesim_cases.front_global:
a key is GLOBAL always or never, so one oracle sees one sequence per key); an empty or over-long key stays too, is not shown to the
oracle and must carry the item error a plain engine gives it.  Result arrays carry sentinels behind n.

Scenarios (the letters are the issue's): a sizes around the thread stride and the tile, mixed across ranks, empty generations; b ragged
keys, key widths up to max_key_bytes, an empty and an over-long key; c one hot key from every rank in one call — the answers turn
OVER_LIMIT where the source-order rule puts the boundary; d skew — everything to one owner, request i to rank i mod W; e an inflow larger
than the front's max_n; f GLOBAL; g sixteen ranks; h one rank equals a plain front; i residency (behind a and b)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):         # (run as a script by tests/test_mesh_cpu.py)
    if _p not in sys.path:
        sys.path.insert(0, _p)
from gubernator_amd.abi import GuberBatch, GuberResult, HostBatch, HostResult, assert_results_equal

NOW0 = 1_700_000_000_000
STEP_MS = 500
LONG_MS, SHORT_MS = 60_000, 300
MAX_KEY = 40                                          # max_key_bytes of every engine here: request records of 128 bytes
TAIL = 64
SENTINEL_U8, SENTINEL_I64 = 99, -7
BEHAVIOR_GLOBAL = 2
POP = 3000


def population(count=POP):
    return [b"k_%06d" % i for i in range(count)]


def spread_population(ring, W, per_owner=190):
    """keys "k_%06d" of which every rank owns per_owner: fnv1 moves a key that differs from its neighbour in the last digits only a few
    ring points, so 3 000 consecutive numbers belong to a handful of sixteen owners; these are picked from numbers 37 apart, owner by owner
    in turn (the 24 hot keys draw() favours are spread over the owners too)"""
    cand = [b"k_%06d" % i for i in range(0, 1_000_000, 37)]
    owner = ring.route(Gen(cand, NOW0).packed())
    mine = [np.nonzero(owner == o)[0][:per_owner] for o in range(W)]
    assert min(len(x) for x in mine) == per_owner, [len(x) for x in mine]
    return [cand[mine[o][j]] for j in range(per_owner) for o in range(W)]


def keys_of_width(width, count):
    """count distinct keys "k_<digits>" of exactly `width` bytes (width 3: ten of them)"""
    count = min(count, 10 ** (width - 2))
    return [b"k_%0*d" % (width - 2, i) for i in range(count)]


def result_arrays(n):
    return dict(status=np.full(n + TAIL, SENTINEL_U8, np.uint8), err=np.full(n + TAIL, SENTINEL_U8, np.uint8),
                limit=np.full(n + TAIL, SENTINEL_I64, np.int64), remaining=np.full(n + TAIL, SENTINEL_I64, np.int64),
                reset_time=np.full(n + TAIL, SENTINEL_I64, np.int64))


class Gen:
    """the generation that arrives at one rank: keys (list of bytes) and columns (numpy); burst / created_at may be None"""

    def __init__(self, keys, now, hits=1, limit=10, duration=LONG_MS, algorithm=0, behavior=0, burst=None, created_at=None):
        n = len(keys)
        self.keys, self.n, self.now = list(keys), n, now
        col = lambda x, dt: np.ascontiguousarray(np.broadcast_to(np.asarray(x, dt), (n,))).copy()
        self.hits, self.limit, self.duration = col(hits, np.int64), col(limit, np.int64), col(duration, np.int64)
        self.algorithm, self.behavior = col(algorithm, np.uint8), col(behavior, np.uint32)
        self.burst = None if burst is None else col(burst, np.int64)
        self.created_at = None if created_at is None else col(created_at, np.int64)

    def packed(self):
        """(key_bytes, key_off): the keys one behind the other and exactly the 8 readable bytes behind the last one that
        include/guber_gpu.h promises (not zero: nothing may depend on them)"""
        off = np.zeros(self.n + 1, np.uint32)
        if self.n:
            off[1:] = np.cumsum([len(k) for k in self.keys])
        kb = np.full(int(off[-1]) + 8, 0xA5, np.uint8)
        kb[:int(off[-1])] = np.frombuffer(b"".join(self.keys), np.uint8)
        return kb, off


def by_ids(pop, ids, now, call, full=False, rng=None):
    """requests over the population `pop`: one limit (5 .. 30) and one algorithm per key, hits 1; every third call's durations are shorter
    than the clock's step"""
    ids = np.asarray(ids, np.int64)
    g = Gen([pop[i] for i in ids], now, limit=5 + ids % 26, duration=SHORT_MS if call % 3 == 2 else LONG_MS, algorithm=(ids // 7) % 2)
    if full:
        g.burst = np.where(rng.random(g.n) < 0.5, 0, g.limit + 3).astype(np.int64)
        g.created_at = (now + rng.integers(-70, 70, g.n)).astype(np.int64)
    return g


def draw(rng, n, pop_size):
    """n ids: half among the first 24 keys (they run over their limits), half anywhere"""
    return np.where(rng.random(n) < 0.5, rng.integers(0, min(24, pop_size), n), rng.integers(0, pop_size, n))


class World:
    """W ranks: engines, placement, front and oracle per rank, the ring, the mesh.
    new_engines(rank, flags_list, kw) -> the rank's engines (kw: cache_size, max_batch, max_key_bytes)
    upload(array) -> (handle, device pointer); download(handle) -> numpy array"""

    def __init__(self, ga, support, W, n_engines, max_n, new_engines, upload, download, hash_kind="fnv1", front_max_n=None, with_global=False):
        from gubernator_amd.mesh import Mesh
        self.ga, self.W, self.max_n, self.upload, self.download = ga, W, max_n, upload, download
        self.ring = ga.Ring([f"gpu{r}" for r in range(W)], 512, hash_kind)
        self.engs, self.places, self.fronts, self.oracles = [], [], [], []
        self.global_engine = n_engines if with_global else -1
        for r in range(W):
            flags = [0] * n_engines + ([ga.FLAG_GLOBAL] if with_global else [])
            engs = new_engines(r, flags, dict(cache_size=1 << 14, max_batch=4096, max_key_bytes=MAX_KEY))
            place = ga.Placement(n_engines) if (n_engines > 1 or with_global) else None
            self.engs.append(engs); self.places.append(place)
            self.fronts.append(ga.Front(engs, place, max_n=front_max_n or max_n, depth=3, global_engine=self.global_engine))
            self.oracles.append(support.Oracle(cache_size=1 << 20, workers=n_engines))   # (the untouched worker rule: workers = the rank's engines)
        self.mesh = Mesh(self.fronts, self.ring, max_n)
        scratch = new_engines(0, [0], dict(cache_size=64, max_batch=256, max_key_bytes=MAX_KEY))[0]
        self.errors = {}
        for kind, key in (("empty", b""), ("too_long", b"\x21" * (MAX_KEY + 1))):
            self.errors[kind] = scratch.eval(HostBatch([key], 1, 10, LONG_MS, NOW0, algorithm=0, behavior=0)).rows()[0]
        scratch.close()
        assert self.errors["empty"][4] == 4 and self.errors["too_long"][4] == 7, self.errors   # GUBER_ITEM_E_EMPTY_KEY, GUBER_ITEM_E_KEY_TOO_LONG
        self.pairs = np.zeros((W, W), np.int64)                   # requests per (source, destination) so far
        self.seen = [dict() for _ in range(W)]                    # per rank: key -> GLOBAL?
        self.calls = 0

    def route(self, g):
        """-> (owner, stay, kind) of a generation by the host ring: stay = GLOBAL, empty or over-long"""
        if g.n == 0:
            return np.zeros(0, np.uint32), np.zeros(0, bool), np.zeros(0, np.uint8)
        owner = self.ring.route(g.packed())
        lens = np.array([len(k) for k in g.keys])
        kind = np.where(lens == 0, 1, np.where(lens > MAX_KEY, 2, 0)).astype(np.uint8)
        return owner, ((g.behavior & BEHAVIOR_GLOBAL) != 0) | (kind != 0), kind

    def expected(self, gens):
        """the oracles' answers, scattered back to (source, index): {name: array} per rank; and the number of forwarded requests"""
        W = self.W
        routed = [self.route(g) for g in gens]
        want = [dict(status=np.zeros(g.n, np.uint8), err=np.zeros(g.n, np.uint8), limit=np.zeros(g.n, np.int64), remaining=np.zeros(g.n, np.int64),
                     reset_time=np.zeros(g.n, np.int64)) for g in gens]
        forwarded = 0
        for s, (g, (owner, stay, kind)) in enumerate(zip(gens, routed)):
            dest = np.where(stay, s, owner)
            for o in range(W):
                self.pairs[s, o] += int((dest == o).sum())
            forwarded += int((dest != s).sum())
            for i in np.nonzero(kind)[0]:
                row = self.errors["empty" if kind[i] == 1 else "too_long"]
                for name, v in zip(("status", "limit", "remaining", "reset_time", "err"), row):
                    want[s][name][i] = v
            for i in np.nonzero(kind == 0)[0]:
                assert self.seen[int(dest[i])].setdefault(g.keys[i], bool(g.behavior[i] & BEHAVIOR_GLOBAL)) == bool(g.behavior[i] & BEHAVIOR_GLOBAL)
        for o in range(W):
            keys, cols, back = [], {k: [] for k in ("hits", "limit", "duration", "algorithm", "behavior", "burst", "created_at", "is_owner")}, []
            for s, (g, (owner, stay, kind)) in enumerate(zip(gens, routed)):
                sel = np.nonzero((np.where(stay, s, owner) == o) & (kind == 0))[0]
                keys += [g.keys[i] for i in sel]
                for name in ("hits", "limit", "duration", "algorithm", "behavior"):
                    cols[name].append(getattr(g, name)[sel])
                cols["burst"].append(np.zeros(len(sel), np.int64) if g.burst is None else g.burst[sel])
                cols["created_at"].append(np.full(len(sel), g.now, np.int64) if g.created_at is None else g.created_at[sel])
                cols["is_owner"].append(np.where(stay[sel], owner[sel] == s, True).astype(np.uint8))
                back += [(s, int(i)) for i in sel]
            if not keys:
                continue
            c = {k: np.concatenate(v) for k, v in cols.items()}
            res = self.oracles[o].eval(HostBatch(keys, c["hits"], c["limit"], c["duration"], gens[0].now, burst=c["burst"], created_at=c["created_at"],
                                                 algorithm=c["algorithm"], behavior=c["behavior"], is_owner=c["is_owner"]))
            for j, (s, i) in enumerate(back):
                for name in ("status", "limit", "remaining", "reset_time", "err"):
                    want[s][name][i] = getattr(res, name)[j]
        return want, forwarded

    def call(self, gens, label):
        """one guber_mesh_eval_dev over gens[r] (None: an empty generation); checks answers, sentinels and the forwarded count; -> answers per rank"""
        W = self.W
        now = next(g.now for g in gens if g is not None)
        gens = [g if g is not None else Gen([], now) for g in gens]
        assert all(g.now == now for g in gens)
        B, R, keep = (GuberBatch * W)(), (GuberResult * W)(), []
        for r, g in enumerate(gens):
            ra = result_arrays(g.n)
            rh = {k: self.upload(v) for k, v in ra.items()}
            p = dict(key_bytes=None, key_off=None, hits=None, limit=None, duration=None, burst=None, created_at=None, algorithm=None, behavior=None)
            h = {}
            if g.n:
                kb, off = g.packed()
                src = dict(key_bytes=kb, key_off=off.view(np.int32), hits=g.hits, limit=g.limit, duration=g.duration, burst=g.burst, created_at=g.created_at,
                           algorithm=g.algorithm, behavior=g.behavior.view(np.int32))
                h = {k: self.upload(np.ascontiguousarray(v)) for k, v in src.items() if v is not None}
                p.update({k: v[1] for k, v in h.items()})
            B[r] = GuberBatch(g.n, 0, p["key_bytes"], p["key_off"], p["hits"], p["limit"], p["duration"], p["burst"], p["created_at"], p["algorithm"],
                              p["behavior"], None, None, None, now)
            R[r] = GuberResult(rh["status"][1], rh["limit"][1], rh["remaining"][1], rh["reset_time"][1], rh["err"][1], 0, 0, 0, 0, 0)
            keep.append((h, rh))
        before = self.mesh.stats()
        self.mesh.eval_dev(B, R)
        self.mesh.synchronize()
        after = self.mesh.stats()
        want, forwarded = self.expected(gens)
        got_all = []
        for r, g in enumerate(gens):
            arrays = {k: self.download(v[0]) for k, v in keep[r][1].items()}
            got, exp = HostResult(g.n), HostResult(g.n)
            for name, a in arrays.items():
                s = SENTINEL_U8 if a.dtype == np.uint8 else SENTINEL_I64
                assert len(a) == g.n + TAIL and (a[g.n:] == s).all(), f"{label}: rank {r}: {name} was written behind its {g.n} answers"
                getattr(got, name)[:g.n] = a[:g.n]
                getattr(exp, name)[:g.n] = want[r][name]
            assert_results_equal(got, exp, f"{label}: rank {r} (n={g.n})")
            got_all.append(got)
        assert after["calls"] - before["calls"] == 1 and after["requests"] - before["requests"] == sum(g.n for g in gens), (label, before, after)
        assert after["forwarded"] - before["forwarded"] == forwarded, (label, after["forwarded"] - before["forwarded"], forwarded)
        self.calls += 1
        return got_all

    def assert_every_pair_used(self, label):
        assert (self.pairs > 0).all(), f"{label}: a (source, destination) pair of ranks never carried a request:\n{self.pairs}"

    def check_residency(self, label):
        """scenario i: every key is resident in exactly the engine of exactly the rank the host ring and the rank's placement name — GLOBAL
        keys in the arrival rank's global engine — and the engines hold as many items as the oracles"""
        for r in range(self.W):
            held = [set(it["key"] for it in e.each()) for e in self.engs[r]]
            keys = sorted(self.seen[r])
            home = {}
            if keys:
                g = Gen(keys, NOW0)
                if self.places[r] is not None:
                    sh, _ = self.places[r].route_keys(*g.packed())
                else:
                    sh = np.zeros(len(keys), np.uint32)
                home = {k: (self.global_engine if self.seen[r][k] else int(j)) for k, j in zip(keys, sh)}
            for j, hs in enumerate(held):
                stray = [k for k in hs if home.get(k) != j]
                assert not stray, f"{label}: rank {r} engine {j} holds {len(stray)} keys that belong elsewhere, e.g. {stray[0]!r} (home {home.get(stray[0])})"
            sizes = [e.size() for e in self.engs[r]]
            assert sum(sizes) == self.oracles[r].size(), (label, r, sizes, self.oracles[r].size())
        # (plain keys: the rank that holds a key is the ring's owner)
        for r in range(self.W):
            plain = [k for k, glob in self.seen[r].items() if not glob]
            if plain:
                assert (self.ring.route(Gen(plain, NOW0).packed()) == r).all(), (label, r)

    def close(self):
        self.mesh.close()
        for f in self.fronts:
            f.close()
        for engs in self.engs:
            for e in engs:
                e.close()
        for p in self.places:
            if p is not None:
                p.close()
        for o in self.oracles:
            o.close()
        self.ring.close()


SIZES_A = [(0, 1, 63), (64, 65, 1023), (1024, 1025, 2049), (2049, 0, 0), (0, 0, 1025), (63, 2049, 1), (1024, 64, 65), (1023, 1, 0),
           (65, 1025, 1024), (2049, 2049, 2049), (1, 1, 1), (64, 0, 63)]


def scenario_a(make_world):
    """sizes: W = 3, two engines per rank, a dozen calls over one population of one-width keys, token and leaky mixed"""
    w = make_world(W=3, n_engines=2, max_n=2049)
    pop, rng = population(), np.random.default_rng(31)
    for c, sizes in enumerate(SIZES_A):
        now = NOW0 + c * STEP_MS
        w.call([by_ids(pop, draw(rng, n, POP), now, c, full=(c + r) % 4 == 1, rng=rng) if n else None for r, n in enumerate(sizes)], f"a call {c} sizes {sizes}")
    w.assert_every_pair_used("a")
    w.check_residency("i after a")
    n = w.calls
    w.close()
    return n


def scenario_b(make_world):
    """ragged keys: one width per call (3, 8, 31, 32, 33, max_key_bytes) with one key a byte longer — at max_key_bytes that one is over-long
    and stays — then a call of mixed widths with an empty key"""
    w = make_world(W=3, n_engines=2, max_n=1025)
    rng = np.random.default_rng(32)
    c = 0
    for width in (3, 8, 31, 32, 33, MAX_KEY):
        now = NOW0 + c * STEP_MS
        pop = keys_of_width(width, 600)
        gens = []
        for r in range(3):
            n = (300, 1025, 257)[(r + c) % 3]
            ids = draw(rng, n, len(pop))
            g = by_ids(pop, ids, now, c)
            odd = int(rng.integers(0, n))
            g.keys[odd] = g.keys[odd] + b"x"
            if width == MAX_KEY:                                   # (the request of World.errors)
                g.hits[odd], g.limit[odd], g.duration[odd], g.algorithm[odd] = 1, 10, LONG_MS, 0
            gens.append(g)
        got = w.call(gens, f"b width {width}")
        if width == MAX_KEY:
            assert all((x.err[:x.n] == 7).sum() == 1 for x in got)
        c += 1
    now = NOW0 + c * STEP_MS
    allw = sum((keys_of_width(x, 40) for x in (3, 5, 8, 9, 16, 24, 31, 32, 33, 39, MAX_KEY)), [])
    gens = []
    for r in range(3):
        ids = rng.integers(0, len(allw), 700)
        g = by_ids(allw, ids, now, c)
        odd = int(rng.integers(0, 700))
        g.keys[odd] = b""
        g.hits[odd], g.limit[odd], g.duration[odd], g.algorithm[odd] = 1, 10, LONG_MS, 0
        gens.append(g)
    got = w.call(gens, "b mixed widths, an empty key")
    assert all((x.err[:x.n] == 4).sum() == 1 for x in got)
    w.assert_every_pair_used("b")
    w.check_residency("i after b")
    n = w.calls
    w.close()
    return n


def scenario_c(make_world):
    """order across sources: every rank sends one hot token key 2 x limit / W times in one call: the owner takes source 0's, then source
    1's, then source 2's — UNDER_LIMIT for the first `limit` of them, OVER_LIMIT from there on, and still OVER_LIMIT in the next call"""
    W, limit = 3, 30
    w = make_world(W=W, n_engines=2, max_n=1025)
    pop, rng = population(), np.random.default_rng(33)
    hot, per = b"k_hot_key", 2 * limit // W
    pos = []
    gens = []
    for r in range(W):
        g = by_ids(pop, rng.integers(0, POP, 300), NOW0, 0)
        at = np.sort(rng.choice(300, per, replace=False))
        for i in at:
            g.keys[i] = hot
            g.hits[i], g.limit[i], g.duration[i], g.algorithm[i] = 1, limit, LONG_MS, 0
        pos.append(at); gens.append(g)
    got = w.call(gens, "c the hot key from every rank")
    seq = np.concatenate([got[r].status[pos[r]] for r in range(W)])
    assert (seq[:limit] == 0).all() and (seq[limit:] == 1).all(), seq
    assert (got[0].status[pos[0]] == 0).all() and (got[2].status[pos[2]] == 1).all()
    assert got[1].status[pos[1]].tolist() == [0] * (limit - per) + [1] * (2 * per - limit)
    gens = []
    for r in range(W):
        g = by_ids(pop, rng.integers(0, POP, 64), NOW0 + STEP_MS, 1)
        g.keys[r] = hot
        g.hits[r], g.limit[r], g.duration[r], g.algorithm[r] = 1, limit, LONG_MS, 0
        gens.append(g)
    got = w.call(gens, "c the next call")
    assert all(got[r].status[r] == 1 and got[r].remaining[r] == 0 for r in range(W))
    w.assert_every_pair_used("c")
    w.close()


def scenario_d(make_world, hash_kind="fnv1"):
    """skew: a call whose every request belongs to owner 1 (the other pairs of ranks carry nothing in that call: said here, and the pairs
    are asserted over the scenario), then a call where request i belongs to rank i mod W"""
    W = 3
    w = make_world(W=W, n_engines=2, max_n=1025, hash_kind=hash_kind)
    pop, rng = population(), np.random.default_rng(34)
    owner = w.ring.route(Gen(pop, NOW0).packed())
    mine = [np.nonzero(owner == o)[0] for o in range(W)]
    assert min(len(x) for x in mine) > 100
    w.call([by_ids(pop, rng.choice(mine[1], 1025), NOW0, 0) for _ in range(W)], "d everything to owner 1")
    assert w.pairs[:, 1].tolist() == [1025] * W and w.pairs.sum() == W * 1025
    ids = [np.array([rng.choice(mine[i % W]) for i in range(1025)]) for _ in range(W)]
    w.call([by_ids(pop, x, NOW0 + STEP_MS, 1) for x in ids], "d request i to rank i mod W")
    w.assert_every_pair_used("d")
    w.close()


def scenario_e(make_world):
    """an inflow larger than the front's max_n: W = 4, every rank sends 2 049 requests that rank 2 owns (the other pairs carry nothing:
    said here) — rank 2's front gets 8 196 requests as generations of at most 2 049"""
    W = 4
    w = make_world(W=W, n_engines=1, max_n=2049)
    pop, rng = population(), np.random.default_rng(35)
    owner = w.ring.route(Gen(pop, NOW0).packed())
    mine = np.nonzero(owner == 2)[0]
    for c in range(2):
        before = w.mesh.stats()["inflow_pieces"]
        w.call([by_ids(pop, rng.choice(mine, 2049), NOW0 + c * STEP_MS, c) for _ in range(W)], f"e call {c}")
        assert w.mesh.stats()["inflow_pieces"] - before >= 4
    assert w.pairs[:, 2].tolist() == [2 * 2049] * W
    w.close()


def scenario_f(make_world):
    """GLOBAL: W = 2, every rank's front has a global_engine; the keys with an even number are GLOBAL (always), the others never.  No GLOBAL
    request is forwarded: World.call compares the mesh's `forwarded` with the number of plain requests other ranks own"""
    W = 2
    w = make_world(W=W, n_engines=1, max_n=2049, with_global=True)
    pop, rng = population(), np.random.default_rng(36)
    for c in range(3):
        gens = []
        for r in range(W):
            ids = draw(rng, 1500, POP)
            g = by_ids(pop, ids, NOW0 + c * STEP_MS, c)
            g.behavior[:] = np.where(ids % 2 == 0, BEHAVIOR_GLOBAL, 0)
            gens.append(g)
        w.call(gens, f"f call {c}")
    w.assert_every_pair_used("f")
    for r in range(W):
        assert w.engs[r][1].size() == sum(1 for glob in w.seen[r].values() if glob) > 0
    w.check_residency("f")
    w.close()


def scenario_g(make_world):
    """W = 16: sixteen ranks of one engine each, 1 025 requests per rank — sixteen-wide tile counts, destination 15's lane mask (the lanes
    behind a generation's end carry 0xff, whose low four bits are 15: they are in nobody's group)"""
    W = 16
    w = make_world(W=W, n_engines=1, max_n=1025)
    pop, rng = spread_population(w.ring, W), np.random.default_rng(37)
    for c in range(2):
        w.call([by_ids(pop, draw(rng, 1025, len(pop)), NOW0 + c * STEP_MS, c) for _ in range(W)], f"g call {c}")
    w.assert_every_pair_used("g")
    w.check_residency("g")
    w.close()


def scenario_h(make_world, plain_front):
    """W = 1: no exchange — the answers are those of a plain front over a second set of engines fed the same generations.
    plain_front(n_engines, max_n) -> (front, engines, placement, eval(gen) -> arrays)"""
    w = make_world(W=1, n_engines=2, max_n=2049, front_max_n=1024)   # (the front takes less than the mesh: 2 049 requests go as three generations)
    ref_eval, ref_close = plain_front(2, 2049)
    pop, rng = population(), np.random.default_rng(38)
    for c, n in enumerate((1025, 0, 2049, 64)):
        now = NOW0 + c * STEP_MS
        if n == 0:
            g = Gen([], now)
        else:
            g = by_ids(pop, draw(rng, n, POP), now, c, full=c == 2, rng=rng)
        got = w.call([g], f"h call {c}")[0]
        if n:
            ref = ref_eval(g)
            for name in ("status", "limit", "remaining", "reset_time", "err"):
                assert np.array_equal(getattr(got, name)[:n], ref[name][:n]), (c, name)
    assert w.mesh.stats()["forwarded"] == 0 and w.mesh.stats()["bytes_moved"] == 0
    ref_close()
    w.close()


# ---- the scenarios on the CPU build of the engine (tests/test_mesh_cpu.py): GUBER_HIP_LIB=tests/hostsim/libenginesim.so python tests/mesh_cases.py <letter>
def _cpu_main(letter):
    import gubernator_amd as ga
    import support
    assert "enginesim" in ga.LIB_PATH, "this entry is for the CPU build of the engine (GUBER_HIP_LIB)"

    def new_engines(rank, flags, kw):
        e0 = ga.Engine(flags=flags[0], **kw)
        return [e0] + [ga.Engine(flags=f, stream=e0.stream_handle(), **kw) for f in flags[1:]]

    def make_world(**kw):
        return World(ga, support, new_engines=new_engines, upload=lambda a: (a, a.ctypes.data), download=lambda a: a, **kw)

    def plain_front(n_engines, max_n):
        engs = new_engines(0, [0] * n_engines, dict(cache_size=1 << 14, max_batch=4096, max_key_bytes=MAX_KEY))
        place = ga.Placement(n_engines)
        fr = ga.Front(engs, place, max_n=max_n, depth=3)

        def run(g):
            kb, off = g.packed()
            hb = HostBatch((kb, off), g.hits, g.limit, g.duration, g.now, burst=g.burst, created_at=g.created_at, algorithm=g.algorithm, behavior=g.behavior)
            r = result_arrays(g.n)
            res = GuberResult(r["status"].ctypes.data, r["limit"].ctypes.data, r["remaining"].ctypes.data, r["reset_time"].ctypes.data, r["err"].ctypes.data, 0, 0, 0, 0, 0)
            assert fr.eval_dev((GuberBatch * 1)(hb.c), (GuberResult * 1)(res), 1) == 1
            fr.synchronize()
            return r

        def close():
            fr.close()
            for e in engs:
                e.close()
            place.close()
        return run, close

    cases = dict(a=lambda: scenario_a(make_world), b=lambda: scenario_b(make_world), c=lambda: scenario_c(make_world),
                 d=lambda: (scenario_d(make_world), scenario_d(make_world, "fnv1a")), e=lambda: scenario_e(make_world),
                 f=lambda: scenario_f(make_world), h=lambda: scenario_h(make_world, plain_front))
    cases[letter]()
    print("MESH CASE OK", letter)


if __name__ == "__main__":
    _cpu_main(sys.argv[1])
