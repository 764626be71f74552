"""Generations for the device front (guber_front_*, gubernator_amd/csrc/guber_kernels_front.h) at the edges its kernels branch on, and the
checks that go with them; shared by tests/test_gpu_front_edges.py (the product library on a GPU) and the `front_edges` case of
tests/enginesim_cases.py (the same kernels compiled for the CPU, under AddressSanitizer).  numpy only: the engine, the oracle and the
device's side of a generation are handed in by the caller.

What the scenarios are for (all of it code no other test reaches):
  key widths      k_fr_scatter copies a packed key as bytes (width < 8), as whole words (a multiple of 8) or as whole words plus an
                  overlapping last one; k_fr_count hashes widths < 32 from four words it requested ahead and width 32 from memory; keys of
                  ONE width above 32 are not packed at all
  sizes           256 requests per thread stride and 1 024 per tile, each with one below and one above
  one odd key     the generation's ragged flag raised by a single lane: at lane 0 (the width everybody is compared with), at a tile's edge,
                  last; an empty key and one over max_key_bytes (answered per item, include/guber_gpu.h GUBER_ITEM_E_*); every such
                  generation is followed, `depth` generations later, by a packed one in the same slot
  skew            one key 2 049 times (rank 1 023 in a tile), everything to the last engine, to engine 0, engine i mod n per lane (every
                  ballot pattern in every wave), runs of 64 (uniform waves)
  GLOBAL          Behavior_GLOBAL requests go to the rule's global_engine whatever their key hashes to
  tight buffers   pack() leaves exactly the 8 readable bytes behind the last key that include/guber_gpu.h promises the kernels
The header documents NULL for burst / created_at / is_owner only (guber_batch_t: `algorithm` and `behavior` carry no "NULL =" clause),
so there is no generation with a null behavior or algorithm column; the three optional columns are absent in every other generation."""
import ctypes as C

import numpy as np

from gubernator_amd.abi import GuberBatch, GuberResult, HostBatch, HostResult, assert_results_equal

NOW0 = 1_700_000_000_000
STEP_MS = 500                                         # the clock between two generations
LONG_MS, SHORT_MS = 60_000, 300                       # durations: long against the step; every third generation shorter than it
PACKED_WIDTHS = (1, 2, 7, 8, 9, 15, 16, 17, 24, 31, 32)
ONE_WIDTH_NOT_PACKED = (33, 40, 64)
SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 2049)
GLOBAL_WIDTHS = (7, 15, 32)
ODD_POSITIONS = (0, 1, 1023, 1024, 2048)             # of n = 2 049: lane 0, its neighbour, a tile's last and first request, the last one
BEHAVIOR_GLOBAL = 2
TAIL = 64                                             # result elements behind n that must keep their sentinels
SENTINEL_U8, SENTINEL_I64 = 99, -7
BIG_N, BIG_KEYS = (1 << 20) + 1025, 50_000            # 1 026 tiles: k_fr_scan's threads take two tiles each, thread 512 the last two

_M = (1 << 64) - 1
_P1, _P2, _P3, _P4, _P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M


def _round(acc, lane):
    return (_rotl((acc + lane * _P2) & _M, 31) * _P1) & _M


def _merge(h, v):
    return ((h ^ _round(0, v)) * _P1 + _P4) & _M


def xxh64(data, seed=0):
    """XXH64 of `data` (the published algorithm, xxHash's doc/xxhash_spec.md) in plain Python integers: the reference the engine's three
    implementations (bytes, four preloaded words, the host's) are compared with"""
    data = bytes(data)
    n, p = len(data), 0
    if n >= 32:
        v1, v2, v3, v4 = (seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed & _M, (seed - _P1) & _M
        while p + 32 <= n:
            v1 = _round(v1, int.from_bytes(data[p:p + 8], "little"))
            v2 = _round(v2, int.from_bytes(data[p + 8:p + 16], "little"))
            v3 = _round(v3, int.from_bytes(data[p + 16:p + 24], "little"))
            v4 = _round(v4, int.from_bytes(data[p + 24:p + 32], "little"))
            p += 32
        h = (_rotl(v1, 1) + _rotl(v2, 7) + _rotl(v3, 12) + _rotl(v4, 18)) & _M
        for v in (v1, v2, v3, v4):
            h = _merge(h, v)
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while p + 8 <= n:
        h = (_rotl(h ^ _round(0, int.from_bytes(data[p:p + 8], "little")), 27) * _P1 + _P4) & _M
        p += 8
    if p + 4 <= n:
        h = (_rotl(h ^ (int.from_bytes(data[p:p + 4], "little") * _P1 & _M), 23) * _P2 + _P3) & _M
        p += 4
    while p < n:
        h = (_rotl(h ^ (data[p] * _P5 & _M), 11) * _P1) & _M
        p += 1
    h ^= h >> 33
    h = (h * _P2) & _M
    h ^= h >> 29
    h = (h * _P3) & _M
    return h ^ (h >> 32)


def _key_matrix(W, count, rng):
    """count distinct rows of W bytes from 1 .. 255"""
    if W == 1:
        assert count <= 200
        return (rng.permutation(255)[:count] + 1).astype(np.uint8).reshape(count, 1)
    m = np.zeros((0, W), np.uint8)
    while len(m) < count:                             # (a collision among a few thousand random keys of two bytes happens; of more, hardly)
        m = np.unique(np.concatenate([m, rng.integers(1, 256, (count, W), dtype=np.uint8)]), axis=0)
    return np.ascontiguousarray(m[rng.permutation(len(m))[:count]])


def keys_of_width(W, count, rng):
    """count distinct keys of exactly W bytes, bytes from 1 .. 255 (W == 1: at most 200 of the 255 there are)"""
    return [bytes(r) for r in _key_matrix(W, count, rng)]


def pack(keys, slack=8):
    """(key_bytes, key_off) of a generation: the keys one behind the other, exactly `slack` readable bytes behind the last one (the
    contract of include/guber_gpu.h is 8) and no padding beyond — key_bytes is an allocation of its own of exactly that size, so
    AddressSanitizer's red zone starts at the ninth byte"""
    off = np.zeros(len(keys) + 1, np.uint32)
    if keys:
        off[1:] = np.cumsum([len(k) for k in keys])
    kb = np.empty(int(off[-1]) + slack, np.uint8)
    kb[:int(off[-1])] = np.frombuffer(b"".join(keys), np.uint8)
    kb[int(off[-1]):] = 0xA5                          # (what lies behind the last key is not zero: nothing may depend on it)
    return kb, off


def _pack_rows(M, ids, slack=8):
    """pack() for n requests that are rows of the key matrix M (the big generations)"""
    n, W = len(ids), M.shape[1]
    kb = np.empty(n * W + slack, np.uint8)
    kb[:n * W] = M[ids].reshape(-1)
    kb[n * W:] = 0xA5
    return kb, (np.arange(n + 1, dtype=np.uint64) * W).astype(np.uint32)


class Gen(HostBatch):
    """a generation: the HostBatch the device gets, plus what the checks need to know about it
         for_oracle   the HostBatch the oracle gets (the same one, or the one without the request the oracle does not model)
         odd          None, or (index, kind) of the one request that differs; kind "empty" / "too_long" are answered per item
         keys         the distinct keys that become resident -> True when they carry Behavior_GLOBAL"""


def _columns(n, g, now, limit, full, rng, behavior=None):
    algorithm = ((np.arange(n) // 97 + g) % 2).astype(np.uint8)              # both algorithms inside one generation
    duration = np.full(n, SHORT_MS if g % 3 == 2 else LONG_MS, np.int64)
    c = dict(hits=np.ones(n, np.int64), limit=limit.astype(np.int64), duration=duration, algorithm=algorithm,
             behavior=np.zeros(n, np.uint32) if behavior is None else behavior.astype(np.uint32), burst=None, created_at=None, is_owner=None)
    if full:
        c["burst"] = np.where(rng.random(n) < 0.5, 0, limit + 3).astype(np.int64)
        c["created_at"] = (now + rng.integers(-70, 70, n)).astype(np.int64)
        c["is_owner"] = (rng.random(n) < 0.8).astype(np.uint8)
    return c


def _batch(cls, keys, c, now, sel=None):
    pick = (lambda a: a) if sel is None else (lambda a: None if a is None else a[sel])
    return cls(pack(keys), pick(c["hits"]), pick(c["limit"]), pick(c["duration"]), now, burst=pick(c["burst"]), created_at=pick(c["created_at"]),
               algorithm=pick(c["algorithm"]), behavior=pick(c["behavior"]), is_owner=pick(c["is_owner"]))


def _make(g, keys, limit, full, rng, behavior=None, odd=None):
    now = NOW0 + g * STEP_MS
    n = len(keys)
    c = _columns(n, g, now, limit, full, rng, behavior)
    if odd is not None and odd[1] in ("empty", "too_long"):                   # the request Engine.eval is asked about once (error_answers)
        i = odd[0]
        c["hits"][i], c["limit"][i], c["duration"][i], c["algorithm"][i], c["behavior"][i] = 1, 10, LONG_MS, 0, 0
        if full:
            c["burst"][i], c["created_at"][i], c["is_owner"][i] = 0, now, 1
    hb = _batch(Gen, keys, c, now)
    hb.odd = odd
    if odd is not None and odd[1] in ("empty", "too_long"):
        sel = np.arange(n) != odd[0]
        hb.for_oracle = _batch(HostBatch, [k for i, k in enumerate(keys) if i != odd[0]], c, now, sel)
    else:
        hb.for_oracle = hb
    glob = np.zeros(n, bool) if behavior is None else (behavior & BEHAVIOR_GLOBAL) != 0
    hb.keys = {k: bool(glob[i]) for i, k in enumerate(keys) if not (odd is not None and i == odd[0] and odd[1] in ("empty", "too_long"))}
    return hb


def _limit_of(ids):
    return 5 + np.asarray(ids) % 26                   # 5 .. 30, one limit per key: hits = 1 over a few generations runs over the small ones


def _draw(rng, n, pop):
    """n ids below pop: half of them among the first 24 keys (so that keys run over their limit), half anywhere"""
    return np.where(rng.random(n) < 0.5, rng.integers(0, min(24, pop), n), rng.integers(0, pop, n))


_POPS = {}


def population(W):
    """the keys of width W the generations draw from (the same in every run: a placement can be fitted to them beforehand); the first 24
    are the hot ones (_draw)"""
    if W not in _POPS:
        _POPS[W] = keys_of_width(W, 200 if W == 1 else (1500 if W == 15 else 600), np.random.default_rng(9000 + W))
    return _POPS[W]


def observed_traffic(rng, n_shards, n=1 << 14):
    """(key_bytes, key_off) of n requests over the 15-byte population as the generations draw them, the first four hot keys a little hotter:
    what Placement.observe_keys is shown.  A key is heavy above an eighth of a shard's fair share (placement.cpp plan_locked: total /
    n_shards x heavy_fraction — 4.2 % of the traffic with three shards, 0.8 % with sixteen); the generations' 2 % per hot key is above
    that from seven shards on, so four keys get another 0.2 / n_shards of the traffic each: 1.6 times the threshold on their own"""
    pop = population(15)
    ids = np.where(rng.random(n) < 0.8 / n_shards, rng.integers(0, 4, n), _draw(rng, n, len(pop)))
    return pack([pop[i] for i in ids])


def generations(n_engines, place, rng, big=False, depth=3, max_key_bytes=1024):
    """yields (label, generation, full_columns) in a fixed order: the scenarios of the module's docstring; `depth` is the front's (a slot is
    reused every `depth` generations: a generation with one odd key is followed by a packed one `depth` later).  `place` routes the keys the
    skewed generations choose (None: one engine).  big: the two generations of BIG_N requests instead."""
    g = 0
    if big:
        M = _key_matrix(15, BIG_KEYS, rng)
        for k in range(2):
            now = NOW0 + g * STEP_MS
            ids = rng.integers(0, BIG_KEYS, BIG_N)
            kb, off = _pack_rows(M, ids)
            if k == 1:                                # the last key one byte longer: the generation is ragged, and only its last lane says so
                kb = np.concatenate([kb[:BIG_N * 15], np.array([0x5A], np.uint8), np.full(8, 0xA5, np.uint8)])
                off = off.copy(); off[BIG_N] += 1
            hb = Gen((kb, off), 1, _limit_of(ids), LONG_MS, now, algorithm=((np.arange(BIG_N) // 97 + g) % 2).astype(np.uint8))
            hb.odd, hb.for_oracle = None, hb
            u = np.unique(ids[:-1] if k == 1 else ids)
            hb.keys = {bytes(M[i]): False for i in u}
            if k == 1:
                hb.keys[bytes(M[ids[-1]]) + b"\x5a"] = False
            yield f"f big generation {k}: n={BIG_N} W=15" + (" last key 16 bytes" if k == 1 else ""), hb, False
            g += 1
        return

    def shard_of(keys):
        if place is None or n_engines == 1:
            return np.zeros(len(keys), np.uint32)
        return place.route_keys(*pack(keys))[0]

    pops = {W: population(W) for W in PACKED_WIDTHS + ONE_WIDTH_NOT_PACKED}
    reserve = {W: len(pops[W]) - len(pops[W]) // 5 for W in GLOBAL_WIDTHS}     # the last fifth of these populations is GLOBAL, always and only there

    def general(W):
        return pops[W][:reserve[W]] if W in reserve else pops[W]

    # a. widths x sizes: every width at n = 2 049 and at one of the smaller sizes (each of those twice)
    for k, W in enumerate(PACKED_WIDTHS + ONE_WIDTH_NOT_PACKED):
        for n in (2049, SIZES[k % 7]):
            pop = general(W)
            ids = _draw(rng, n, len(pop))
            full = g % 2 == 1
            yield f"a W={W} n={n} full={full}", _make(g, [pop[i] for i in ids], _limit_of(ids), full, rng), full
            g += 1

    # b. one odd key among 2 049 of width 15; blocks of `depth` such generations, then `depth` packed ones in the same slots
    pop = general(15)
    other = {14: keys_of_width(14, 8, rng), 16: keys_of_width(16, 8, rng)}
    cases = [(kind, pos) for kind in ("neighbour", "empty", "too_long") for pos in ODD_POSITIONS]
    for lo in range(0, len(cases), depth):
        block = cases[lo:lo + depth]
        for kind, pos in block:
            ids = _draw(rng, 2049, len(pop))
            keys = [pop[i] for i in ids]
            if kind == "neighbour":
                w = 14 if ODD_POSITIONS.index(pos) % 2 == 0 else 16
                keys[pos], what = other[w][ODD_POSITIONS.index(pos)], f"width {w}"
            else:
                keys[pos], what = (b"" if kind == "empty" else b"\x21" * (max_key_bytes + 1)), kind
            full = g % 2 == 1
            yield f"b W=15 n=2049 one key {what} at {pos} full={full}", _make(g, keys, _limit_of(ids), full, rng, odd=(pos, kind)), full
            g += 1
        for _ in block:
            ids = _draw(rng, 2049, len(pop))
            full = g % 2 == 1
            yield f"b W=15 n=2049 packed again in the slot of an odd one full={full}", _make(g, [pop[i] for i in ids], _limit_of(ids), full, rng), full
            g += 1

    # c. skew, keys chosen by the engine the placement's host rule names
    sh = shard_of(pop)
    by_engine = [np.nonzero(sh == e)[0] for e in range(n_engines)]
    assert all(len(b) for b in by_engine), [len(b) for b in by_engine]
    n = 2049
    skews = [("one key", np.full(n, by_engine[n_engines - 1][0])),
             ("all to the last engine", by_engine[n_engines - 1][rng.integers(0, len(by_engine[n_engines - 1]), n)]),
             ("all to engine 0", by_engine[0][rng.integers(0, len(by_engine[0]), n)]),
             ("request i to engine i mod n", np.array([by_engine[i % n_engines][rng.integers(0, len(by_engine[i % n_engines]))] for i in range(n)])),
             ("runs of 64 per engine", np.array([by_engine[(i // 64) % n_engines][rng.integers(0, len(by_engine[(i // 64) % n_engines]))] for i in range(n)]))]
    for what, ids in skews:
        full = g % 2 == 1
        yield f"c W=15 n={n} {what} full={full}", _make(g, [pop[i] for i in ids], _limit_of(ids), full, rng), full
        g += 1

    # d. GLOBAL: a third of the keys in play carry the bit, always
    for W in GLOBAL_WIDTHS:
        r = reserve[W]
        ng = len(pops[W]) - r
        for n in (2049, 1025):
            ids = np.where(rng.random(n) < 1 / 3, r + rng.integers(0, ng, n), rng.integers(0, 2 * ng, n))    # ng GLOBAL keys, 2 ng others
            beh = np.where(ids >= r, BEHAVIOR_GLOBAL, 0)
            full = g % 2 == 1
            yield f"d W={W} n={n} GLOBAL full={full}", _make(g, [pops[W][i] for i in ids], _limit_of(ids), full, rng, behavior=beh), full
            g += 1


def error_answers(engine, max_key_bytes=1024, now=NOW0):
    """what Engine.eval answers the empty and the over-long key with (the per-item errors of include/guber_gpu.h): {kind: row}; the request
    is the one _make() writes at the odd position.  `engine` is a scratch engine of the caller's."""
    out = {}
    for kind, key in (("empty", b""), ("too_long", b"\x21" * (max_key_bytes + 1))):
        res = engine.eval(HostBatch([key], 1, 10, LONG_MS, now, algorithm=0, behavior=0))
        out[kind] = res.rows()[0]
    assert out["empty"][4] == 4 and out["too_long"][4] == 7, out       # GUBER_ITEM_E_EMPTY_KEY, GUBER_ITEM_E_KEY_TOO_LONG
    return out


def result_arrays(n):
    """a generation's result arrays, n + TAIL long, filled with sentinels"""
    return dict(status=np.full(n + TAIL, SENTINEL_U8, np.uint8), err=np.full(n + TAIL, SENTINEL_U8, np.uint8),
                limit=np.full(n + TAIL, SENTINEL_I64, np.int64), remaining=np.full(n + TAIL, SENTINEL_I64, np.int64),
                reset_time=np.full(n + TAIL, SENTINEL_I64, np.int64))


def check_generation(label, hb, r, want, errors):
    """r: the result arrays (numpy, n + TAIL long) after the generation; want: the oracle's answers to hb.for_oracle"""
    n = hb.n
    for name, a in r.items():
        s = SENTINEL_U8 if a.dtype == np.uint8 else SENTINEL_I64
        assert len(a) == n + TAIL and (a[n:] == s).all(), f"{label}: {name} written behind the generation's end: {a[n:].tolist()}"
    got = HostResult(n)
    for name in ("status", "limit", "remaining", "reset_time", "err"):
        getattr(got, name)[:n] = r[name][:n]
    if hb.for_oracle is hb:
        assert_results_equal(got, want, label)
        return
    i, kind = hb.odd
    assert got.rows()[i] == errors[kind], f"{label}: the {kind} key's answer {got.rows()[i]}, Engine.eval's {errors[kind]}"
    rest = HostResult(n - 1)
    sel = np.arange(n) != i
    for name in ("status", "limit", "remaining", "reset_time", "err"):
        getattr(rest, name)[:n - 1] = r[name][:n][sel]
    assert_results_equal(rest, want, label + " (the other requests)")


def check_hashes(place, keys):
    """Placement.route_keys -> (shard, hash): the hash is XXH64 of the key (xxh64 above), the shard what guber_placement_shard says for it"""
    keys = list(keys)
    sh, hh = place.route_keys(*pack(keys))
    for k, s, h in zip(keys, sh.tolist(), hh.tolist()):
        assert h == xxh64(k), f"XXH64 of the {len(k)}-byte key {k!r}: {h:#x}, expected {xxh64(k):#x}"
        assert place.shard(h) == s, (k, s, place.shard(h))
    return sh


def check_residency(engs, place, keys, global_keys, global_engine, now, orc, probe_limit=None):
    """every key is resident (Engine.get_item, when the oracle still holds it at `now`) in the engine the placement's host rule names —
    GLOBAL keys in the global engine — and, by the engines' full listings (Engine.each), in no other; the engines hold as many items as
    the oracle.  probe_limit: look up only that many of the keys one by one (the listings still cover every key)"""
    keys, global_keys = list(keys), set(global_keys)
    sh = check_hashes(place, keys) if place is not None else np.zeros(len(keys), np.uint32)
    home = {k: (global_engine if k in global_keys and len(engs) > 1 else int(s)) for k, s in zip(keys, sh)}
    held = [set(it["key"] for it in e.each()) for e in engs]
    for j, hs in enumerate(held):
        stray = [k for k in hs if home.get(k) != j]
        assert not stray, f"engine {j} holds {len(stray)} keys that belong elsewhere (or to nobody), e.g. {stray[0]!r} of engine {home.get(stray[0])}"
    sizes = [e.size() for e in engs]
    assert sum(sizes) == orc.size() == len(home), (sizes, orc.size(), len(home))
    probe = set(keys if probe_limit is None else keys[::max(1, len(keys) // probe_limit)])
    for k, j in home.items():                         # (after the sizes: a lookup drops an item that has expired, lrucache.go:106-122)
        assert k in held[j], f"key {k!r} is not listed by engine {j}"
        if k not in probe:
            continue
        assert (engs[j].get_item(k, now) is not None) == (orc.get_item(k, now) is not None), f"key {k!r} in engine {j}: the engine's lookup and the oracle's disagree"
    return sizes


def drive(ga, engs, fr, place, orc, gens, device_side, fetch, errors, global_engine, threads=0, group=6, probe_limit=None):
    """the generations through fr.eval_dev, `group` per call (the routing runs ahead, slots go round), each against the oracle.
    device_side(hb, full, r) -> (GuberBatch, GuberResult, keep-alive) with r = result_arrays(n) as the result arrays' initial content;
    fetch(keep-alive) -> the result arrays as numpy after the call.  -> (generations run, the engines' sizes)"""
    keys, count, now = {}, 0, NOW0
    pending = []

    def flush():
        N = len(pending)
        if not N:
            return
        assert fr.eval_dev((GuberBatch * N)(*[p[3][0] for p in pending]), (GuberResult * N)(*[p[3][1] for p in pending]), N) == N
        fr.synchronize()
        for label, hb, full, side in pending:
            want = orc.eval(hb.for_oracle, threads=threads) if threads else orc.eval(hb.for_oracle)
            check_generation(label, hb, fetch(side[2]), want, errors)
        pending.clear()

    for label, hb, full in gens:
        side = device_side(hb, full, result_arrays(hb.n))
        pending.append((label, hb, full, side))
        for k, glob in hb.keys.items():
            assert keys.setdefault(k, glob) == glob, k                 # (a key is GLOBAL always or never)
        count += 1
        now = hb.now_ms
        if len(pending) == group:
            flush()
    flush()
    st = fr.stats()
    assert st["generations"] == count and st["forced_flushes"] == 0, st
    sizes = check_residency(engs, place, keys, [k for k, glob in keys.items() if glob], global_engine, now, orc, probe_limit)
    return count, sizes
