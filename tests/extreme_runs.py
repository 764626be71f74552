"""Scripts that send what the random streams and tests/eval_runs.py leave out through every batch pipeline: int64 extremes, negatives and
pre-loaded float64 Remaining (fractions, negatives, 2^53, 1e300) in uniform runs at ranks past a tile and in walked segments, items that
carry CacheItem.InvalidAt (cache.go:43-57), and created_at ranges on the thresholds of the owner-partitioned pipeline's packed range
(18 bits of offset from the batch clock, 8 bits of span: guber_kernels_part.h gm_pack).  Shared by tests/test_kernels_devsim.py (the
kernel source on the CPU) and tests/test_gpu_extreme_runs.py (the product library); numpy only — the engine and the oracle are the
caller's, and the reference for everything is the oracle.

Every case is (label, steps); a step is one of
    ("add", [keyword dicts for make_item])      LRUCache.Add of pre-loaded items
    ("eval", HostBatch)                         one batch
    ("get", key)                                LRUCache.GetItem at the clock of the last batch
    ("get", key, invalid_at)                    the same, and the item is there and still carries this non-zero InvalidAt
    ("compact",)                                a rebuild of the table (no-op for the oracle)
fed identically to the oracle and to the engine under test.

Shapes (eval_runs._layout's): hot keys 600 times each among 40 keys asked for once (every hot key in all tiles, the last tile partial),
257 times each (rank 256 is the first whose tile base is not 0), and 190 requests of hot keys + 10 others: one workgroup."""
import numpy as np

from gubernator_amd.abi import HostBatch

NOW0 = 1_700_000_500_000
TOKEN, LEAKY = 0, 1
GREGORIAN, RESET_REMAINING, DRAIN_OVER_LIMIT = 4, 8, 32
INVALID_ALGORITHM = 7
MINUTE = 60_000
SHAPES = [(600, 40), (257, 40), (190, 10)]          # the last one is the whole batch: its 190 are shared out among the hot keys
CHUNK = 37                                          # hot keys take turns in chunks of 37 requests: group sizes differ from tile to tile

# the value lists of test_extreme_value_runs_on_the_device (tests/test_gpu_parity.py)
I64 = [0, 1, -1, 2, 3, 7, 100, 2**31, 2**53, 2**53 + 1, 2**62, -(2**62), 2**63 - 1, -(2**63), 2**63 - 2, -(2**63) + 1]
F64 = [0.0, 0.5, 1.0, 1.5, -1.0, -0.25, 99.999, 2.0**53, 2.0**53 + 2, 9.3e18, -9.3e18, 1e300, -1e300, 3.0, 10.0]
DURATIONS = [0, 1, 3, 1000, 60_000, -1, -(2**62), 2**62, 2**63 - 1]
BURSTS = [0, 0, 15, -3, 2**62, 2**63 - 1]
BEHAVIORS = [0, 0, 32, 8, 40]
CLOCK_STEPS = [0, 1, 40, 1200, 70_000]


def layout(tag, shape, hot):
    """-> (keys, [positions of hot key h], positions of the others) for `hot` hot keys in a batch of the given shape"""
    run, others = shape
    counts = [run] * hot if run + others > 256 else [run // hot + (1 if h < run % hot else 0) for h in range(hot)]
    n = sum(counts) + others
    other_at = (np.arange(others) * n // others + n // (2 * others)).astype(np.int64)
    is_hot = np.ones(n, bool)
    is_hot[other_at] = False
    owner = np.full(n, -1, np.int64)
    left, h = list(counts), 0
    slots = np.nonzero(is_hot)[0]
    p = 0
    while p < len(slots):
        while left[h] == 0:
            h = (h + 1) % hot
        take = min(CHUNK, left[h])
        owner[slots[p:p + take]] = h
        left[h] -= take
        p += take
        h = (h + 1) % hot
    keys, o = [], 0
    for i in range(n):
        if owner[i] >= 0:
            keys.append(f"hot_{tag}_{owner[i]}".encode())
        else:
            keys.append(f"one_{tag}_{o}".encode())
            o += 1
    return keys, [np.nonzero(owner == h)[0] for h in range(hot)], other_at


def _columns(n, now):
    return dict(hits=np.ones(n, np.int64), limit=np.full(n, 100, np.int64), duration=np.full(n, MINUTE, np.int64), burst=np.zeros(n, np.int64),
                created_at=np.full(n, now, np.int64), algorithm=np.zeros(n, np.uint8), behavior=np.zeros(n, np.uint32))


def _batch(keys, c, now, **extra):
    return HostBatch(keys, c["hits"], c["limit"], c["duration"], now, burst=c["burst"], created_at=c["created_at"], algorithm=c["algorithm"],
                     behavior=c["behavior"], **extra)


def _gets(keys, ats):
    return [("get", keys[int(at[0])]) for at in ats]


def _extreme_item(rng, key, t):
    """an item of either algorithm with extreme fields, as test_extreme_value_runs_on_the_device draws it"""
    return dict(key=key, algorithm=int(rng.integers(0, 2)), limit=int(rng.choice(I64)), duration=int(rng.choice([1000, 60_000, 0, -5, 2**62])),
                remaining=int(rng.choice(I64)), remaining_f=float(rng.choice(F64)), stamp=t - int(rng.choice([0, 1, 999, 10**9])),
                burst=int(rng.choice(I64[:8] + [2**62])), expire_at=t + int(rng.choice([0, 1, 60_000, -1, 2**62])))


def _extreme_request(rng, t):
    return dict(hits=int(rng.choice(I64 + [1, 1, 1, 2, 5])), limit=int(rng.choice(I64 + [10, 100])), duration=int(rng.choice(DURATIONS)),
                algorithm=int(rng.choice([0, 1])), behavior=int(rng.choice(BEHAVIORS)), burst=int(rng.choice(BURSTS)),
                created_at=int(rng.choice([t, t, t - 5, t + 5, 0, -1, 2**62, -(2**62), t - 10**9])))


def _put(c, at, req):
    for name, v in req.items():
        c[name][at] = v


# ---- case 1 -----------------------------------------------------------------------------------------------------------------------
BIG = 2**63 - 1


def _edge_specs(t):
    """(item, request) pairs that drive mul_lt (rank x hits against Remaining in 128 bits) to its edges: with hits 2^55 the product passes
    2^63 - 1 at rank 256 exactly, with 2^62 it wraps at rank 2, with 3 it never does; 2^53 and 2^53 + 1 are where float64 stops
    telling integers apart"""
    tok = lambda rem, limit: dict(algorithm=TOKEN, limit=limit, duration=MINUTE, remaining=rem, stamp=t, expire_at=t + MINUTE)
    lky = lambda rem, limit: dict(algorithm=LEAKY, limit=limit, duration=MINUTE, remaining_f=rem, stamp=t, burst=limit, expire_at=t + MINUTE)
    req = lambda algo, hits, limit: dict(algorithm=algo, hits=hits, limit=limit, duration=MINUTE, burst=0, created_at=t)
    return [(tok(BIG, BIG), req(TOKEN, 2**62, BIG)), (tok(BIG, BIG), req(TOKEN, 2**55, BIG)), (tok(BIG, BIG), req(TOKEN, 3, BIG)),
            (tok(2**53, 2**62), req(TOKEN, 1, 2**62)), (tok(2**53 + 1, 2**62), req(TOKEN, 1, 2**62)),
            (lky(2.0**53, 2**62), req(LEAKY, 1, 2**62)), (lky(2.0**53 + 2, 2**62), req(LEAKY, 1, 2**62)), (lky(2.0**53, 2**53), req(LEAKY, 1, 2**53))]


def extreme_uniform_cases(trials=100, seed=2026, now=NOW0):
    """-> [(label, steps)]: the edges of _edge_specs four keys to a batch, at every shape, with and without DRAIN_OVER_LIMIT, twice in a row;
    then `trials` scripts of 3-4 hot keys (1-3 in the one-workgroup shape), each pre-loaded with probability 0.7, and 1-3 phases in
    which every hot key's requests are identical and extreme; the others draw one extreme request each"""
    out = []
    t = now
    for si, shape in enumerate(SHAPES):
        for drain in (0, DRAIN_OVER_LIMIT):
            specs = _edge_specs(t)
            for half in range(2):
                mine = specs[4 * half:4 * half + 4]
                keys, ats, _ = layout(f"e{si}_{drain}_{half}", shape, len(mine))
                steps = [("add", [dict(item, key=keys[int(at[0])]) for (item, _), at in zip(mine, ats)])]
                for again in range(2):
                    c = _columns(len(keys), t + again)
                    for (_, req), at in zip(mine, ats):
                        _put(c, at, dict(req, created_at=t + again, behavior=drain))
                    steps += [("eval", _batch(keys, c, t + again))] + _gets(keys, ats)
                out.append((f"edges of rank x hits, shape {shape}, keys {4 * half}..{4 * half + 3}{' DRAIN' if drain else ''}", steps))
            t += 10
    rng = np.random.default_rng(seed)
    for trial in range(trials):
        shape = SHAPES[trial % 3]
        hot = int(rng.integers(3, 5)) if shape[0] + shape[1] > 256 else int(rng.integers(1, 4))
        keys, ats, other_at = layout(f"u{trial}", shape, hot)
        t = now + 1000 + int(rng.integers(0, 10_000))
        steps, items = [], [_extreme_item(rng, keys[int(at[0])], t) for at in ats if rng.random() < 0.7]
        if items:
            steps.append(("add", items))
        for phase in range(int(rng.integers(1, 4))):
            c = _columns(len(keys), t)
            for at in ats:
                _put(c, at, _extreme_request(rng, t))
            for i in other_at:
                _put(c, i, _extreme_request(rng, t))
            steps += [("eval", _batch(keys, c, t))] + _gets(keys, ats)
            t += int(rng.choice(CLOCK_STEPS))
        out.append((f"uniform extremes, trial {trial}, shape {shape}, {hot} hot keys", steps))
    return out


# ---- case 2 -----------------------------------------------------------------------------------------------------------------------
def extreme_walk_cases(trials=18, seed=2027, now=NOW0 + 100_000):
    """-> [(label, steps)]: the pre-loads of case 1, but every request of a hot key draws its own hits, limit, duration, burst, behaviour and
    algorithm — limit 0 and negative limits (rate = duration / limit is +-Inf or NaN), rates that are no integers (1000 / 7, 1 / 3), an
    invalid algorithm here and there: the segment is walked serially.  Then leaky keys whose requests differ in created_at only, by
    amounts that leak fractions of a token."""
    out = []
    rng = np.random.default_rng(seed)
    limits = np.array(I64 + [0, 0, -7, 7, 3, 10, 100], dtype=object)
    durations = np.array(DURATIONS + [1000, 1000, 1, 1], dtype=object)
    for trial in range(trials):
        shape = SHAPES[trial % 3]
        hot = 3 if shape[0] + shape[1] > 256 else 2
        keys, ats, _ = layout(f"w{trial}", shape, hot)
        n = len(keys)
        t = now + int(rng.integers(0, 10_000))
        steps, items = [], [_extreme_item(rng, keys[int(at[0])], t) for at in ats if rng.random() < 0.7]
        if items:
            steps.append(("add", items))
        for phase in range(2):
            c = _columns(n, t)
            for h, at in enumerate(ats):
                m = len(at)
                if h == 0:                                      # rates that are no integers, limits around 0: the float path of the leaky walk
                    c["limit"][at] = rng.choice([7, 3, 0, -7, 1, 100], m)
                    c["duration"][at] = rng.choice([1000, 1, MINUTE], m)
                    c["hits"][at] = rng.choice([1, 1, 0, 2, -1, 2**62], m)
                    c["algorithm"][at] = rng.choice([LEAKY, LEAKY, LEAKY, TOKEN], m)
                else:
                    c["limit"][at] = rng.choice(limits, m).astype(np.int64)
                    c["duration"][at] = rng.choice(durations, m).astype(np.int64)
                    c["hits"][at] = rng.choice(np.array(I64 + [1, 1, 1, 2, 5], dtype=object), m).astype(np.int64)
                    c["algorithm"][at] = rng.integers(0, 2, m)
                c["burst"][at] = rng.choice(np.array(BURSTS, dtype=object), m).astype(np.int64)
                c["behavior"][at] = rng.choice(BEHAVIORS, m)
                c["algorithm"][at[rng.random(m) < 0.03]] = INVALID_ALGORITHM
            steps += [("eval", _batch(keys, c, t))] + _gets(keys, ats)
            t += int(rng.choice(CLOCK_STEPS))
        out.append((f"walked extremes, trial {trial}, shape {shape}", steps))
    # leaky buckets with a fraction of a token left; the requests differ in created_at only, 60 ms a token (and 1000 / 7 ms a token)
    for si, shape in enumerate(SHAPES):
        hot = 3 if shape[0] + shape[1] > 256 else 2
        keys, ats, _ = layout(f"wc{si}", shape, hot)
        t = now + 50_000 + si
        rems, lims = [500.25, 0.75, 3.5], [1000, 1000, 7]
        steps = [("add", [dict(key=keys[int(at[0])], algorithm=LEAKY, limit=lims[h], duration=MINUTE if h < 2 else 1000, remaining_f=rems[h], stamp=t - 7,
                               burst=lims[h], expire_at=t + MINUTE) for h, at in enumerate(ats)])]
        for phase in range(2):
            c = _columns(len(keys), t)
            c["algorithm"][:] = LEAKY
            for h, at in enumerate(ats):
                c["limit"][at] = lims[h]
                c["duration"][at] = MINUTE if h < 2 else 1000
                c["hits"][at] = 1 if phase == 0 else 0
                c["created_at"][at] = t + np.sort(rng.integers(0, 400, len(at)))
            steps += [("eval", _batch(keys, c, t))] + _gets(keys, ats)
            t += 25
        out.append((f"walked leaky keys that differ in created_at only, fractions of a token, shape {shape}", steps))
    return out


# ---- case 3 -----------------------------------------------------------------------------------------------------------------------
def _invalid_values(now):
    return [0, now - 1, now, now + 1, now + MINUTE, 2**62, -1]


def _stored(key, algo, now, invalid_at, expire_at):
    """a bucket half used, of limit 100 a minute: what the plain requests of case 3 ask for"""
    if algo == TOKEN:
        return dict(key=key, algorithm=TOKEN, limit=100, duration=MINUTE, remaining=50, stamp=now - 10, expire_at=expire_at, invalid_at=invalid_at)
    return dict(key=key, algorithm=LEAKY, limit=100, duration=MINUTE, remaining_f=50.5, stamp=now - 10, burst=100, expire_at=expire_at, invalid_at=invalid_at)


def invalid_at_cases(now=NOW0 + 200_000):
    """-> [(label, steps)]: scripts of one algorithm each (a request of the other algorithm would replace the item, and the new item has
    invalid_at 0 for the rest of the script).  Items pre-loaded with invalid_at in {0, now - 1, now, now + 1, now + 60 000, 2^62, -1} and
    expire_at in {now + 60 000, now - 1} — the hot keys four combinations to a script, the keys asked for once cycle through all of them —,
    then (i) / (ii) the plain run of the script's algorithm at now (hits 1, limit and duration the stored ones), (iii) a walked segment
    at now + 1, (iv) the plain run again at now + 2 and now + 60 001, where items expire by InvalidAt alone and come back with invalid_at 0;
    GetItem of the hot keys and of eight others after every batch; a rebuild of the table and GetItem again after the batch at now + 2 (items
    with invalid_at now + 60 000 and 2^62 are alive there) and at the end.  A get whose item must still carry the invalid_at it was loaded
    with says so: ("get", key, invalid_at) — checked on the oracle's answer, so that no batch meets items without InvalidAt only."""
    out = []
    for si, shape in enumerate(SHAPES):
        for algo in (TOKEN, LEAKY):
            t = now + (2 * si + algo) * 200_000
            combos = [(inv, exp) for inv in _invalid_values(t) for exp in (t + MINUTE, t - 1)]
            for g in range(0, len(combos), 4):
                mine = combos[g:g + 4]
                keys, ats, other_at = layout(f"i{si}_{algo}_{g}", shape, len(mine))
                n = len(keys)
                loaded = [(keys[int(at[0])], inv, exp) for (inv, exp), at in zip(mine, ats)]
                loaded += [(keys[int(i)],) + combos[(g + 3 * j) % len(combos)] for j, i in enumerate(other_at[:8])]
                steps = [("add", [_stored(k, algo, t, inv, exp) for k, inv, exp in loaded] +
                                 [_stored(keys[int(i)], algo, t, *combos[(g + 3 * j) % len(combos)]) for j, i in enumerate(other_at) if j >= 8])]

                def watch(clock):
                    """the gets after the batch at `clock`: an item loaded alive (expire_at not passed at the first batch) whose invalid_at
                    has not passed by `clock` has been updated in place by every batch so far"""
                    return [("get", k, inv) if inv != 0 and inv >= clock and exp >= t else ("get", k) for k, inv, exp in loaded]

                def plain(clock):
                    c = _columns(n, clock)
                    c["algorithm"][:] = algo
                    return [("eval", _batch(keys, c, clock))] + watch(clock)
                steps += plain(t)
                c = _columns(n, t + 1)                                  # the walk: hits 1, 2, 1, 2, ...
                c["algorithm"][:] = algo
                for at in ats:
                    c["hits"][at] = 1 + np.arange(len(at)) % 2
                steps += [("eval", _batch(keys, c, t + 1))] + watch(t + 1)
                steps += plain(t + 2) + [("compact",)] + watch(t + 2)
                # (a token bucket keeps the expire_at it was loaded with, now + 60 000: at now + 60 001 it has expired by that as well; a
                # leaky bucket's expire_at follows its last request, so InvalidAt alone decides and 2^62 is alive at the end)
                end = [("get", k, inv) if algo == LEAKY and inv == 2**62 and exp >= t else ("get", k) for k, inv, exp in loaded]
                steps += plain(t + MINUTE + 1)[:1] + end + [("compact",)] + end
                out.append((f"InvalidAt, {'leaky' if algo else 'token'}, shape {shape}, combinations {g}..{g + len(mine) - 1}", steps))
    return out


def invalid_at_steady_case(invalid_at_of_odd_keys, shape=SHAPES[0], now=NOW0 + 900_000):
    """-> (steps, groups of keys with invalid_at 0, groups of the others): token items of limit 100 a minute, no burst, and the steady-state
    batch of case 3 (i) on them — hits 1, the stored limit and duration.  Even keys (the hot key first) carry invalid_at 0, odd ones the
    given value: with 0 everywhere every (key, tile) group of the owner-partitioned pipeline is answered by a 32-byte record."""
    keys, ats, other_at = layout(f"s{invalid_at_of_odd_keys != 0}", shape, 2)
    order = [keys[int(at[0])] for at in ats] + [keys[int(i)] for i in other_at]
    items = [_stored(k, TOKEN, now, invalid_at_of_odd_keys if j % 2 else 0, now + MINUTE) for j, k in enumerate(order)]
    c = _columns(len(keys), now)
    tiles = lambda at: len(np.unique(np.asarray(at) // 256))
    groups = [tiles(ats[0]) + len(other_at[0::2]), tiles(ats[1]) + len(other_at[1::2])]
    return [("add", items), ("eval", _batch(keys, c, now)), ("eval", _batch(keys, c, now + 1))] + _gets(keys, ats), groups[0], groups[1]


# ---- case 4 -----------------------------------------------------------------------------------------------------------------------
FAR_LO, FAR_HI = -131072, 131071                 # k_part: created_at - now outside [FAR_LO, FAR_HI] does not fit the message (G_CFAR)


def created_at_edge_cases(greg_fn, now=NOW0 + 2_000_000):
    """-> [(label, steps)]: for token and for leaky buckets, four resident hot keys — limit 1 in 10^12 ms (no offset below leaks or expires
    it), limit 1000 a minute (131 s expire it, 60 ms leak a token), limit 1000 in ten minutes (131 s leak 218 tokens and expire
    nothing: the sign of the offset decides) and limit 1 in 131 072 ms (a request at -131073 leaves the bucket expired for the requests
    behind it, one at +131071 leaks nothing: what -131073 turns into in 18 bits) — whose requests differ in created_at only: all at one offset from the batch clock on either
    side of both thresholds; one request 255 / 256 ms from the rest of its tile's group (these also with hits 0 and in one workgroup's
    batch); the key's group of tile 0 at [0, 255] and that of tile 1 at [1, 256] / at [0, 255] again; a group out of range next to groups
    in range; 255 ms that straddle a threshold.  Every script makes its buckets resident at the clock of the run (offset 0 leaks
    nothing), then runs.  Last, a DURATION_IS_GREGORIAN key (hours) whose host-precomputed greg_expire differs between its first
    and its second tile, and its twin with equal values.  greg_fn(now_ms, d) -> (greg_expire, greg_duration)."""
    def one(d):
        return lambda at, tile: np.full(len(at), d, np.int64)

    def odd_one(base, d):                           # everybody at `base`, the third request of tile 0's group d later
        def f(at, tile):
            off = np.full(len(at), base, np.int64)
            off[np.nonzero(tile == tile[0])[0][2]] = base + d
            return off
        return f

    def per_tile(ranges):                           # ranges[k] = (lo, hi) of the key's k-th tile (the last one for the tiles after it)
        def f(at, tile):
            off = np.zeros(len(at), np.int64)
            for k, tl in enumerate(np.unique(tile)):
                lo, hi = ranges[min(k, len(ranges) - 1)]
                idx = np.nonzero(tile == tl)[0]
                off[idx] = lo
                off[idx[1]] = hi
            return off
        return f

    patterns = [(f"all at {d:+d}", one(d), True) for d in (FAR_LO - 1, FAR_LO, FAR_LO + 1, FAR_HI - 1, FAR_HI, FAR_HI + 1)]
    patterns += [("one request 255 later", odd_one(0, 255), True), ("one request 256 later", odd_one(0, 256), True),
                 ("one request 255 earlier", odd_one(0, -255), False), ("one request 256 earlier", odd_one(0, -256), False),
                 ("tile 0 at [0, 255], then [1, 256]", per_tile([(0, 255), (1, 256)]), False),
                 ("every tile at [0, 255]", per_tile([(0, 255)]), False),
                 ("tile 0 at [0, 255], then [0, 256]", per_tile([(0, 255), (0, 256)]), False),
                 # a group that is out of range next to groups that are in range, or out of range elsewhere: no range describes the key
                 ("tile 0 at +131072, then -5", per_tile([(FAR_HI + 1, FAR_HI + 1), (-5, -5)]), False),
                 ("tile 0 at +131072, then +200000", per_tile([(FAR_HI + 1, FAR_HI + 1), (200_000, 200_000)]), False),
                 ("tile 0 at -131072, then -5", per_tile([(FAR_LO, FAR_LO), (-5, -5)]), False),
                 ("tile 0 at -131073, then 0", per_tile([(FAR_LO - 1, FAR_LO - 1), (0, 0)]), False),
                 ("tile 0 at -131073, then +70000", per_tile([(FAR_LO - 1, FAR_LO - 1), (70_000, 70_000)]), False),
                 ("255 ms across the lower threshold", odd_one(FAR_LO - 100, 255), False),
                 ("255 ms up to the upper threshold", odd_one(FAR_HI - 255, 255), False),
                 ("256 ms up to past the upper threshold", odd_one(FAR_HI - 255, 256), False)]
    out = []
    t = now
    buckets = [(1, 10**12), (1000, MINUTE), (1000, 10 * MINUTE), (1, -FAR_LO)]
    for algo in (TOKEN, LEAKY):
        for pi, (what, offsets, every_way) in enumerate(patterns):
            for hits, shape in [(1, SHAPES[0])] + ([(0, SHAPES[0]), (1, SHAPES[2])] if every_way else []):
                keys, ats, _ = layout(f"c{algo}_{pi}_{hits}_{shape[0]}", shape, len(buckets))
                c = _columns(len(keys), t)
                c["algorithm"][:] = algo
                c["hits"][:] = 0
                for at, (limit, duration) in zip(ats, buckets):
                    c["limit"][at] = limit
                    c["duration"][at] = duration
                steps = [("eval", _batch(keys, c, t))]                     # resident, untouched
                c = {k: v.copy() for k, v in c.items()}
                c["hits"][:] = hits
                for at in ats:
                    c["created_at"][at] = t + offsets(at, at // 256)
                steps += [("eval", _batch(keys, c, t))] + _gets(keys, ats)
                out.append((f"created_at, {'leaky' if algo else 'token'}, {what}, hits {hits}, shape {shape}", steps))
                t += 3
    # calendar columns that differ inside one key: the message cannot carry them (G_ODD), more than one group of such a key is walked
    for algo in (TOKEN, LEAKY):
        for differ in (True, False):
            keys, ats, _ = layout(f"g{algo}_{int(differ)}", SHAPES[0], 2)
            n = len(keys)
            steps = []
            for again in range(2):
                c = _columns(n, t)
                c["algorithm"][:] = algo
                ge, gd = np.zeros(n, np.int64), np.zeros(n, np.int64)
                for at in ats:
                    c["behavior"][at] = GREGORIAN
                    c["duration"][at] = 1
                    c["limit"][at] = 1000
                    ge[at], gd[at] = greg_fn(t, 1)
                    if differ:
                        tile = at // 256
                        ge[at[tile == np.unique(tile)[1]]] += 1000
                steps += [("eval", _batch(keys, c, t, greg_expire=ge, greg_duration=gd))] + _gets(keys, ats)
                t += 1
            out.append((f"calendar columns {'that differ between the tiles of one key' if differ else 'equal in every tile'}, {'leaky' if algo else 'token'}", steps))
    return out


# ---- the driver both callers use ----------------------------------------------------------------------------------------------------
ITEM_FIELDS = ("algorithm", "status", "limit", "duration", "remaining", "stamp", "burst", "expire_at", "invalid_at")


def assert_items_equal(got, want, what):
    """GetItem's answers field by field; remaining_f equal or NaN on both sides, nothing else has slack"""
    if got is None or want is None:
        assert got is None and want is None, (what, got, want)
        return
    for f in ITEM_FIELDS:
        assert got[f] == want[f], (what, f, got, want)
    a, b = got["remaining_f"], want["remaining_f"]
    assert a == b or (a != a and b != b), (what, "remaining_f", got, want)


def run_script(label, steps, backend, oracle, make_item, assert_results_equal, after_eval=None):
    """one case through `backend` and the oracle, step by step.  backend: add(items), eval(batch) -> (result, the batch's counters: over,
    hits, misses and as many more of HostResult.counters() as it has), get(key, now_ms), compact(now_ms), size(), each() -> items or
    None; after_eval(k, batch) is the caller's hook (which kernels ran)."""
    clock = None
    for k, step in enumerate(steps):
        what = f"{label}, step {k} ({step[0]})"
        if step[0] == "add":
            for d in step[1]:
                oracle.add_item(make_item(**d))
            backend.add([make_item(**d) for d in step[1]])
        elif step[0] == "eval":
            b = step[1]
            clock = b.now_ms
            want = oracle.eval(b)
            got, counted = backend.eval(b)
            assert_results_equal(got, want, what)
            assert tuple(counted) == want.counters()[:len(counted)], (what, counted, want.counters())
            if after_eval is not None:
                after_eval(k, b)
        elif step[0] == "get":
            assert clock is not None, "a get follows a batch"
            want = oracle.get_item(step[1], clock)
            if len(step) > 2:
                assert step[2] != 0 and want is not None and want["invalid_at"] == step[2], (what, step, want)
            assert_items_equal(backend.get(step[1], clock), want, f"{what} {step[1]!r}")
        elif step[0] == "compact":
            backend.compact(clock)
            items = backend.each()
            if items is not None:
                by_key = lambda d: d["key"]
                got, want = sorted(items, key=by_key), sorted(oracle.each(), key=by_key)
                assert [d["key"] for d in got] == [d["key"] for d in want], what
                for g, w in zip(got, want):
                    assert_items_equal(g, w, f"{what} each {w['key']!r}")
        else:
            raise AssertionError(step[0])
        assert backend.size() == oracle.size(), (what, backend.size(), oracle.size())
