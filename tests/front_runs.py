"""Generations for the device front's copy kernels (k_fr_scatter / k_fr_out, gubernator_amd/csrc/guber_kernels_front.h) at the edges of
their index arithmetic, and the checks that go with them; shared by tests/test_gpu_front_runs.py (the product library on a GPU) and
tests/test_front_runs_cpu.py (the generators themselves).  numpy only, like tests/front_edges.py, whose keys, buffers and checks it uses.

The two kernels put a tile of 1 024 requests into the shares' order in LDS: request i = (engine e, rank) has the local place lbase[e] + rank,
lbase the exclusive prefix of the tile's sixteen counts, and sorted element j finds its engine back from lbase alone.  What that can get wrong
is decided by HOW A TILE'S REQUESTS ARE SPREAD OVER THE ENGINES, so every generation here is built from a plan — the engine of every
request — and keys chosen by the engine the placement's rule gives them:
  one          everything to one (middle) engine: a run of 1 024, every lbase below it 0 and every one above it 1 024
  last         everything to the last engine, all others empty
  ends         only the first and the last engine populated: the empty ones between them have the last one's lbase
  single_first one engine holds exactly ONE request of the whole generation, the first of the last tile; the others share the rest
  single_last  ... the last request of the first tile
  mod          request i to engine i mod n
  tail_middle  i mod n in the full tiles, a last partial tile whose only requests go to a middle engine
Sizes: one below, at and above the thread stride (256) and the tile (1 024), two and four tiles plus one.  Keys: one width of 7, 8, 9,
16, 32 bytes per generation (bytes; whole words; whole words and an overlapping last one), and per size above 1 one ragged generation — a
single key of another width, the last request of a run — followed `depth` generations later, in the same slot, by a packed one of that size.
burst / created_at / is_owner are present in every second generation."""
import numpy as np

import front_edges as fe
from gubernator_amd.abi import GuberBatch, GuberResult

TILE = 1024
SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 2049, 4097)
ENGINE_COUNTS = (1, 2, 12, 16)
WIDTHS = (7, 8, 9, 16, 32)
ODD_WIDTH = 11                                        # the one key of a ragged generation
PLANS = ("one", "last", "ends", "single_first", "single_last", "mod", "tail_middle")
KEYS_PER_ENGINE = 28                                  # per width, on average: five widths and the odd keys make about 150 keys per engine ...
CACHE_PER_ENGINE = 96                                 # ... over caches of 96 items: they bind (the oracle's workers hold as many each)


def lone_engine(n_engines):
    """the engine that holds exactly one request in the single_* plans"""
    return 1 if n_engines > 2 else n_engines - 1


def plan(kind, n, n_engines):
    """-> uint32[n]: the engine of every request"""
    E, i = n_engines, np.arange(n)
    mid = E // 2
    if kind == "one":
        return np.full(n, mid, np.uint32)
    if kind == "last":
        return np.full(n, E - 1, np.uint32)
    if kind == "ends":
        return np.where((i * 7 // 3) % 2 == 0, 0, E - 1).astype(np.uint32)
    if kind in ("single_first", "single_last"):
        lone = lone_engine(E)
        others = np.array([e for e in range(E) if e != lone] or [0], np.uint32)
        out = others[i % len(others)]
        at = (n - 1) // TILE * TILE if kind == "single_first" else min(n, TILE) - 1
        out[at] = lone
        return out
    if kind == "mod":
        return (i % E).astype(np.uint32)
    if kind == "tail_middle":
        return np.where(i >= n // TILE * TILE, mid, i % E).astype(np.uint32)
    raise ValueError(kind)


def run_end(engines):
    """the last request of the first tile's longest run (the first such engine's): where a ragged generation's odd key goes"""
    first = engines[:TILE]
    e = int(np.argmax(np.bincount(first)))
    return int(np.nonzero(first == e)[0][-1])


def pools(n_engines, route, rng):
    """{width: [keys of engine 0, keys of engine 1, ...]} for WIDTHS and ODD_WIDTH; route(keys) -> the engine of every key (the placement's
    host rule; None: one engine)"""
    out = {}
    for W in WIDTHS + (ODD_WIDTH,):
        keys = fe.keys_of_width(W, KEYS_PER_ENGINE * n_engines, rng)
        sh = np.zeros(len(keys), np.uint32) if route is None else np.asarray(route(keys))
        out[W] = [[k for k, s in zip(keys, sh.tolist()) if s == e] for e in range(n_engines)]
        assert all(len(b) >= 2 for b in out[W]), (W, [len(b) for b in out[W]])
    return out


def generations(n_engines, route, rng, depth=3):
    """yields (label, generation, full_columns, engines): per size a ragged generation and one per plan — the packed one `depth` later lies in
    the ragged one's slot — the widths going round.  engines: the plan the keys were chosen by."""
    assert len(PLANS) >= depth
    P = pools(n_engines, route, rng)
    g = 0

    def make(kind, n, W, odd_at=None):
        nonlocal g
        engines = plan(kind, n, n_engines)
        pick = rng.integers(0, 1 << 30, n)
        keys = [P[W][e][r % len(P[W][e])] for e, r in zip(engines.tolist(), pick.tolist())]
        ids = np.array([hash_id(k) for k in keys])
        what = f"W={W}"
        if odd_at is not None:
            b = P[ODD_WIDTH][int(engines[odd_at])]
            keys[odd_at] = b[int(pick[odd_at]) % len(b)]
            what = f"W={W} one key of {ODD_WIDTH} bytes at {odd_at}"
        full = g % 2 == 1
        hb = fe._make(g, keys, fe._limit_of(ids), full, rng)
        g += 1
        return f"n={n} engines={n_engines} {kind} {what} full={full}", hb, full, engines

    for n in SIZES:
        W0 = WIDTHS[g % len(WIDTHS)]
        yield make("mod", n, W0, odd_at=run_end(plan("mod", n, n_engines)) if n > 1 else None)      # (one request is one width)
        for k, kind in enumerate(PLANS):
            yield make(kind, n, W0 if k == depth - 1 else WIDTHS[g % len(WIDTHS)])      # (k == depth - 1: the ragged one's slot, its width again)


def hash_id(key):
    """a small number per key (its limit follows from it: one limit per key)"""
    return int.from_bytes(key[:4], "little") % 1000


def drive(engs, fr, orc, gens, device_side, fetch, depth=3):
    """the generations through fr.eval_dev, two, three and depth + 1 per call in turn (the routing runs ahead; the slots go round across
    the calls, and inside one of depth + 1 a slot is routed into again behind its own answers), each against the
    oracle: answers in arrival order, the sentinels behind n untouched (front_edges.check_generation), nothing forced, no retries, as many
    resident items as the oracle holds.  device_side / fetch as front_edges.drive takes them.  -> generations run"""
    retries0 = sum(e.stats()["retries"] for e in engs)
    count, pending, groups = 0, [], [2, 3, depth + 1]

    def flush():
        N = len(pending)
        assert fr.eval_dev((GuberBatch * N)(*[p[2][0] for p in pending]), (GuberResult * N)(*[p[2][1] for p in pending]), N) == N
        fr.synchronize()
        for label, hb, side in pending:
            fe.check_generation(label, hb, fetch(side[2]), orc.eval(hb), {})
        pending.clear()

    for label, hb, full, _ in gens:
        pending.append((label, hb, device_side(hb, full, fe.result_arrays(hb.n))))
        count += 1
        if len(pending) == groups[0]:
            flush()
            groups.append(groups.pop(0))
    if pending:
        flush()
    st = fr.stats()
    assert st["generations"] == count and st["forced_flushes"] == 0, st
    assert sum(e.stats()["retries"] for e in engs) == retries0
    sizes = [e.size() for e in engs]
    assert sum(sizes) == orc.size(), (sizes, orc.size())
    return count
