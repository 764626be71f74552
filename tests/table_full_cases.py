"""Cases for the two ways the open-addressed table (gubernator_amd/csrc/guber_table.h) refuses a new key with GUBER_ITEM_E_TABLE_FULL — the
long-key arena and the probe bound — and for probe chains that cross the table's end; shared by tests/test_gpu_table_full.py (the product
library on a GPU) and tests/test_table_full_cpu.py (the same kernels compiled for the CPU).  numpy plus support / streams only.  Every case
takes an engine factory (keyword arguments of gubernator_amd.Engine -> engine) and a pipeline of PIPELINES, and compares with the oracle.

Geometry unless a case says otherwise: table_slots 4 096, max_key_bytes 512, max_batch 1 024, long keys of 408 bytes: the arena is exactly
1 MiB = 1 048 576 bytes, 2 570 such keys fill 1 048 560 of them, and the directory asks for a rebuild above 3 584 tags.

  1  churn over a cache of 1 000: the arena's bound — not the tag limit — asks for the rebuilds, nothing is refused
  2  a cache's worth (3 000) of keys of 63 .. 512 bytes, twins that differ in the last byte or are one byte longer: the arena grows, the
     keys survive the rebuilds
  3  GUBER_FLAG_TEST_FIXED_ARENA: the arena neither grows nor asks for a rebuild, so a full arena is reachable — new long keys are
     refused, every request of them, in the same launch, on the resend and until a rebuild has made room; nothing else notices
  4  the probe bound: 4 096 keys under one tag and one home fill max_probe; further keys of that home are refused and take no slot
  5  a cluster that spills over the table's end into slots 0 .., and keys with homes 0 .. 3 that probe past the spill"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)                          # (run as a script: the package is importable from the repository tree)

import streams
import support
from support import HostBatch, Oracle

WEAK_HASH, FIXED_ARENA = 1, 512
E_TABLE_FULL = 6
# (name, flags, largest batch): "every pipeline" = the two-launch one, the radix sequence, the careful round, the owner-partitioned one,
# the two-launch one with the owner-partitioned switched off, and the one-launch path of batches of <= 256 requests
PIPELINES = (("two_launch", 0, 1024), ("radix", 2, 1024), ("careful", 4, 1024), ("part", 64, 1024), ("no_part", 128, 1024), ("small", 0, 200))
GEOM = dict(table_slots=4096, max_key_bytes=512, max_batch=1024)
LONG, ARENA, TAG_LIMIT, FIT = 408, 1 << 20, 3584, 2570
HOUR = 3_600_000
FIELDS = ("status", "limit", "remaining", "reset_time", "err")
# what the CPU build runs smaller (the fiber emulation runs a tile in about a second): the keys per batch while case 4's chain is filled
# — n new keys under ONE hash take about n rounds of up to n requests, each walking the chain — nothing else
CPU_CHAIN_BATCH = 32


def long_key(tag, length=LONG):
    return tag.ljust(length, b"x")


def chunks(seq, m):
    return [seq[i:i + m] for i in range(0, len(seq), m)]


def both(e, o, keys, now, what, duration=HOUR, limit=9, hits=1):
    """one batch through the engine and the oracle, equal element-wise -> the engine's result"""
    b = HostBatch(keys, hits, limit, duration, now)
    got = e.eval(b)
    support.assert_results_equal(got, o.eval(b), what)
    return got


def assert_subset_equal(got, keep, want, what):
    """got at the positions `keep` equals want (a batch of len(keep) requests) element-wise"""
    for name in FIELDS:
        g, w = getattr(got, name)[keep], getattr(want, name)[:len(keep)]
        if not np.array_equal(g, w):
            i = int(np.nonzero(g != w)[0][0])
            raise AssertionError(f"{what}: {name} differs at {int((g != w).sum())} of {len(keep)} positions; first at request {int(keep[i])}: got {int(g[i])} want {int(w[i])}")


def assert_refused(got, idx, what):
    """every request at idx: GUBER_ITEM_E_TABLE_FULL and nothing else"""
    err = got.err[idx]
    assert (err == E_TABLE_FULL).all(), f"{what}: {int((err != E_TABLE_FULL).sum())} of {len(idx)} requests of refused keys were not refused; first at {int(idx[np.nonzero(err != E_TABLE_FULL)[0][0]])}: err {int(err[err != E_TABLE_FULL][0])}"
    for name in ("status", "limit", "remaining", "reset_time"):
        assert (getattr(got, name)[idx] == 0).all(), (what, name)


def with_refusals(e, o, keys, refused, now, what, **kw):
    """`keys` through the engine, the same without the keys of `refused` (a set) through the oracle, in the same order: the others equal the
    oracle, every request of a refused key is refused -> the engine's result"""
    is_ref = np.array([k in refused for k in keys])
    keep, idx = np.nonzero(~is_ref)[0], np.nonzero(is_ref)[0]
    got = e.eval(HostBatch(keys, 1, 9, HOUR, now, **kw))
    want = o.eval(HostBatch([keys[i] for i in keep], 1, 9, HOUR, now, **kw))
    assert (got.err[keep] == 0).all(), f"{what}: {int((got.err[keep] != 0).sum())} requests of resident or short keys have an error; first err {int(got.err[keep][got.err[keep] != 0][0])}"
    assert_subset_equal(got, keep, want, what)
    assert_refused(got, idx, what)
    return got


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
def case_churn_over_a_small_cache(factory, pipeline):
    name, flags, cap = pipeline
    small = cap <= 256
    steps, fresh, nres = (24, 200, 25) if small else (12, 400, 50)
    e, o = factory(cache_size=1000, flags=flags, **GEOM), Oracle(cache_size=1000)
    residents = [long_key(b"c1_res_%03d_" % i) for i in range(nres)]
    now = streams.NOW0
    top = 0
    for step in range(steps):
        keys = [long_key(b"c1_%02d_%03d_" % (step, i)) for i in range(fresh)] + residents
        got = both(e, o, keys, now, f"churn[{name}] step {step}")
        assert (got.err[:len(keys)] == 0).all(), (name, step)
        assert e.size() == o.size(), (name, step, e.size(), o.size())
        top = max(top, e.stats()["tags_used"])
        now += 1000
    st = e.stats()
    assert st["compactions"] >= 1, st
    assert top <= TAG_LIMIT - 450, f"{name}: {top} tags: the tag limit, not the arena, may have asked for the rebuild"
    e.close(); o.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------
LENGTHS = (63, 64, 65, 71, 72, 73, 200, 408, 512)     # around the inline limit (62) and the 8-byte padding of arena allocations
WEIGHTS = (.02, .02, .02, .02, .02, .02, .08, .3, .5)  # mostly the long ones: the 3 000 keys take more than the arena's first 1 MiB


def cache_worth_of_keys(n=3000, seed=2):
    """n keys of LENGTHS; one in four has a twin that differs only in its last byte and a partner that is one byte longer (for a key of
    512 bytes — the longest the engine takes — the partner is the one byte shorter)"""
    rng = np.random.default_rng(seed)
    keys, i = [], 0
    while len(keys) < n:
        L = int(rng.choice(LENGTHS, p=WEIGHTS))
        k = (b"c2_%05d_" % i) + bytes(rng.integers(97, 123, L - 9, dtype=np.uint8))
        keys.append(k)
        if i % 4 == 0:
            keys.append(k[:-1] + bytes([k[-1] ^ 1]))
            keys.append(k + b"q" if L < 512 else k[:-1])
        i += 1
    keys = keys[:n]
    assert len(set(keys)) == n
    return keys


def case_a_caches_worth_of_long_keys(factory, pipeline):
    name, flags, cap = pipeline
    per = min(cap, 400)
    e, o = factory(cache_size=3000, flags=flags, **GEOM), Oracle(cache_size=3000)
    keys = cache_worth_of_keys()
    assert sum((len(k) + 7) & ~7 for k in keys) > ARENA + 100_000                    # (all live at once: only a larger arena holds them)
    rng = np.random.default_rng(22)
    now = streams.NOW0

    def round_of(ks, what):
        nonlocal now
        for j, part in enumerate(chunks(ks, per)):
            got = both(e, o, part, now, f"{what}[{name}] batch {j}")
            assert (got.err[:len(part)] == 0).all(), (name, what, j)
            assert e.size() == o.size(), (name, what, j, e.size(), o.size())
            now += 1000

    round_of(keys, "insert")
    round_of([keys[i] for i in rng.permutation(len(keys))], "again")                 # (the keys survived the rebuilds into a larger arena)
    round_of([long_key(b"c2_new_%03d_" % i, int(LENGTHS[i % len(LENGTHS)])) for i in range(400)], "new keys: evictions start")
    round_of([keys[i] for i in rng.permutation(len(keys))], "once more")
    assert e.stats()["compactions"] >= 1
    e.close(); o.close()


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
def batch_x():
    """-> (keys, residents in it, refused): 100 resident long keys, 50 new short keys of at most 62 bytes, 40 new long keys at two positions
    each that are not adjacent, interleaved"""
    residents = [long_key(b"c3_%04d_" % i) for i in range(0, 2500, 25)]
    short = [(b"c3_short_%02d_" % i).ljust(12 + i, b"s") for i in range(50)]          # 12 .. 61 bytes
    short[49] = short[49].ljust(62, b"s")
    new = [long_key(b"c3_new_%02d_" % i) for i in range(40)]
    keys = []
    for half, order in ((0, list(range(40))), (1, [(i + 20) % 40 for i in range(40)])):
        r, s = residents[50 * half:50 * half + 50], short[25 * half:25 * half + 25]
        for i in range(50):
            keys.append(r[i])
            if i < 40:
                keys.append(new[order[i]])
            if i % 2 == 0:
                keys.append(s[i // 2])
    assert len(keys) == 230 and all(len(k) <= 62 for k in short)
    for k in new:
        at = [i for i, x in enumerate(keys) if x == k]
        assert len(at) == 2 and at[1] - at[0] > 1
    return keys, residents, set(new)


def case_the_arena_refuses(factory, pipeline, store_channel=False):
    """-> what the engine counted over batch X (retries, cache hits, misses, over the limit): the same on every pipeline"""
    name, flags, cap = pipeline
    e, o = factory(cache_size=3000, flags=flags | FIXED_ARENA, **GEOM), Oracle(cache_size=3000)
    now = streams.NOW0
    fill = [long_key(b"c3_%04d_" % i) for i in range(FIT)]
    for j, part in enumerate(chunks(fill, min(cap, 400))):
        got = both(e, o, part, now, f"fill[{name}] batch {j}")
        assert (got.err[:len(part)] == 0).all(), f"fill[{name}] batch {j}: {int((got.err[:len(part)] != 0).sum())} of the {FIT} keys that fill the arena were refused"
    assert e.size() == o.size() == FIT
    keys, residents, refused = batch_x()
    before = e.stats()
    now += 1000
    with_refusals(e, o, keys, refused, now, f"X[{name}]")
    after = e.stats()
    assert e.size() == o.size(), (name, e.size(), o.size())
    figures = {k: after[k] - before[k] for k in ("retries", "cache_hits", "cache_misses", "over_limit_count")}
    # X again: the same 80 requests are refused, the others go on, the size stays
    size = e.size()
    if store_channel:                                # (the same batch through guber_eval_batch_store: a refused request raises no event)
        b = HostBatch(keys, 1, 9, HOUR, now + 1)
        got, ev, _items = e.eval_store_raw(b)
        is_ref = np.array([k in refused for k in keys])
        keep, idx = np.nonzero(~is_ref)[0], np.nonzero(is_ref)[0]
        assert_subset_equal(got, keep, o.eval(HostBatch([keys[i] for i in keep], 1, 9, HOUR, now + 1)), f"X again, with the Store side channel[{name}]")
        assert_refused(got, idx, f"X again, with the Store side channel[{name}]")
        assert (ev[idx] == 0).all(), f"{int((ev[idx] != 0).sum())} refused requests raised OnChange / Remove"
        assert (ev[keep] & 1).any()                  # (the channel did report the served requests' changes)
    else:
        with_refusals(e, o, keys, refused, now + 1, f"X again[{name}]")
    assert e.size() == size == o.size(), (name, e.size(), size, o.size())
    # room: 100 residents leave, the table is rebuilt; the refused keys are new keys now
    for k in residents:
        e.remove_item(k); o.remove_item(k)
    assert e.size() == o.size()
    e.compact(now + 1)
    assert e.size() == o.size()
    twice = sorted(refused) + sorted(refused)[::-1]
    got = both(e, o, twice, now + 2, f"the refused keys after the rebuild[{name}]")
    assert (got.err[:len(twice)] == 0).all()
    assert e.size() == o.size()
    got = both(e, o, twice, now + 3, f"the refused keys once more[{name}]")
    assert (got.err[:len(twice)] == 0).all()
    assert e.size() == o.size()
    e.close(); o.close()
    return figures


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
_CHAIN = None


def xxh(key):
    return support.oracle_lib().oracle_xxhash64(key, len(key), 0)


def chain_keys():
    """keys by their home under GUBER_FLAG_TEST_WEAK_HASH (the hash's bits 7 .. 12 are kept: 64 homes, one tag each), searched once:
    'group' 4 096 keys of home 5 — 12 .. 16 bytes, and 8 pairs of 61, 62, 63 and 64 bytes that differ only in their last byte (key_equal on the
    last inline word, and the arena under a shared tag) —, 'more' 64 further keys of home 5, 'home40' 64 keys, 'zero' 4 keys whose masked hash is 0"""
    global _CHAIN
    if _CHAIN is not None:
        return _CHAIN
    want = {5 << 7: 4096 - 16 + 64, 40 << 7: 64, 0: 4}
    found = {m: [] for m in want}
    i = 0
    while any(len(found[m]) < want[m] for m in want):
        k = (b"c4_%07d_" % i).ljust(12 + i % 5, b"k")
        m = xxh(k) & 0x1f80
        if m in want and len(found[m]) < want[m]:
            found[m].append(k)
        i += 1
    pairs, j = [], 0
    for L in (61, 62, 63, 64):
        got = 0
        while got < 2:
            a = (b"c4_pair_%02d_%07d_" % (L, j)).ljust(L, b"p")
            b = a[:-1] + b"q"
            j += 1
            if xxh(a) & 0x1f80 == 5 << 7 and xxh(b) & 0x1f80 == 5 << 7:
                pairs += [a, b]; got += 1
    home5 = found[5 << 7]
    group = home5[:2000] + pairs[:8] + home5[2000:4080 - 50] + pairs[8:] + home5[4080 - 50:4080]     # (the last 50 inserted are short keys)
    assert len(group) == 4096 and len(set(group)) == 4096
    _CHAIN = dict(group=group, more=home5[4080:], home40=found[40 << 7], zero=found[0], pairs=pairs)
    return _CHAIN


def case_the_probe_bound(factory, pipeline, chain_batch=0):
    name, flags, cap = pipeline
    K = chain_keys()
    e = factory(cache_size=6000, table_slots=8192, max_key_bytes=512, max_batch=1024, flags=flags | WEAK_HASH)
    o = Oracle(cache_size=6000)
    now = streams.NOW0
    group = K["group"]
    for j, part in enumerate(chunks(group, chain_batch or (256 if cap <= 256 else 512))):
        got = both(e, o, part, now, f"chain[{name}] batch {j}")
        assert (got.err[:len(part)] == 0).all(), f"chain[{name}] batch {j}: errors {sorted(set(got.err[:len(part)].tolist()))}"
    assert e.size() == o.size() == 4096
    st0 = e.stats()
    assert st0["tags_used"] == 4096, st0
    # the chain holds slots 5 .. 4 100 = max_probe entries: further keys of home 5 find no entry — refused, and no slot is taken
    more = K["more"]
    residents = group[:75] + K["pairs"] + group[3000:3059] + group[-50:]               # (the last 50 inserted sit at the chain's far end)
    assert len(residents) == 200 and len(set(residents)) == 200
    halves = ([], [])
    for i in range(200):
        halves[i // 100].append(residents[i])
        if i % 100 < 64:
            halves[i // 100].append(more[(i % 100 + 32 * (i // 100)) % 64])
    now += 1000
    for j, keys in enumerate(halves if cap <= 256 else (halves[0] + halves[1],)):      # (each new key twice; the one-launch path: once per batch)
        with_refusals(e, o, keys, set(more), now, f"past the probe bound[{name}] {j}")
    st = e.stats()
    assert e.size() == o.size() == 4096 and st["tags_used"] == 4096, (e.size(), st)
    # recovery: 64 residents leave, the table is rebuilt — the chain is 4 032 entries long —, the refused keys are new keys: the chain
    # holds slots 5 .. 4 100 again
    for k in group[1000:1064]:
        e.remove_item(k); o.remove_item(k)
    e.compact(now)
    assert e.size() == o.size() == 4032
    twice = more + more[::-1]
    for t in (1, 2):
        got = both(e, o, twice, now + t, f"the refused keys after the rebuild[{name}] {t}")
        assert (got.err[:len(twice)] == 0).all()
        assert e.size() == o.size() == 4096
    # other homes, whose windows reach free slots.  Masked hash 0 (probe_packed's tag = h ? h : 1): home 0, window 0 .. 4 095, free 0 .. 4.
    # Home 40: window 40 .. 4 135 of which 40 .. 4 100 are the chain's, so 4 101 .. 4 135 = 35 keys are served like the oracle and the
    # window is exhausted for the other 29 of the 64: refused, no slot taken.  (Behind the recovery, not before it: with these entries
    # in the cluster the rebuilt chain would end 35 slots further on, and the recovered keys would pass home 5's bound.)
    now += 1000
    got = both(e, o, K["zero"], now, f"masked hash 0[{name}]")
    assert (got.err[:len(K["zero"])] == 0).all()
    got = both(e, o, K["home40"][:35], now, f"home 40[{name}]")
    assert (got.err[:35] == 0).all()
    assert e.size() == o.size() == 4096 + 4 + 35
    tags = e.stats()["tags_used"]
    rest = K["home40"][35:]
    with_refusals(e, o, rest + group[-20:] + rest[::-1], set(rest), now + 1, f"home 40, past its window[{name}]")
    assert e.size() == o.size() and e.stats()["tags_used"] == tags
    e.close(); o.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
_WRAP = None


def wrap_keys():
    """-> (40 keys whose home (hash >> 7) & 1023 is >= 1 020, 40 keys with homes 0 .. 3), lengths 8, 16, 17, 40 and 100 mixed"""
    global _WRAP
    if _WRAP is None:
        hi, lo, i = [], [], 0
        while len(hi) < 40 or len(lo) < 40:
            k = (b"w%06d" % i).ljust((8, 16, 17, 40, 100)[i % 5], b"w")
            home = (xxh(k) >> 7) & 1023
            if home >= 1020 and len(hi) < 40:
                hi.append(k)
            elif home <= 3 and len(lo) < 40:
                lo.append(k)
            i += 1
        assert {len(k) for k in hi} == {len(k) for k in lo} == {8, 16, 17, 40, 100}
        _WRAP = (hi, lo)
    return _WRAP


def case_a_chain_across_the_tables_end(factory, pipeline, move=False):
    name, flags, cap = pipeline
    cfg = dict(cache_size=512, table_slots=1024, max_key_bytes=512, max_batch=1024)
    e, o = factory(flags=flags, **cfg), Oracle(cache_size=512)
    hi, lo = wrap_keys()
    keys = hi + lo
    dur = [20 if i % 2 else HOUR for i in range(80)]                                # (every second key is short-lived)
    now = streams.NOW0

    def hit(what, t, ks=keys, d=dur):
        got = both(e, o, ks, t, f"{what}[{name}]", duration=d)
        assert (got.err[:len(ks)] == 0).all(), (name, what)
        assert e.size() == o.size(), (name, what, e.size(), o.size())

    both(e, o, hi, now, f"insert the cluster[{name}]", duration=dur[:40])            # (the cluster first: it spills into slots 0 .. 35)
    both(e, o, lo, now, f"insert homes 0 .. 3[{name}]", duration=dur[40:])
    assert e.size() == o.size() == 80
    hit("hit again", now + 1)
    hit("half of them expired", now + 1001)
    e.compact(now + 1001)
    assert e.size() == o.size()
    hit("after the rebuild", now + 1002)
    # cache operations on three wrapped keys
    t = now + 1003
    for k in (hi[0], hi[17], hi[39]):
        ge, go = e.get_item(k, t), o.get_item(k, t)
        assert ge == go and ge is not None, (k, ge, go)
        e.remove_item(k); o.remove_item(k)
        assert e.get_item(k, t) is None and o.get_item(k, t) is None
        assert e.size() == o.size()
        it = dict(limit=9, duration=HOUR, remaining=4, stamp=t, expire_at=t + HOUR)
        assert e.add_item(support.make_item(k, 0, **it), t) == o.add_item(support.make_item(k, 0, **it), t) == False
        ge, go = e.get_item(k, t), o.get_item(k, t)
        assert ge == go and ge is not None and ge["remaining"] == 4, (k, ge, go)
        assert e.size() == o.size()
    hit("after the cache operations", now + 1004)
    if move:                                         # the wrapped keys move into a second table by their hashes, and back
        b = factory(flags=flags, stream=e.stream_handle(), **cfg)
        hashes = [xxh(k) for k in hi]
        was = {k: e.get_item(k, t + 2) for k in hi}
        assert e.move_items_to(b, hashes) == 40
        assert e.size() == 40 and b.size() == 40 and e.size() + b.size() == o.size()
        for k in hi:
            assert e.get_item(k, t + 2) is None and b.get_item(k, t + 2) == was[k] == o.get_item(k, t + 2), k
        assert b.move_items_to(e, hashes) == 40
        assert e.size() == 80 == o.size() and b.size() == 0
        for k in hi:
            assert e.get_item(k, t + 2) == was[k], k
        b.close()
        hit("after the move and back", now + 1006)
    e.close(); o.close()


def run_all(factory, cpu=False):
    figures = {}
    for p in PIPELINES:
        case_churn_over_a_small_cache(factory, p)
        case_a_caches_worth_of_long_keys(factory, p)
        figures[p[0]] = case_the_arena_refuses(factory, p, store_channel=p[0] == "two_launch")
        case_the_probe_bound(factory, p, chain_batch=CPU_CHAIN_BATCH if cpu else 0)
        case_a_chain_across_the_tables_end(factory, p, move=p[0] == "two_launch")
        print(f"{p[0]}: ok", flush=True)
    assert len({tuple(sorted(f.items())) for f in figures.values()}) == 1, f"batch X was counted differently by the pipelines: {figures}"


if __name__ == "__main__":
    import gubernator_amd as ga
    run_all(lambda **kw: ga.Engine(**kw), cpu="enginesim" in ga.LIB_PATH)
    print("TABLE FULL CASES OK")
