"""The engine's counters where production is after seconds to days (GUBER_FLAG_TEST_LATE_COUNTERS, gubernator_amd/csrc/guber_test_flags.h):
the 53-bit recency stamp (Rec::pad = bits 0..31, Rec::meta >> 11 = bits 32..52) crossing 2^52 — pad goes from 0xffffffff to 0, the twenty
lower high bits flip and meta bit 31 is set —, the directory's 31-bit epoch, the claim table's 16-bit epoch and the snapshot ring's 32-bit
sequence at their wraps.  The driver of tests/test_gpu_late_counters.py (the product library on a GPU) and tests/test_late_counters_cpu.py
(the kernel source on the CPU, tests/hostsim/devsim.cpp); numpy only.

Every comparison is exact equality with the bounded-LRU oracle.  Every run POSITIONS its crossing by arithmetic of its own — Mirror counts
what the engine hands out: a batch of n requests takes n stamps (whatever pieces it is evaluated in), Add one per item, GetItem and Remove
one, a batch one epoch, a two-launch batch one claim epoch — and asserts that the crossing lies strictly inside the run.

A backend is anything with  eval(HostBatch) -> HostResult,  totals() -> (over_limit, hits, misses, unexpired_evictions, size) so far,
and for the cache operations  add_items([GuberItem], now_ms) -> [existed],  get_item(key, now_ms) -> dict | None."""
import os
import re

import numpy as np

import streams
import support
from support import HostBatch

FLAG = 256                                   # gubernator_amd.FLAG_TEST_LATE_COUNTERS
SEQ_NEXT = (1 << 52) - 4096                  # GUBER_TEST_LATE_SEQ_NEXT
EPOCH = 0x7fffffff - 12                      # GUBER_TEST_LATE_EPOCH
EPOCH16 = 0xffff - 12                        # GUBER_TEST_LATE_EPOCH16
RB_SEQ = 0xffffffff - 8                      # GUBER_TEST_LATE_RB_SEQ
CROSSING = 1 << 52                           # the first stamp with pad == 0 and meta bit 31 set
INVALID_ALGORITHM = 7                        # workers.go:317-321 rejects it before the cache is looked at


def header_values():
    """the flag and the four start values as gubernator_amd/csrc/guber_test_flags.h spells them (C integer expressions of literals)"""
    text = open(os.path.join(support.ROOT, "gubernator_amd", "csrc", "guber_test_flags.h")).read()
    out = {}
    for name in ("GUBER_FLAG_TEST_LATE_COUNTERS", "GUBER_TEST_LATE_SEQ_NEXT", "GUBER_TEST_LATE_EPOCH", "GUBER_TEST_LATE_EPOCH16", "GUBER_TEST_LATE_RB_SEQ"):
        expr = re.search(r"^#define %s\s+(.+?)\s*(?:/\*|$)" % name, text, re.M).group(1)
        assert re.fullmatch(r"[0-9a-fxulUL()<\-+ ]+", expr), expr
        out[name] = eval(re.sub(r"(?<=[0-9a-f])(?:ull|u)\b", "", expr, flags=re.I))
    return out


class Mirror:
    """what an engine created with FLAG has handed out, counted by the test"""

    def __init__(self, seq=SEQ_NEXT):
        self.seq, self.epoch, self.epoch16, self.rb_seq = seq, EPOCH, EPOCH16, RB_SEQ

    def stamps(self, n):
        """n stamps -> the first of them"""
        first = self.seq
        self.seq += n
        return first

    def batch(self, n):
        """one batch of n requests through a batch pipeline -> (first stamp, directory epoch wrapped, claim epoch wrapped) — batch_prelude:
        ++epoch >= 0x7fffffff clears the claims and restarts at 1; plan_fast: ++epoch16 > 0xffff wipes the table and restarts at 1"""
        first = self.stamps(n)
        self.epoch += 1
        wrapped = self.epoch >= 0x7fffffff
        if wrapped:
            self.epoch = 1
        self.epoch16 += 1
        wrapped16 = self.epoch16 > 0xffff
        if wrapped16:
            self.epoch16 = 1
        return first, wrapped, wrapped16

    def snapshot(self):
        """one counter snapshot -> its sequence number wrapped (0 is skipped: ++rb_seq ? rb_seq : ++rb_seq)"""
        self.rb_seq = (self.rb_seq + 1) & 0xffffffff
        if self.rb_seq == 0:
            self.rb_seq = 1
            return True
        return False


def oracle_totals(orc):
    return tuple(int(x) for x in orc.counters()) + (int(orc.size()),)


def advance(be, mirror, stamps, now_ms, chunk=200, epochs=False, exact=True):
    """`stamps` recency stamps handed out and nothing else: batches of requests with an algorithm the reference rejects before it looks at
    the cache (every one an error answer, no bucket reached) — size and counters must not move.  epochs: every batch also takes one
    directory epoch and one claim epoch (true of batches of 257 requests and more, or an engine without the one-launch path, whose
    cache does not bind: the caller's business); otherwise the mirror's epochs are left alone and mean nothing afterwards.  -> batches used"""
    assert stamps >= 0
    before, used = be.totals(), 0
    launched = be.batches() if hasattr(be, "batches") else None
    while stamps:
        n = min(stamps, chunk)
        b = HostBatch([b"late_advance_%d" % (i & 3) for i in range(n)], 1, 10, 60_000, now_ms, algorithm=np.full(n, INVALID_ALGORITHM, np.uint8))
        res = be.eval(b)
        assert (res.err[:n] != 0).all(), "an invalid-algorithm request was answered"
        if epochs:
            mirror.batch(n)
        else:
            mirror.stamps(n)
        stamps -= n
        used += 1
    assert be.totals() == before, (be.totals(), before)
    if launched is not None and exact:                   # (one prelude per batch: no piece, retry round or fall-back took stamps of its own)
        assert be.batches() - launched == used, (be.batches() - launched, used)
    return used


WORKLOADS = ("cyclic scan", "random walk", "zipf", "expiring")


def bounded_batches(name, nkeys, bsz, pins, steps, seed=3):
    """the workloads of test_evicted_keys_that_return_meet_the_reference_list: `bsz` requests over `nkeys` keys + `pins` keys touched by every
    batch, both algorithms; expiring = short durations with the clock moving"""
    rng = np.random.default_rng(seed)
    z = streams.ZipfSampler(nkeys, seed=seed + 6)
    now, pos = streams.NOW0, 0
    for _ in range(steps):
        if name == "cyclic scan":
            ids = (pos + np.arange(bsz)) % nkeys
            pos += bsz
        elif name == "zipf":
            ids = z.draw(bsz)
        else:
            ids = rng.integers(0, nkeys, bsz)
        keys = [f"ret_{int(i)}" for i in ids] + [f"pin_{i}" for i in range(pins)]
        yield HostBatch(keys, 1, 1000, 1500 if name == "expiring" else 3_600_000, now,
                        algorithm=np.concatenate([(ids & 1).astype(np.uint8), np.zeros(pins, np.uint8)]))
        now += 1000


def resident_keys(orc):
    return {d["key"] for d in orc.each()}


def evicted_unasked(before, after, b):
    """did the reference evict in batch b?  An item that was in its list before the batch, that no request of the batch names and that is
    gone afterwards can only have left from the back of the list (lrucache.go:98-100,138-149): before / after = resident_keys around b"""
    asked = {bytes(b.key_bytes[b.key_off[i]:b.key_off[i + 1]]) for i in range(b.n)}
    return any(k not in asked and k not in after for k in before)


def run_bounded(be, orc, mirror, cs, batches, what, per_batch_counters=True, witness="list"):
    """the batches against the oracle: answers, the batch's aggregates (where the backend reports them), the totals and the size after every
    batch.  -> [(first stamp, n, the reference evicted in this batch, the backend's tail-list rebuilds so far)] per batch — witness "list": evicted_unasked, from the reference's list
    around the batch; "unexpired": the batch's count of unexpired evictions is not 0 (cheaper; complete where no item expires during the run)"""
    trace, after = [], resident_keys(orc) if witness == "list" else None
    for step, b in enumerate(batches):
        before = after
        first = mirror.batch(b.n)[0]
        got, want = be.eval(b), orc.eval(b)
        support.assert_results_equal(got, want, f"{what} step {step} (stamps {first - CROSSING:+d} .. {first + b.n - 1 - CROSSING:+d} around 2^52)")
        if per_batch_counters:
            assert got.counters() == want.counters(), (what, step, got.counters(), want.counters())
        assert be.totals() == oracle_totals(orc), (what, step, be.totals(), oracle_totals(orc))
        assert orc.size() <= cs
        if witness == "list":
            after = resident_keys(orc)
        trace.append((first, b.n, evicted_unasked(before, after, b) if witness == "list" else want.counters()[3] > 0,
                      be.rebuilds() if hasattr(be, "rebuilds") else None))
    return trace


def crossing_step(trace):
    """the batch that hands out stamp 2^52 together with older ones (None: the crossing is not strictly inside a batch of the run)"""
    for i, t in enumerate(trace):
        if t[0] < CROSSING < t[0] + t[1]:
            return i
    return None


def assert_crossing_inside(trace, cs, each_side=5, what=""):
    """the positioning assertion: stamp 2^52 is handed out inside batch k, and in at least `each_side` batches before k and as many after it
    the cache binds — the reference evicts in the middle of the batch (evicted_unasked)"""
    k = crossing_step(trace)
    assert k is not None, (what, [(t[0] - CROSSING, t[1]) for t in trace][:4])
    binds = [t[2] for t in trace]
    before, after = sum(binds[:k]), sum(binds[k + 1:])
    assert before >= each_side and after >= each_side, (what, k, before, after)
    return k, before, after


def assert_rebuilds_on_both_sides(trace, k):
    """the tail list was built from stamps below 2^52 only (before batch k) and again with stamps from both sides in one sort (after it)"""
    assert trace[k - 1][3] >= 1 and trace[-1][3] > trace[k][3], (trace[k - 1][3], trace[k][3], trace[-1][3])


def stamps_to_put_crossing_in(mirror, step, n, offset):
    """how far to advance so that stamp 2^52 is request `offset` of batch `step` of a run of n-request batches"""
    assert 0 < offset < n
    adv = CROSSING - (step * n + offset) - mirror.seq
    assert adv >= 0, "the run starts behind the place it wants the crossing at"
    return adv


def duplicate_batches(steps, n, nkeys, seed, prefix=b"wrap"):
    """`steps` batches of n requests over nkeys keys (duplicates inside every batch), both algorithms, limits that are reached"""
    rng = np.random.default_rng(seed)
    keys = [prefix + b"_%d" % i for i in range(nkeys)]
    for s in range(steps):
        ids = rng.integers(0, nkeys, n)
        yield HostBatch([keys[i] for i in ids], rng.integers(0, 3, n), 400, 3_600_000, streams.NOW0 + s * 50, algorithm=(ids & 1).astype(np.uint8))


def recency_items(names, now_ms):
    return [support.make_item(k, support.TOKEN, limit=10, duration=3_600_000, remaining=9 - (i % 7), stamp=now_ms, expire_at=now_ms + 3_600_000)
            for i, k in enumerate(names)]


def cache_sequence(be, orc, mirror, one_call):
    """LRUCache.Add of 11 items into a cache of 10 (one call of the ABI, or item by item), GetItem on the oldest survivor, Add of one more —
    stamp 2^52 is handed out in the middle of the first eleven.  The victims must be the reference's: item 0 (the oldest stamp, below 2^52),
    then item 2 (item 1 was moved to the front by GetItem, with a stamp above 2^52).  mirror.seq must be 2^52 - 6 on entry."""
    now = streams.NOW0
    assert mirror.seq == CROSSING - 6
    names = [f"seq_{i}" for i in range(12)]
    items = recency_items(names, now)
    for it in items[:11]:
        orc.add_item(it, now)
    if one_call:
        assert be.add_items(items[:11], now) == [False] * 11
        mirror.stamps(11)
    else:
        for it in items[:11]:
            assert be.add_items([it], now) == [False]
            mirror.stamps(1)
    assert mirror.seq - 11 < CROSSING < mirror.seq                          # (the crossing is inside the eleven)
    assert be.totals() == oracle_totals(orc) and orc.size() == 10 and orc.counters()[3] == 1
    a, g = orc.get_item(names[1], now), be.get_item(names[1], now)          # the oldest item left: to the front (lrucache.go:123)
    mirror.stamps(1)
    assert a is not None and g is not None and a["remaining"] == g["remaining"], (a, g)
    orc.add_item(items[11], now)
    assert be.add_items([items[11]], now) == [False]
    mirror.stamps(1)
    assert be.totals() == oracle_totals(orc) and orc.counters()[3] == 2
    left = []
    for k in names:                                                         # (GetItem moves what it finds: the same in both, in the same order)
        a, g = orc.get_item(k, now), be.get_item(k, now)
        mirror.stamps(1)
        assert (a is None) == (g is None), (k, a, g)
        if a is not None:
            assert a["remaining"] == g["remaining"] and a["algorithm"] == g["algorithm"] and a["status"] == g["status"], (k, a, g)
            left.append(k)
    assert left == [names[1]] + names[3:], left
    assert be.totals() == oracle_totals(orc)


class CountingCache:
    """a cache-operations backend for scenarios.run_cache_vectors that counts the stamps its operations take (Add, GetItem and Remove one
    each) and, when the case is over, asserts that stamp 2^52 was handed out inside it"""

    def __init__(self, be, mirror, on_close=None):
        self.be, self.mirror, self.on_close, self.first = be, mirror, on_close, mirror.seq

    def add_item(self, item, now_ms=0):
        self.mirror.stamps(1)
        return self.be.add_items([item], now_ms)[0]

    def get_item(self, key, now_ms):
        self.mirror.stamps(1)
        return self.be.get_item(key, now_ms)

    def remove_item(self, key):
        self.mirror.stamps(1)
        self.be.remove_item(key)

    def size(self):
        return self.be.totals()[4]

    def counters(self):
        return self.be.totals()[:4]

    def close(self):
        assert self.first < CROSSING <= self.mirror.seq - 1, (self.first - CROSSING, self.mirror.seq - CROSSING)   # (stamp 2^52 and older ones)
        if self.on_close:
            self.on_close()
