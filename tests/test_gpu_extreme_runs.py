"""tests/extreme_runs.py on the device, through every batch pipeline: Go's integer and float rules (the __umul64hi arm of mul_lt, the
device's fp64 division and conversions) in runs at ranks past a tile and in walked segments, with the bucket carried as SegRec, GRec and
the 32-byte GRecS; items with CacheItem.InvalidAt (W.sinv[] in k_front -> k_eval2 and k_own -> k_eval3); created_at ranges on the
thresholds of k_part's packed range.  Every batch, its counters, the size after every step and GetItem field by field equal the oracle's;
per-kernel timing is on and every batch is checked for the kernels that ran, so that no case passes on another pipeline than the one
its flags name.  The CPU twin (the kernel source on the host) is in tests/test_kernels_devsim.py."""
import functools

import pytest

import extreme_runs
import gubernator_amd as ga
import support
from support import Oracle

pytestmark = pytest.mark.gpu

# the engine flags of test_adversarial_streams (tests/test_gpu_parity.py): default, two-launch for small batches too, never
# owner-partitioned, owner-partitioned, radix, careful
FLAGS = [0, 32, 128, 64, 2, 4]
PAIR, PART, RADIX = {"k_front", "k_eval2"}, {"k_part", "k_own", "k_eval3"}, {"k_resolve", "k_scatter(first)", "k_heads", "k_eval"}
# a batch of one workgroup takes the one-launch path unless the flags say otherwise (guber_engine_create: no_small) — FLAG_NO_PART
# leaves it alone; k_small has no entry in the per-kernel timing: its batches are counted by guber_stats_t.small_batches, and one it
# declined (a group whose requests differ) is re-run by the two-launch pipeline, which the timing shows
SMALL_PATH = (0, 128)


class ScriptEngine:
    """extreme_runs.run_script's backend over the product library; records (n, answered by k_small, kernels timed) for every batch"""

    def __init__(self, flags):
        self.flags = flags
        self.e = ga.Engine(cache_size=1 << 16, max_batch=4096, flags=flags)
        self.e.profile(True)
        self.ran = []

    def add(self, items):
        self.e.add_items(items)

    def eval(self, b):
        small0 = self.e.stats()["small_batches"]
        res = self.e.eval(b)
        kernels = {k for k, (launches, _) in self.e.profile_read().items() if launches}
        self.ran.append((b.n, self.e.stats()["small_batches"] - small0, kernels))
        return res, res.counters()

    def get(self, key, now_ms):
        return self.e.get_item(key, now_ms)

    def compact(self, now_ms):
        self.e.compact(now_ms)

    def each(self):
        return self.e.each()

    def size(self):
        return self.e.size()

    def close(self):
        self.e.close()


def assert_kernels(be, by_k_small):
    """which kernels answered: k_small the batches of one workgroup under flags 0 (and 128) — "all" of them where every group is a run of
    identical requests, "some", or "none" where every such batch holds a segment to walk —, under the other flags none; everything
    else the pipeline the flags name"""
    flags = be.flags
    pipeline = PART if flags == 64 else RADIX if flags == 2 else PAIR
    by_small = 0
    assert be.ran
    for n, small, kernels in be.ran:
        what = (flags, n, small, sorted(kernels))
        if n <= 256 and flags in SMALL_PATH:
            assert small == 1, what
            assert kernels == set() or kernels == PAIR, what              # answered by k_small, or declined and re-run
            by_small += not kernels
            assert by_k_small == "some" or (by_k_small == "all") == (not kernels), what
        else:
            assert small == 0, what
            assert kernels >= pipeline and not kernels & ((PAIR | PART | RADIX) - pipeline), what
    assert (by_small > 0) == (flags in SMALL_PATH and by_k_small != "none"), (flags, by_small)


def run_family(flags, cases, by_k_small="some"):
    be, orc = ScriptEngine(flags), Oracle(cache_size=1 << 16)
    try:
        for label, steps in cases:
            extreme_runs.run_script(f"flags {flags}: {label}", steps, be, orc, support.make_item, support.assert_results_equal)
        assert_kernels(be, by_k_small)
    finally:
        be.close()


@functools.lru_cache(maxsize=None)
def cases_of(family):
    return {"uniform": extreme_runs.extreme_uniform_cases, "walk": extreme_runs.extreme_walk_cases, "invalid_at": extreme_runs.invalid_at_cases,
            "created_at": lambda: extreme_runs.created_at_edge_cases(support.gregorian)}[family]()


@pytest.mark.parametrize("flags", FLAGS)
def test_extreme_uniform_runs(flags):
    """extreme_runs.extreme_uniform_cases: 12 scripts that drive rank x hits against Remaining = 2^63 - 1, 2^53 and 2^53 + 1 to the edges
    at ranks >= 256, then 100 scripts of 3-4 hot keys, pre-loaded extreme items of either algorithm and 1-3 phases of identical extreme
    requests, 600 / 257 times each and in batches of 200 (k_small under flags 0)"""
    run_family(flags, cases_of("uniform"), by_k_small="all")


@pytest.mark.parametrize("flags", FLAGS)
def test_extreme_walked_segments(flags):
    """extreme_runs.extreme_walk_cases: the pre-loads under requests that all differ — limit 0 and below (rate +-Inf, NaN), rates that are
    no integers, an invalid algorithm here and there — and leaky keys that differ in created_at only by fractions of a token: the
    serial walk and its go_f2i on the device"""
    run_family(flags, cases_of("walk"), by_k_small="none")


@pytest.mark.parametrize("flags", FLAGS)
def test_invalid_at_items(flags):
    """extreme_runs.invalid_at_cases: items with InvalidAt before, at and after the clock, 2^62 and -1, expired by ExpireAt or not, under
    token runs, leaky runs, a walk, and the batches where InvalidAt alone expires them; GetItem after every batch (a survivor keeps its
    invalid_at), a rebuild of the table, GetItem again and Each against the oracle's items"""
    run_family(flags, cases_of("invalid_at"))


@pytest.mark.parametrize("flags", FLAGS)
def test_created_at_edge_ranges(flags):
    """extreme_runs.created_at_edge_cases: created_at at -131073 / -131072 / -131071 and 131070 / 131071 / 131072 ms from the batch clock,
    ranges 255 and 256 ms wide inside a tile's group and across the tiles of a key, groups out of range next to groups in range,
    calendar columns that differ inside one key"""
    run_family(flags, cases_of("created_at"))
