"""Batches that pin the paths of the evaluation kernels which the random streams reach only by chance: the uniform runs the closed
forms of guber_algo.h decline (fixed point, period-2 cycle, reconfigure / create then extrapolate, stepping one by one, the calendar),
the serial walk of a heterogeneous segment (the recency stamp it leaves included), and the walk's step from one 32-tile word of the
segment's tile map to the next.  Shared by
tests/test_kernels_devsim.py (the kernel source on the CPU) and tests/test_gpu_parity.py (the product library); numpy only — the engine
and the oracle are the caller's.

Every case is a list of batches: an optional batch that makes the bucket resident, the batch the case is about, and a batch of 8 plain
requests on the same keys, which shows the bucket the run left behind.  The caller compares every batch with the oracle."""
import numpy as np

from gubernator_amd.abi import HostBatch

NOW0 = 1_700_000_000_000
TOKEN, LEAKY = 0, 1
GREGORIAN, RESET_REMAINING, DRAIN_OVER_LIMIT = 4, 8, 32
INVALID_ALGORITHM = 7
MINUTE = 60_000
RUN, OTHERS = 600, 40                  # one key 600 times (3 tiles, the last one partial) among 40 keys asked for once
SMALL_RUN, SMALL_OTHERS = 190, 10      # the same in a batch of 200: one launch, one workgroup


def _layout(tag, run, others):
    """the keys of a batch of run + others requests and the positions of the run's key: the other keys spread evenly between them"""
    n = run + others
    other_at = (np.arange(others) * n // others + n // (2 * others)).astype(np.int64)
    is_run = np.ones(n, bool)
    is_run[other_at] = False
    hot = f"run_{tag}".encode()
    keys, o = [], 0
    for i in range(n):
        if is_run[i]:
            keys.append(hot)
        else:
            keys.append(f"one_{tag}_{o}".encode())
            o += 1
    return keys, np.nonzero(is_run)[0]


def _columns(n, **kw):
    c = dict(hits=np.ones(n, np.int64), limit=np.full(n, 100, np.int64), duration=np.full(n, MINUTE, np.int64), algorithm=np.zeros(n, np.uint8),
             behavior=np.zeros(n, np.uint32))
    for k, v in kw.items():
        c[k][:] = v
    return c


def _batch(keys, c, now, **extra):
    return HostBatch(keys, c["hits"], c["limit"], c["duration"], now, algorithm=c["algorithm"], behavior=c["behavior"], **extra)


def _after(keys, at, now, algorithm, limit, duration=MINUTE):
    """8 plain requests on the case's keys: the run's key four times, four of the others"""
    run = keys[at[0]]
    others = [k for k in keys[:64] if k != run][:4]
    ks = [run] * 4 + others
    ks = (ks * 8)[:8]
    return HostBatch(ks, 1, limit, duration, now, algorithm=algorithm)


def uniform_cases(greg_fn, run=RUN, others=OTHERS, now=NOW0):
    """-> [(label, [batches])]: ONE key `run` times with identical requests that token_fast / leaky_fast decline, each case with and
    without DRAIN_OVER_LIMIT.  greg_fn(now_ms, d) -> (greg_expire, greg_duration) as the host layer precomputes them."""
    out = []
    for drain in (0, DRAIN_OVER_LIMIT):
        # (label, algorithm, what the run's requests carry, the resident bucket's limit or None for a new key)
        specs = [("token RESET_REMAINING hits 1: period 2", TOKEN, dict(behavior=RESET_REMAINING), None),
                 ("token hits 0: fixed point", TOKEN, dict(hits=0), None),
                 ("token hits -1: stepped one by one", TOKEN, dict(hits=-1), None),
                 ("token limit 100 -> 5000 hits 3: reconfigure, then extrapolate", TOKEN, dict(hits=3, limit=5000), 100),
                 ("leaky new key limit 1000: create, then extrapolate", LEAKY, dict(limit=1000), None),
                 ("leaky new key limit 100: over the limit mid-run", LEAKY, dict(limit=100), None),
                 ("leaky GREGORIAN with the calendar columns", LEAKY, dict(limit=1000, duration=1, behavior=GREGORIAN), None)]
        for k, (what, algo, req, resident) in enumerate(specs):
            label = f"{what}{' DRAIN' if drain else ''} n={run + others}"
            keys, at = _layout(f"u{run}_{drain}_{k}", run, others)
            n = len(keys)
            batches = []
            if resident is not None:
                batches.append(_batch(keys, _columns(n, algorithm=algo, limit=resident), now))
                now += 1
            c = _columns(n, algorithm=algo)
            for name, v in req.items():
                c[name][at] = v
            c["behavior"][at] |= drain
            extra = {}
            if req.get("behavior", 0) & GREGORIAN:
                ge, gd = np.zeros(n, np.int64), np.zeros(n, np.int64)
                ge[at], gd[at] = greg_fn(now, int(req["duration"]))
                extra = dict(greg_expire=ge, greg_duration=gd)
            batches.append(_batch(keys, c, now, **extra))
            now += 1
            batches.append(_after(keys, at, now, algo, int(c["limit"][at[0]])))
            now += 1
            out.append((label, batches))
    return out


def walk_cases(now=NOW0 + 1000):
    """-> [(label, [batches])]: segments whose requests differ — the segment's first request walks them in order"""
    out = []
    # hits 1, 2, 1, 2, ... and an invalid algorithm last: the bucket's recency stamp is that of the last request that reached the cache
    keys, at = _layout("w_alt", RUN, OTHERS)
    n = len(keys)
    c = _columns(n, limit=5000)
    c["hits"][at] = 1 + np.arange(RUN) % 2
    c["algorithm"][at[-1]] = INVALID_ALGORITHM
    out.append(("walk: hits 1 / 2 alternating, an invalid algorithm last", [_batch(keys, c, now), _after(keys, at, now + 1, TOKEN, 5000)]))
    now += 2
    # nothing but invalid algorithms: no request reaches the cache, no bucket is written
    keys, at = _layout("w_inv", RUN, OTHERS)
    c = _columns(n)
    c["algorithm"][at] = INVALID_ALGORITHM
    out.append(("run: every request of an invalid algorithm", [_batch(keys, c, now), _after(keys, at, now + 1, TOKEN, 100)]))
    now += 2
    # a leaky key whose requests differ only in created_at: a new key is walked; the resident bucket, with nobody leaking, is a run in
    # which every request uses its own created_at
    keys, at = _layout("w_created", RUN, OTHERS)
    c = _columns(n, algorithm=LEAKY, limit=1000)
    batches = []
    for step in range(2):
        created = np.full(n, now, np.int64)
        created[at] = now - np.arange(RUN) % 50
        batches.append(_batch(keys, c, now, created_at=created))
        now += 1
    batches.append(_after(keys, at, now, LEAKY, 1000))
    out.append(("walk: a leaky key whose requests differ only in created_at", batches))
    return out


WORD_N, WORD_TILES = 8704, (0, 31, 32, 33)            # 34 tiles of 256: the tile map's second 32-tile word holds tiles 32 and 33


def bitmap_word_case(now=NOW0 + 2000):
    """-> (label, [batches]): 8 704 requests, all distinct keys but one whose requests differ and sit in tiles 0, 31, 32 and 33 only"""
    at = np.array([t * 256 + p for t in WORD_TILES for p in (3, 100, 255)], np.int64)
    hot = b"run_word"
    keys = [f"word_{i}".encode() for i in range(WORD_N)]
    for i in at:
        keys[i] = hot
    c = _columns(WORD_N, limit=5000)
    c["hits"][at] = 1 + np.arange(len(at)) % 2
    return "walk across a word of the tile map: tiles 0, 31, 32, 33", [_batch(keys, c, now), _after(keys, at, now + 1, TOKEN, 5000)]


RECENCY_CACHE = 64


def recency_case(now=NOW0 + 4000):
    """-> (label, [batches]) for a cache of RECENCY_CACHE items: the walked segment of walk_cases (its key's last request that reached the
    cache is the batch's second to last: the key is the most recent of the batch's 41), then 30 new keys, which push the 7 oldest items
    out, then the 8 plain requests.  A bucket stamped with any earlier request of the segment is among the seven."""
    keys, at = _layout("r_alt", RUN, OTHERS)
    c = _columns(len(keys), limit=5000)
    c["hits"][at] = 1 + np.arange(RUN) % 2
    c["algorithm"][at[-1]] = INVALID_ALGORITHM
    crowd = HostBatch([f"new_r_{i}".encode() for i in range(30)], 1, 5000, MINUTE, now + 1)
    return "walk under a binding cache: stamped with the last request that reached the cache", [_batch(keys, c, now), crowd, _after(keys, at, now + 2, TOKEN, 5000)]


def all_cases(greg_fn):
    """what both callers run through the batch pipelines"""
    return uniform_cases(greg_fn) + walk_cases() + [bitmap_word_case()]
