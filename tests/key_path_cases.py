"""Generations for the key path of the device front and the pipelines behind it (gubernator_amd/csrc: key_fetch_spec and
xxhash64_words4_uniform in k_fr_count / k_part / k_front, BatchView::key_width for the pieces of a packed generation's shares), and the
CPU case that drives them; shared by tests/test_gpu_key_path.py (the product library on a GPU) and tests/test_key_path_cpu.py (the same
kernels compiled for the CPU).  numpy only, like tests/front_runs.py, whose driver and checks it uses.

What can go wrong on this path is decided by the KEY WIDTH (which loads fetch the key: 8 bytes up to width 8, 16 up to 16, 16 + 8 up to
24, 32 up to 31, none at 32; which rounds the hash runs: width >> 3 word rounds, the 4-byte round, width & 3 byte rounds), by WHERE A KEY
LIES (a share's piece starts at d0 x width: odd addresses for odd widths; the last keys of a buffer, 8 readable bytes behind them) and by
WHICH PIPELINE a piece takes (caches that bind send it through the LRU pre-pass, which cuts it into pieces of the cache's size, and the
two-launch pipeline; others through the owner-partitioned one) — so: every width of WIDTHS at every size of the caller's choice, sizes
around the wave (64), the thread stride of the copy kernels (256) and the tile (1 024), keys drawn from small pools so that they repeat
across tiles and across the pieces' boundaries, per size one generation with a single key of another width and one whose keys are all
33 bytes (one width, but not packed), each followed `depth` generations later, in the same slot, by a packed one.  The 8 bytes behind a
key buffer are 0xFF.  burst / created_at / is_owner are present in every second generation."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)                          # (run as a script: the package is importable from the repository tree)

import front_edges as fe
import front_runs as frn

SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
CPU_SIZES = (1, 63, 64, 65, 257, 1025)                # the fiber emulation runs a tile in about a second: the smallest sizes
WIDTHS = (1, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32)
ODD_WIDTH, WIDE = 11, 33                              # the one key of a ragged generation; a single width that is not packed
ENGINE_COUNTS = (1, 3, 16)
KEYS_PER_ENGINE = 28                                  # per width: thirteen widths make about 360 keys per engine ...
CACHE_PER_ENGINE = 192                                # ... over caches of 192 items: they bind, and a share above 192 requests goes in pieces


def pack_ff(keys):
    """front_edges.pack with 0xFF in the 8 readable bytes behind the last key"""
    kb, off = fe.pack(keys)
    kb[int(off[-1]):] = 0xFF
    return kb, off


def pools(n_engines, route, rng):
    """{width: [keys of engine 0, keys of engine 1, ...]}; route(keys) -> the engine of every key (None: one engine).  Width 1 has 255
    keys in all (bytes 1 .. 255)."""
    out = {}
    for W in WIDTHS + (ODD_WIDTH, WIDE):
        keys = [bytes([b]) for b in rng.permutation(255) + 1] if W == 1 else fe.keys_of_width(W, KEYS_PER_ENGINE * n_engines, rng)
        sh = np.zeros(len(keys), np.uint32) if route is None else np.asarray(route(keys))
        out[W] = [[k for k, s in zip(keys, sh.tolist()) if s == e] for e in range(n_engines)]
        assert all(len(b) >= 2 for b in out[W]), (W, [len(b) for b in out[W]])
    return out


def generations(n_engines, route, rng, sizes=SIZES, widths_per_size=None, depth=3):
    """yields (label, generation, full_columns, engines) as front_runs.generations does.  Per size: packed generations of widths_per_size
    widths (None: all of WIDTHS; otherwise the widths go round, so that every width meets several sizes), with the two ragged ones in
    between — the packed generation `depth` behind each lies in its slot."""
    P = pools(n_engines, route, rng)
    g = w_at = 0

    def make(n, W, odd_at=None):
        nonlocal g
        engines = (np.arange(n) * 7 // 3 % n_engines).astype(np.uint32)
        pick = rng.integers(0, 1 << 30, n)
        keys = [P[W][e][r % len(P[W][e])] for e, r in zip(engines.tolist(), pick.tolist())]
        what = f"W={W}"
        if odd_at is not None:
            b = P[ODD_WIDTH][int(engines[odd_at])]
            keys[odd_at] = b[int(pick[odd_at]) % len(b)]
            what += f" one key of {ODD_WIDTH} bytes at {odd_at}"
        full = g % 2 == 1
        now = fe.NOW0 + g * fe.STEP_MS
        c = fe._columns(n, g, now, fe._limit_of(np.array([frn.hash_id(k) for k in keys])), full, rng)
        hb = fe.Gen(pack_ff(keys), c["hits"], c["limit"], c["duration"], now, burst=c["burst"], created_at=c["created_at"], algorithm=c["algorithm"],
                    behavior=c["behavior"], is_owner=c["is_owner"])
        hb.odd, hb.for_oracle = None, hb
        g += 1
        return f"n={n} engines={n_engines} {what} full={full}", hb, full, engines

    for n in sizes:
        ws = list(WIDTHS) if widths_per_size is None else [WIDTHS[(w_at + k) % len(WIDTHS)] for k in range(widths_per_size)]
        w_at += 0 if widths_per_size is None else widths_per_size
        assert len(ws) >= depth
        for k, W in enumerate(ws):
            if k == 1 and n > 1:                      # (one request is one width)
                yield make(n, W, odd_at=n - 1 if g % 2 else n // 2)
            if k == 2:
                yield make(n, WIDE)
            yield make(n, W)


def count(sizes, widths_per_size=None):
    per = len(WIDTHS) if widths_per_size is None else widths_per_size
    return sum(per + 1 + (1 if n > 1 else 0) for n in sizes)


def cpu_case(n_engines):
    """the generations at the smallest sizes through guber_front_eval_dev on the CPU build of the engine ("device" pointers are numpy
    buffers), against ONE oracle with as many workers: front_runs.drive's checks"""
    import gubernator_amd as ga
    import support
    assert "enginesim" in ga.LIB_PATH, "this case is for the CPU build of the engine (GUBER_HIP_LIB)"
    rng = np.random.default_rng(3100 + n_engines)
    place = ga.Placement(n_engines) if n_engines > 1 else None
    e0 = ga.Engine(cache_size=CACHE_PER_ENGINE, max_batch=8192)
    engs = [e0] + [ga.Engine(cache_size=CACHE_PER_ENGINE, max_batch=8192, stream=e0.stream_handle()) for _ in range(n_engines - 1)]
    fr = ga.Front(engs, place, max_n=max(CPU_SIZES), depth=3)
    orc = support.Oracle(cache_size=CACHE_PER_ENGINE * n_engines, workers=n_engines)
    route = (lambda keys: place.route_keys(*fe.pack(keys))[0]) if place is not None else None

    def device_side(hb, full, r):
        cols = dict(key_bytes=hb.key_bytes, key_off=hb.key_off.view(np.int32), hits=hb.hits, limit=hb.limit, duration=hb.duration, algorithm=hb.algorithm,
                    behavior=hb.behavior.view(np.int32), burst=hb.burst if full else None, created_at=hb.created_at if full else None,
                    is_owner=hb.is_owner if full else None)
        p = {k: (v.ctypes.data if v is not None else None) for k, v in cols.items()}
        b = ga.GuberBatch(hb.n, 0, p["key_bytes"], p["key_off"], p["hits"], p["limit"], p["duration"], p["burst"], p["created_at"], p["algorithm"], p["behavior"],
                          p["is_owner"], None, None, hb.now_ms)
        res = ga.GuberResult(r["status"].ctypes.data, r["limit"].ctypes.data, r["remaining"].ctypes.data, r["reset_time"].ctypes.data, r["err"].ctypes.data, 0, 0, 0, 0, 0)
        return b, res, (cols, r)

    got = frn.drive(engs, fr, orc, generations(n_engines, route, rng, sizes=CPU_SIZES, widths_per_size=4), device_side, lambda keep: keep[1])
    assert got == count(CPU_SIZES, 4), got
    assert sum(e.stats()["eviction_passes"] for e in engs) >= 1          # (the caches did bind)
    fr.close()
    for e in engs:
        e.close()
    if place is not None:
        place.close()
    orc.close()


if __name__ == "__main__":
    for ne in ENGINE_COUNTS:
        cpu_case(ne)
    print("KEY PATH CASE OK")
