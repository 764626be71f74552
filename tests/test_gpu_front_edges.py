"""guber_front_* on the GPU at the edges its routing kernels branch on (tests/front_edges.py): packed key widths 1 .. 32 and single widths
above, sizes around k_fr_scatter's thread stride and the tile, one odd key in a generation of one width, every request to one engine or
to engine i mod n, GLOBAL requests, fronts of 16, 13, 3 and 1 engines, a generation of more than 1 024 tiles, and the wire decoder's key
rows at two row strides.  Every answer equals ONE oracle fed the requests in arrival order; every key is resident in the engine the
placement's host rule names and in no other; the hash the host routes by equals an XXH64 written in plain Python; nothing is written
behind a generation's results.  The scenarios a - d run on the CPU build of the engine, under AddressSanitizer, in
tests/test_enginesim_cpu.py."""
import numpy as np
import pytest

import gubernator_amd as ga
import front_edges as fe
import support
import wire_replay
from gubernator_amd import wire as gw
from support import Oracle

pytestmark = pytest.mark.gpu


def on_device(torch, dev):
    """(device_side, fetch) for front_edges.drive: a generation's columns and result arrays as device tensors of exactly their size"""
    def device_side(hb, full, r):
        cols = dict(key_bytes=hb.key_bytes, key_off=hb.key_off.view(np.int32), hits=hb.hits, limit=hb.limit, duration=hb.duration, algorithm=hb.algorithm,
                    behavior=hb.behavior.view(np.int32), burst=hb.burst if full else None, created_at=hb.created_at if full else None,
                    is_owner=hb.is_owner if full else None)                       # (None: the column is absent)
        t = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if v is not None else None) for k, v in cols.items()}
        p = {k: (v.data_ptr() if v is not None else None) for k, v in t.items()}
        rt = {k: torch.from_numpy(v).to(dev) for k, v in r.items()}
        b = ga.GuberBatch(hb.n, 0, p["key_bytes"], p["key_off"], p["hits"], p["limit"], p["duration"], p["burst"], p["created_at"], p["algorithm"], p["behavior"],
                          p["is_owner"], None, None, hb.now_ms)
        res = ga.GuberResult(rt["status"].data_ptr(), rt["limit"].data_ptr(), rt["remaining"].data_ptr(), rt["reset_time"].data_ptr(), rt["err"].data_ptr(), 0, 0, 0, 0, 0)
        torch.cuda.synchronize(dev)
        return b, res, (t, rt)

    def fetch(keep):
        return {k: v.cpu().numpy() for k, v in keep[1].items()}
    return device_side, fetch


@pytest.mark.parametrize("n_engines", [16, 13, 3, 1])
def test_key_widths_tile_edges_and_skew(n_engines):
    """front_edges' scenarios a - d (the module's docstring says why there is no e) back to back through ONE front of depth 3 — the smallest
    a front accepts (guber_front_create: 3 .. 16), so a slot is reused every third generation — over n_engines engines on two streams:
    16 and 3 engines with the placement fitted to the traffic (hot keys placed individually), 13 and 1 with the untouched worker rule"""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1600 + n_engines)
    place = ga.Placement(n_engines)
    if n_engines in (16, 3):
        place.observe_keys(*fe.observed_traffic(np.random.default_rng(77), n_engines))
        place.rebalance(0.125, True)
        assert place.n_hot() > 0
    strs = [torch.cuda.Stream(device=dev) for _ in range(min(2, n_engines))]
    engs = [ga.Engine(cache_size=1 << 14, max_batch=4096, stream=strs[j * len(strs) // n_engines].cuda_stream) for j in range(n_engines)]
    scratch = ga.Engine(cache_size=64, max_batch=256)
    errors = fe.error_answers(scratch)
    scratch.close()
    fr = ga.Front(engs, place if n_engines > 1 else None, max_n=2049, depth=3, global_engine=n_engines - 1)
    orc = Oracle(cache_size=1 << 20)
    device_side, fetch = on_device(torch, dev)
    count, sizes = fe.drive(ga, engs, fr, place, orc, fe.generations(n_engines, place, rng, depth=3), device_side, fetch, errors, n_engines - 1)
    assert count == 69 and min(sizes) > 0, (count, sizes)
    fr.close()
    for e in engs:
        e.close()
    place.close()


def test_a_generation_of_more_than_1024_tiles():
    """two generations of 1 048 576 + 1 025 requests (1 026 tiles: every thread of k_fr_scan sums two tiles, thread 512 the last two, the
    threads behind it none) over 50 000 keys of 15 bytes on 16 engines over three streams; the second one's last key is a byte longer, so
    it is ragged by its last lane alone.  Shares go in one piece (max_batch 131 072 against about 65 600 per engine)."""
    import torch
    dev = torch.device("cuda", 0)
    S = 16
    rng = np.random.default_rng(4242)
    place = ga.Placement(S)
    strs = [torch.cuda.Stream(device=dev) for _ in range(3)]
    engs = [ga.Engine(cache_size=1 << 14, max_batch=131072, stream=strs[j * 3 // S].cuda_stream) for j in range(S)]
    fr = ga.Front(engs, place, max_n=fe.BIG_N, depth=3)
    orc = Oracle(cache_size=1 << 20, workers=8)
    device_side, fetch = on_device(torch, dev)
    count, sizes = fe.drive(ga, engs, fr, place, orc, fe.generations(S, place, rng, big=True), device_side, fetch, {}, -1, threads=8, group=2, probe_limit=2000)
    assert count == 2 and min(sizes) > 0, (count, sizes)
    assert sum(e.stats()["retries"] for e in engs) == 0
    fr.close()
    for e in engs:
        e.close()
    place.close()


@pytest.mark.parametrize("max_key_bytes", [16, 64])
def test_rows_from_the_wire_decoder_at_key_width_edges(max_key_bytes):
    """guber_wire_dev_eval_front: the decoder's key rows (key_stride, key_len) instead of packed keys.  The decoder's rows are
    max_key_bytes rounded up to 8, plus 8, bytes apart: max_key_bytes 16 gives key_stride 24 (below the 32 bytes k_fr_count's speculative
    hash needs of a row: every key is hashed from memory) and 64 gives 72 (the four words are requested ahead).  max_key_bytes 24 would
    give 32 already, so the smaller geometry is 16 and takes the HashKey widths that fit it.  HashKey = name + "_" + unique_key of one
    width per run — 3, 8, 15, 16 at stride 24; 3, 8, 24, 31, 32, 33 at stride 72 (3 is the shortest HashKey there is: name and unique_key
    are both non-empty, gubernator.go:208-217) — and a run of width 15 whose last key is a byte longer;
    n = 1, 257, 1 025 items over four tables; every run equals ONE oracle fed the flat item list."""
    from test_wire_cpu import NOW, expected_key
    rng = np.random.default_rng(50 + max_key_bytes)
    place = ga.Placement(4)
    e0 = ga.Engine(cache_size=1 << 14, max_batch=4096, max_key_bytes=max_key_bytes)
    engs = [e0] + [ga.Engine(cache_size=1 << 14, max_batch=4096, max_key_bytes=max_key_bytes, stream=e0.stream_handle()) for _ in range(3)]
    fr = ga.Front(engs, place, max_n=4096, depth=3)
    dec = gw.DevWireDecoder(e0, max_items=4096, max_payload_bytes=1 << 20, max_rpcs=64)
    o = support.Oracle(cache_size=1 << 20)
    now = NOW
    widths = [3, 8, 15, 16] if max_key_bytes == 16 else [3, 8, 24, 31, 32, 33]
    seen = set()
    for run, W in enumerate(widths + ["ragged"]):
        for n in (1, 257, 1025):
            w = 15 if W == "ragged" else W
            pop = 40 if w == 3 else 300                                  # ("n_" + one character: the digits and letters)
            alphabet = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
            def ukey(k):
                return alphabet[k] if w == 3 else ("%0*d" % (w - 2, k))
            ids = rng.integers(0, pop, n)
            flat = [dict(name="n", unique_key=ukey(int(k)), hits=1, limit=5 + int(k) % 26, duration=60_000, algorithm=int(i // 97 + run) % 2,
                         behavior=0, burst=0, created_at=0) for i, k in enumerate(ids)]
            if W == "ragged":
                flat[-1]["unique_key"] += "x"
            assert all(len(expected_key(r)) == w for r in flat[:-1])
            cut = sorted(set(rng.integers(0, n + 1, 3).tolist()) | {0, n})
            rpcs = [flat[a:b] for a, b in zip(cut, cut[1:]) if b > a]
            status, first, count, got_n = dec.decode([wire_replay.pb_request(r) for r in rpcs], now)
            assert (status == 0).all() and got_n == n
            cols = dec.columns()
            assert cols["keys"] == [expected_key(r) for r in flat]
            got = dec.eval_front(fr)
            want = o.eval(support.HostBatch([expected_key(r) for r in flat], 1, np.array([r["limit"] for r in flat], np.int64), 60_000, now,
                                            algorithm=np.array([r["algorithm"] for r in flat], np.uint8)))
            res = ga.HostResult(n)
            for name in ("status", "limit", "remaining", "reset_time", "err"):
                getattr(res, name)[:n] = getattr(got, name)[:n]
            support.assert_results_equal(res, want, f"stride {8 + (max_key_bytes + 7) // 8 * 8} width {W} n={n}")
            seen.update(expected_key(r) for r in flat)
            now += 700
    keys = sorted(k if isinstance(k, bytes) else k.encode() for k in seen)
    sh = fe.check_hashes(place, keys)
    held = [set(it["key"] for it in e.each()) for e in engs]
    for k, j in zip(keys, sh.tolist()):
        assert [q for q in range(4) if k in held[q]] == [j], (k, j)
    assert sum(e.size() for e in engs) == o.size() == len(keys)
    dec.close(); fr.close()
    for e in engs:
        e.close()
    place.close(); o.close()
