"""The key path on the GPU (tests/key_path_cases.py): k_fr_count, k_part and k_front fetch a fixed-width key with the loads its width needs
(key_fetch_spec) and hash it with the rounds its width has (xxhash64_words4_uniform); the pieces of a packed generation's shares carry
BatchView::key_width instead of offsets, which k_fr_scatter no longer writes, and fwd[] is written only for the payload stage's fronts.
Fronts of 1, 3 and 16 engines over max_batch 8 192 and caches of 192 items that bind — so a fixed-width share also goes through the LRU
pre-pass, in pieces that start at d0 x width, and the two-launch pipeline — every packed width 1 .. 32 at every size around the wave, the
copy kernels' thread stride and the tile, ragged generations in between and packed ones behind them in the same slot, 0xFF behind the key
buffers, all optional columns in every second generation.  Against ONE oracle with as many workers, as tests/test_gpu_front_runs.py:
every answer in arrival order, the sentinels behind the results untouched, no retries, nothing forced, as many resident items.  One
payload-stage case: the encoder still finds every answer through fwd[]."""
import ctypes as C

import numpy as np
import pytest

import gubernator_amd as ga
import front_edges as fe
import front_runs as frn
import key_path_cases as kp
import support
import wire_replay
from gubernator_amd import wire as gw
from support import Oracle
from test_gpu_front_edges import on_device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_engines", kp.ENGINE_COUNTS)
def test_fixed_width_keys_through_every_pipeline(n_engines):
    """11 sizes x (11 packed widths + a generation with one odd key + one of 33-byte keys) back to back through ONE front of depth 3"""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3100 + n_engines)
    place = ga.Placement(n_engines) if n_engines > 1 else None
    strs = [torch.cuda.Stream(device=dev) for _ in range(min(2, n_engines))]
    engs = [ga.Engine(cache_size=kp.CACHE_PER_ENGINE, max_batch=8192, stream=strs[j * len(strs) // n_engines].cuda_stream) for j in range(n_engines)]
    fr = ga.Front(engs, place, max_n=max(kp.SIZES), depth=3)
    orc = Oracle(cache_size=kp.CACHE_PER_ENGINE * n_engines, workers=n_engines)
    route = (lambda keys: place.route_keys(*fe.pack(keys))[0]) if place is not None else None
    device_side, fetch = on_device(torch, dev)
    count = frn.drive(engs, fr, orc, kp.generations(n_engines, route, rng), device_side, fetch)
    assert count == kp.count(kp.SIZES) == 142
    assert sum(e.stats()["eviction_passes"] for e in engs) >= 1          # (the caches did bind)
    fr.close()
    for e in engs:
        e.close()
    if place is not None:
        place.close()
    orc.close()


def test_the_payload_stages_encoder_still_reads_fwd():
    """tests/test_gpu_wire_pool.py's one-caller shape at its smallest that still routes (four tables of one stream, RPCs of 1 .. 699
    requests with every field, twenty of them): k_wire_enc takes item i's answer from the shares at fwd[i], so the response bytes equal
    the host transcoder's around ONE oracle only if k_fr_scatter wrote fwd[] for this front — the only kind it still writes it for"""
    from test_wire_cpu import NOW, rand_reqs
    rng = np.random.default_rng(35)
    e0 = ga.Engine(cache_size=1 << 16, max_batch=8192, max_key_bytes=256)
    engs = [e0] + [ga.Engine(cache_size=1 << 16, max_batch=8192, max_key_bytes=256, stream=e0.stream_handle()) for _ in range(3)]
    place = ga.Placement(4)
    pool = gw.WirePool(engs, place, stages=3, max_items=8192, max_payload_bytes=1 << 20, max_rpcs=64)
    o = support.Oracle(cache_size=1 << 20)
    wb = gw.WireBatch(4096, 1 << 20)
    now = NOW
    for k in range(20):
        reqs = rand_reqs(rng, int(rng.integers(1, 700)), bad=(k % 3 == 0))
        payload = wire_replay.pb_request(reqs, peer=bool(k & 1))
        pool.set_clock(now)
        got = pool.get_rate_limits(payload, wrap_errors=not (k & 1))
        wb.reset(now)
        first, count = wb.decode(payload, max_per_rpc=1000)
        o.lib.oracle_eval_batch(o.h, C.byref(wb.view()), C.byref(wb.result()))
        assert got == wb.encode(first, count, wrap_errors=not (k & 1)), f"RPC {k}: {len(reqs)} requests"
        now += int(rng.integers(0, 900))
    pool.close()
    for e in reversed(engs):
        e.close()
    place.close()
    o.close(); wb.close()
