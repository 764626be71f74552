"""guber_front_* on the GPU at the edges of its copy kernels' index arithmetic (tests/front_runs.py): k_fr_scatter and k_fr_out put a tile
into the shares' order in LDS and find a sorted element's engine back from the prefix of the tile's sixteen counts — so: everything to one
engine, to the last one, only the first and the last engine populated, an engine with exactly one request at a tile's first and last
position, engine i mod n, a last partial tile that goes to a middle engine; sizes around the thread stride and the tile, up to four tiles and
one; packed keys of 7, 8, 9, 16 and 32 bytes, a ragged generation per size whose one odd key ends a run, and a packed one behind it in the
same slot; all optional columns in every second generation.  Fronts of 1, 2, 12 and 16 engines over caches that bind, against ONE oracle
with as many workers (the untouched placement IS the reference's worker rule, as in tests/test_gpu_front.py): every answer in arrival
order, the sentinels behind a generation's results untouched, nothing forced, no retries, as many resident items as the oracle."""
import numpy as np
import pytest

import gubernator_amd as ga
import front_edges as fe
import front_runs as frn
from support import Oracle
from test_gpu_front_edges import on_device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_engines", frn.ENGINE_COUNTS)
def test_runs_of_every_shape_through_the_copy_kernels(n_engines):
    """72 generations (nine sizes x (a ragged one + seven plans)) back to back through ONE front of depth 3, handed in two, three and
    four (depth + 1) per call: a slot is reused every third generation, across calls and inside one"""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2600 + n_engines)
    place = ga.Placement(n_engines) if n_engines > 1 else None
    strs = [torch.cuda.Stream(device=dev) for _ in range(min(2, n_engines))]
    engs = [ga.Engine(cache_size=frn.CACHE_PER_ENGINE, max_batch=8192, stream=strs[j * len(strs) // n_engines].cuda_stream) for j in range(n_engines)]
    fr = ga.Front(engs, place, max_n=max(frn.SIZES), depth=3)
    orc = Oracle(cache_size=frn.CACHE_PER_ENGINE * n_engines, workers=n_engines)
    route = (lambda keys: place.route_keys(*fe.pack(keys))[0]) if place is not None else None
    device_side, fetch = on_device(torch, dev)
    count = frn.drive(engs, fr, orc, frn.generations(n_engines, route, rng, depth=3), device_side, fetch)
    assert count == len(frn.SIZES) * (1 + len(frn.PLANS))
    assert sum(e.stats()["eviction_passes"] for e in engs) >= 1          # (the caches did bind)
    fr.close()
    for e in engs:
        e.close()
    if place is not None:
        place.close()
    orc.close()
