"""guber_front_probe_missing_dev / guber_front_eval_store_dev on the GPU (tests/front_store.py): the Store side channel — Store.Get on a
miss, Remove / OnChange after a request, store.go:49-65 — for generations routed on the device.  Parity: random generations with a
write-through mock store through probe -> Store.Get -> add_items -> eval_store_dev against ONE oracle (answers, the events in arrival
order with their items, every key's whole call sequence, the engines' sizes), on fronts whose generations take one pair of launches for
all tables and on one whose shares take the owner-partitioned pipeline, in pieces.  Probe edges: against a ten-line model of the two
rules.  Collisions: engines whose election sees six bits of the hash — the host decides, and a counter says that it did."""
import numpy as np
import pytest

import gubernator_amd as ga
import front_edges as fe
import front_store as fs
import support
from support import Oracle
from test_gpu_front_edges import on_device

pytestmark = pytest.mark.gpu


def device(torch):
    dev = torch.device("cuda", 0)
    device_side, fetch = on_device(torch, dev)

    def make_dev_gen(hb):
        b, res, keep = device_side(hb, True, fe.result_arrays(hb.n))
        b._keep = res._keep = keep

        def fetched():
            out = fetch(keep)
            for name, a in out.items():
                s = fe.SENTINEL_U8 if a.dtype == np.uint8 else fe.SENTINEL_I64
                assert (a[hb.n:] == s).all(), f"{name} written behind the generation's end"
            return out
        return b, res, fetched
    return dev, make_dev_gen


def setup(torch, dev, n_engines, n_streams, max_batch, flags=0, max_n=4096, global_engine=-1):
    place = ga.Placement(n_engines) if n_engines > 1 else None
    strs = [torch.cuda.Stream(device=dev) for _ in range(n_streams)]
    engs = [ga.Engine(cache_size=1 << 14, max_batch=max_batch, flags=flags, stream=strs[j * n_streams // n_engines].cuda_stream) for j in range(n_engines)]
    for e in engs:
        e.profile(True)
    front = ga.Front(engs, place, max_n=max_n, depth=3, global_engine=global_engine)
    route = (lambda keys: place.route_keys(*fe.pack(keys))[0]) if place is not None else None
    return place, engs, front, route, strs


def launches(engs):
    out, us = {}, {}
    for e in engs:
        for k, v in e.profile_read().items():
            out[k] = out.get(k, 0) + v[0]
            us[k] = us.get(k, 0.0) + v[1] * 1e3
    return {k: v for k, v in out.items() if v}, us


def close(place, engs, front):
    front.close()
    for e in engs:
        e.close()
    if place is not None:
        place.close()


PART = ("k_eval3", "k_eval3_multi", "k_evalpart_multi")


@pytest.mark.parametrize("n_engines,n_streams,max_batch,flags,resets,want", [
    (1, 1, 8192, 0, True, ("k_eval2", "k_eval3")),
    (4, 1, 8192, 0, True, ("k_eval2_multi",)),
    (16, 1, 8192, 0, True, ("k_eval2_multi",)),
    (6, 3, 2048, ga.FLAG_TEST_FORCE_PART, True, PART),
    (6, 3, 256, ga.FLAG_TEST_FORCE_PART, False, PART),
], ids=["1_engine", "4_engines-one_pair", "16_engines-one_pair", "6_engines_3_streams-owner_partitioned", "6_engines_3_streams-shares_in_pieces"])
def test_store_generations_match_the_oracle(n_engines, n_streams, max_batch, flags, resets, want):
    """12 generations of 1 - 3000 requests (400 keys, Zipf 1.3, both algorithms, RESET_REMAINING and DRAIN_OVER_LIMIT mixed in, is_owner = 0
    in every third), caches that do not bind.  1, 4 and 16 engines on one stream: one pair of launches for all tables.  6 engines on three
    streams, created with FLAG_TEST_FORCE_PART so that shares of a few hundred requests take the owner-partitioned pipeline (k_part / k_own /
    k_eval3, the held-back k_eval3 included).  The generator's resets cut a generation every few hundred requests, so with max_batch 2048 no
    share is cut into pieces; the last case runs the same generator without RESET_REMAINING (no cuts: shares of up to a thousand requests)
    over engines of max_batch 256, whose shares go in pieces with the side channel's pointers offset like their results."""
    import torch
    dev, make_dev_gen = device(torch)
    place, engs, front, _, strs = setup(torch, dev, n_engines, n_streams, max_batch, flags)
    orc = Oracle(cache_size=1 << 20)
    count, cuts = fs.parity(front, engs, orc, make_dev_gen, support.MockStore, seed=500 + n_engines, steps=12, max_n=3000, resets=resets)
    ran, us = launches(engs)
    st = front.store_stats()
    print(f"{n_engines} engines: {count} generations, {cuts} cuts, {st}, launches {ran}")
    print("microseconds per launch:", {k: round(us[k] / ran[k], 1) for k in fs.NEW_KERNELS if ran.get(k)})
    assert count == 12 and (cuts > 0) == resets and st["collisions"] == 0, st
    assert all(ran.get(k, 0) > 0 for k in fs.NEW_KERNELS), ran
    assert ran["k_fr_ask"] == 2 * ran["k_fr_elect"] == 2 * ran["k_fr_missing"] and ran["k_fr_out_store"] == st["evaluations"], (ran, st)
    assert any(ran.get(k, 0) > 0 for k in want), (want, ran)
    if n_engines > 1 and n_streams == 1:
        assert ran.get("k_own_multi", 0) == 0 and ran.get("k_own", 0) == 0, ran
    if not resets:                                                  # (without pieces an engine takes at most one batch per generation)
        assert sum(e.stats()["batches"] for e in engs) > n_engines * count, [e.stats()["batches"] for e in engs]
    assert sum(e.stats()["retries"] for e in engs) == 0
    close(place, engs, front)
    orc.close()


@pytest.mark.parametrize("n_engines", [3, 1])
@pytest.mark.parametrize("packed", [True, False], ids=["packed_16", "ragged"])
def test_the_probe_at_its_edges(n_engines, packed):
    """n in (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049) x (every key resident: nothing asked; every key missing and distinct: everything
    asked, and GUBER_E_NOMEM with the size needed when the arrays hold one entry too few; half resident with repeats); one key 2 049 times;
    everything routed to the last engine; a cut at 1, at 1 024 and at n - 1; a reset as the last request of its key; resets on two keys; an
    ask candidate behind the cut; an empty key — each against front_store.model()"""
    import torch
    dev, make_dev_gen = device(torch)
    place, engs, front, route, strs = setup(torch, dev, n_engines, 1, 4096)
    p = fs.Probe(front, engs, make_dev_gen, route)
    fs.probe_sizes_and_residency(p, packed)
    fs.probe_skew_and_cuts(p, packed, n=2049, n_engines=n_engines)
    ran, _ = launches(engs)
    assert ran.get("k_fr_elect", 0) > 0 and ran.get("k_fr_out_store", 0) == 0 and front.store_stats()["collisions"] == 0, ran
    close(place, engs, front)


def test_the_contract_between_probe_and_evaluation():
    """guber_front_eval_store_dev after a cut report, with another generation than the probed one, or after a plain call has dropped the
    probed generation: GUBER_E_INVALID_ARG; the plain guber_front_eval_dev in between answers as the oracle does"""
    import torch
    dev, make_dev_gen = device(torch)
    place, engs, front, route, strs = setup(torch, dev, 3, 1, 4096)
    orc = Oracle(cache_size=1 << 20)
    fs.probe_contract(fs.Probe(front, engs, make_dev_gen, route), orc)
    close(place, engs, front)
    orc.close()


def test_global_requests_are_a_key_of_their_own():
    """a front whose rule names a global_engine (the last of three engines): a key's Behavior_GLOBAL requests live in that engine's table —
    asked for there, resident there, and neither cutting nor cut by the key's other requests, as include/guber_gpu.h says"""
    import torch
    dev, make_dev_gen = device(torch)
    place, engs, front, route, strs = setup(torch, dev, 3, 1, 4096, global_engine=2)
    fs.probe_global(fs.Probe(front, engs, make_dev_gen, route), 2)
    assert front.store_stats()["collisions"] == 0
    close(place, engs, front)


def test_keys_that_share_a_hash_are_decided_on_the_host():
    """engines created with FLAG_TEST_WEAK_HASH (six bits of the hash reach the election table), 300 keys, n = 2 049, probe only: the list
    and cut_at equal the model's exactly, and guber_front_store_stats_t.collisions says the host decided"""
    import torch
    dev, make_dev_gen = device(torch)
    place, engs, front, route, strs = setup(torch, dev, 3, 1, 4096, flags=ga.FLAG_TEST_WEAK_HASH)
    fs.probe_collisions(fs.Probe(front, engs, make_dev_gen, route))
    close(place, engs, front)
