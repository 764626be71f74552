"""guber_mesh_* on the GPU (gubernator_amd/csrc/guber_mesh.h, guber_kernels_mesh.h): the scenarios of tests/mesh_cases.py with every rank a
logical rank of device 0 — a stream of requests per rank, routed to its owning ranks on the device by the ring, evaluated there in
source order, answered in arrival order where it arrived.  Every answer equals ONE oracle per rank fed what the order rule says; nothing is
written behind a generation's results; every key is resident in exactly the engine of exactly the rank the host ring and placement name.
Scenarios a - f and h also run on the CPU build of the engine (tests/test_mesh_cpu.py)."""
import numpy as np
import pytest

import gubernator_amd as ga
import mesh_cases as mc
import support

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    dev = torch.device("cuda", 0)
    strs = [torch.cuda.Stream(device=dev) for _ in range(2)]

    def new_engines(rank, flags, kw):
        # (the engines of all ranks on two streams: a rank's engines alternate between them, so do the ranks of one engine)
        return [ga.Engine(flags=f, stream=strs[(rank + j) % 2].cuda_stream, **kw) for j, f in enumerate(flags)]

    def upload(a):
        t = torch.from_numpy(a).to(dev)
        torch.cuda.synchronize(dev)
        return t, t.data_ptr()

    def make_world(**kw):
        return mc.World(ga, support, new_engines=new_engines, upload=upload, download=lambda t: t.cpu().numpy(), **kw)

    def plain_front(n_engines, max_n):
        engs = new_engines(0, [0] * n_engines, dict(cache_size=1 << 14, max_batch=4096, max_key_bytes=mc.MAX_KEY))
        place = ga.Placement(n_engines)
        fr = ga.Front(engs, place, max_n=max_n, depth=3)

        def run(g):
            kb, off = g.packed()
            src = dict(key_bytes=kb, key_off=off.view(np.int32), hits=g.hits, limit=g.limit, duration=g.duration, burst=g.burst, created_at=g.created_at,
                       algorithm=g.algorithm, behavior=g.behavior.view(np.int32))
            h = {k: (upload(np.ascontiguousarray(v)) if v is not None else (None, None)) for k, v in src.items()}
            r = {k: upload(v) for k, v in mc.result_arrays(g.n).items()}
            b = ga.GuberBatch(g.n, 0, h["key_bytes"][1], h["key_off"][1], h["hits"][1], h["limit"][1], h["duration"][1], h["burst"][1], h["created_at"][1],
                              h["algorithm"][1], h["behavior"][1], None, None, None, g.now)
            res = ga.GuberResult(r["status"][1], r["limit"][1], r["remaining"][1], r["reset_time"][1], r["err"][1], 0, 0, 0, 0, 0)
            assert fr.eval_dev((ga.GuberBatch * 1)(b), (ga.GuberResult * 1)(res), 1) == 1
            fr.synchronize()
            return {k: v[0].cpu().numpy() for k, v in r.items()}

        def close():
            fr.close()
            for e in engs:
                e.close()
            place.close()
        return run, close
    return make_world, plain_front


def test_a_sizes_around_the_tile_mixed_across_ranks_and_residency(gpu):
    """a + i: W = 3, two engines per rank, generations of 0, 1, 63, 64, 65, 1 023, 1 024, 1 025 and 2 049 requests mixed across the ranks of
    a call, one rank empty, all but one empty; a dozen calls over one population, buckets run out; then every key's residency"""
    assert mc.scenario_a(gpu[0]) == len(mc.SIZES_A)


def test_b_ragged_empty_and_over_long_keys_and_residency(gpu):
    """b + i: key widths 3, 8, 31, 32, 33 and max_key_bytes with one key a byte longer per call, a call of mixed widths; the empty key and
    the key of max_key_bytes + 1 stay on their arrival rank (the forwarded count says so) with the front's item error"""
    assert mc.scenario_b(gpu[0]) == 7


def test_c_the_order_across_sources(gpu):
    """c: one hot token key from every rank in one call turns OVER_LIMIT exactly where source 0, 1, 2 in turn exhaust it, and stays so"""
    mc.scenario_c(gpu[0])


@pytest.mark.parametrize("hash_kind", ["fnv1", "fnv1a"])
def test_d_skew(gpu, hash_kind):
    """d: every request of every rank to one owner; request i to rank i mod W — on a ring of either hash"""
    mc.scenario_d(gpu[0], hash_kind)


def test_e_an_inflow_larger_than_the_fronts_max_n(gpu):
    """e: W = 4, every rank sends 2 049 requests rank 2 owns: its front takes 8 196 requests as generations of at most 2 049"""
    mc.scenario_e(gpu[0])


def test_f_global_requests_stay_on_their_arrival_rank(gpu):
    """f: W = 2, half of the requests GLOBAL: none is forwarded, they end up in the arrival rank's GLOBAL engine with is_owner from the ring"""
    mc.scenario_f(gpu[0])


def test_g_sixteen_ranks(gpu):
    """g: sixteen ranks of one engine each on two streams, 1 025 requests per rank (a ring of 64 KB: searched in global memory)"""
    mc.scenario_g(gpu[0])


def test_h_one_rank_is_the_front_alone(gpu):
    """h: W = 1 does no exchange: the answers of a plain front over a second set of engines"""
    mc.scenario_h(*gpu)
