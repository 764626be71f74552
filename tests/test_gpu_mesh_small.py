"""guber_mesh_eval_small on the GPU (gubernator_amd/csrc/guber_mesh.h; the kernel: k_mx_small, guber_kernels_small.h): the scenarios of
tests/mesh_small_cases.py with every rank a logical rank of device 0 — a call of at most 256 requests over all ranks, from host memory,
one launch per rank.  Every answer equals ONE oracle per rank fed what the order rule says, nothing is written behind a generation's
results, the statistics move as guber_mesh_eval_dev moves them, and every key is resident in exactly the engine of exactly the rank the
host ring and placement name.  With one device the arena is read by the device that allocated it: a kernel on one GPU reading what
another rank's caller wrote through it is not exercised here.  The same scenarios run on the CPU build (tests/test_mesh_small_cpu.py)."""
import numpy as np
import pytest

import gubernator_amd as ga
import mesh_cases as mc
import mesh_small_cases as ms
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
    return ms.wrap_world(ga, support, new_engines, upload, lambda t: t.cpu().numpy()), plain_front


def test_a_sizes_up_to_one_tile_the_refusal_of_257_and_residency(gpu):
    """a: W = 3, two engines and a GLOBAL engine per rank, totals of 0, 1, 2, 63, 64, 65, 255, 256 spread unevenly, a dozen calls with the
    clock advancing, burst / created_at given and NULL; 257 is GUBER_E_BATCH_TOO_LARGE and moves nothing; every key's residency"""
    assert ms.scenario_a(gpu[0]) == len(ms.SIZES_A)


def test_b_ragged_empty_and_over_long_keys_and_ranks_of_different_key_limits(gpu):
    """b: widths 1, 8, 31, 32, 33, max_key_bytes, the empty key, an over-long one; `forwarded` as guber_mesh_eval_dev counts it on a twin
    world; a 40-byte key between a rank of 32 and a rank of 64 bytes"""
    ms.scenario_b(gpu[0])


def test_c_the_order_across_sources(gpu):
    """c: one hot token key from every rank turns OVER_LIMIT where source 0, 1, 2 in turn exhaust it; 256 requests of one key"""
    ms.scenario_c(gpu[0])


def test_d_a_share_that_falls_back_is_rerun_and_the_others_stand(gpu):
    """d: one key whose requests differ within a call: exactly one share goes through the general pipeline, the answers are the oracles'"""
    ms.scenario_d(gpu[0])


def test_e_wholesale_fall_back(gpu):
    """e: caches that may bind and a careful engine: no small launch, the oracles' answers; evictions as on a twin world"""
    ms.scenario_e(gpu[0])


def test_f_mixing_with_the_general_path(gpu):
    """f: guber_mesh_eval_small and guber_mesh_eval_dev alternate: one world of oracles, and the engines' statistics of a twin world"""
    ms.scenario_f(gpu[0])


def test_g_the_rule_is_the_devices(gpu):
    """g: hot keys pinned elsewhere, their buckets moved, guber_front_set_rule: a small call finds them there"""
    ms.scenario_g(gpu[0])


def test_h_global_requests_stay(gpu):
    """h: GLOBAL requests at their owner and at a non-owner, with and without a global_engine"""
    ms.scenario_h(gpu[0])


def test_i_one_rank_and_sixteen(gpu):
    """i: W = 1 equals a plain front; W = 16 of one engine each, 16 requests then 256, rings of both hashes"""
    ms.scenario_i(*gpu)
