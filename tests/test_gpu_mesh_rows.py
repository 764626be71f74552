"""Key rows through the mesh of fronts on the GPU — guber_mesh_eval_rows_dev (k_mx_count<true> / k_mx_pack<true>,
gubernator_amd/csrc/guber_kernels_mesh.h) and guber_wire_dev_eval_mesh on top of it: the cases of tests/mesh_rows_cases.py with every rank a
logical rank of device 0.  Serialized RPC payloads are decoded on the device per rank, their items routed to the owning ranks by the ring,
evaluated there in source order and answered where their payload arrived; every answer equals ONE oracle per rank fed what the order rule
says, the forwarded counts equal the host ring's, every key is resident in exactly the engine of exactly the rank the ring and the
placement name, and rows give what packed keys give.  All cases but the sixteen ranks also run on the CPU build of the engine
(tests/test_mesh_rows_cpu.py)."""
import numpy as np
import pytest

import gubernator_amd as ga
import mesh_cases as mc
import mesh_rows_cases as mr
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
        return mr.RowsWorld(ga, support, new_engines=new_engines, upload=upload, download=lambda t: t.cpu().numpy(), **kw)

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
    return make_world, plain_front, mr.wire_front_of(ga, new_engines)


def test_a_wire_sizes_around_the_tile_mixed_across_ranks_and_residency(gpu):
    """a: payloads of 0, 1, 63, 64, 65, 1 023, 1 024, 1 025 and 2 049 items mixed across three ranks, a rank without a decoder, all ranks but
    one empty; a dozen calls over one population, buckets run out; forwarded counts, every pair of ranks, every key's residency"""
    mr.case_a(gpu[0])


def test_b_wire_key_widths_at_both_strides(gpu):
    """b: stride 24 (no speculative read) widths 3, 8, 15, 16; stride 72 widths 3, 8, 24, 31, 32, 33, 64; a ragged run and a mixed call at
    each; an item with an empty unique_key per generation: error 4, in its place, not forwarded"""
    mr.case_b(gpu[0])


def test_c_wire_the_order_across_sources(gpu):
    """c: one hot token key in a payload at every rank turns OVER_LIMIT exactly where source 0, 1, 2 in turn exhaust it"""
    mr.case_c(gpu[0])


def test_d_wire_global_items_stay_on_their_arrival_rank(gpu):
    """d: W = 2, half of the items Behavior_GLOBAL: none forwarded, resident in the arrival rank's GLOBAL engine, is_owner from the ring"""
    mr.case_d(gpu[0])


def test_e_wire_an_inflow_larger_than_the_fronts_max_n(gpu):
    """e: W = 4, every rank's payloads hold 2 049 items rank 2 owns: its front takes 8 196 items as generations of at most 2 049"""
    mr.case_e(gpu[0])


def test_r_wire_refusals_leave_the_engines_alone(gpu):
    """a GUBER_WIRE_RPC_PEER payload, two now_ms, a decoder twice, n_items above the mesh's max_n: refused, sizes and counts unchanged"""
    mr.case_r(gpu[0])


def test_f_rows_equal_packed(gpu):
    """f: two identical worlds, the same generations packed and in rows of stride 48 with 0xA5 behind every key, the last row ending at its
    allocation's end: answers, forwarded counts and residency element-wise equal; an empty and an over-long key per generation stay"""
    mr.case_f(gpu[0])


def test_g_mixed_forms_in_one_call(gpu):
    """g: packed, rows of stride 48 and rows of stride 24 in one call over engines of max_key_bytes 16, moving on from call to call"""
    mr.case_g(gpu[0])


def test_h_one_rank_is_the_front_alone(gpu):
    """h: W = 1 in rows equals a plain front; through the wire it equals guber_wire_dev_eval_front fed the same payloads"""
    mr.case_h(*gpu)


def test_h16_sixteen_ranks_in_rows(gpu):
    """sixteen ranks of one engine each, 1 025 rows per rank (a ring of 64 KB: searched in global memory)"""
    mr.case_h16(gpu[0])
