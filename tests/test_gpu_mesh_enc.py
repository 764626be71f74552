"""guber_wire_dev_eval_mesh_enc on the GPU: the cases of tests/mesh_enc_cases.py with every rank a logical rank of device 0.  Serialized
GetRateLimitsReq payloads are decoded per rank, their items routed to the owning ranks by the ring (k_mx_count leaves the ring's owner per
item), evaluated there and answered where the payload arrived as serialized GetRateLimitsResp bytes written by k_wire_enc_owner, with
metadata{"owner": <address>} on every answer another rank owns; an RPC with an item error is the host transcoder's.  Every RPC's bytes equal
what the protobuf runtime writes for the per-rank oracles' answers, the host ring's owners and the texts of include/guber_wire.h.  The same
cases run on the CPU build of the engine in tests/test_mesh_enc_cpu.py."""
import pytest

import gubernator_amd as ga
import mesh_enc_cases as me
import support

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_world():
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

    return me.world_maker(ga, support, new_engines, upload, lambda t: t.cpu().numpy())


def test_a_sizes_around_the_encoders_piece_and_a_twin_world(make_world):
    """a: W = 3; RPCs of 0, 1, 3, 4, 5, 63, 64, 65, P - 1, P, P + 1, 2 P + 1 items mixed across ranks, a rank without a decoder, a decoder
    that decoded nothing, a dozen calls over one population; bytes per RPC, owner_rank, forwarded, sentinels; state equals eval_mesh's"""
    me.case_a(make_world)


def test_b_the_eight_address_lengths(make_world):
    """b: W = 8, addresses of 1, 11, 100, 118, 119, 127, 128, 264 bytes; bodies of 127 and 128 bytes; int64 limits 2^63 - 1 and -1"""
    me.case_b(make_world)


def test_c_every_class_of_item_in_one_rpc(make_world):
    """c: local, forwarded, GLOBAL at its owner and at a non-owner, empty unique_key, empty name, over-long key: the host's RPC; the same
    classes without the rejected items: the device's"""
    me.case_c(make_world)


def test_d_item_errors(make_world):
    """d: forwarded, local and GLOBAL-non-owner Gregorian-invalid items and a forwarded invalid algorithm, in RPCs of P + 1 and of 5 items;
    the other RPCs of the decode stay on the device"""
    me.case_d(make_world)


def test_e_a_malformed_payload_between_two_good_ones(make_world):
    """e: len 0 for the payload the decode turned away; its neighbours are right"""
    me.case_e(make_world)


def test_r_refusals_leave_the_engines_alone(make_world):
    """an empty, an over-long and a NULL address, a cap one below the bound, a peer RPC, two now_ms: refused, state and counters unchanged"""
    me.case_r(make_world)


def test_h_one_rank(make_world):
    """h: W = 1: owner_rank 0 or 0xFF, no metadata, an empty and an over-long key; state equals eval_mesh's"""
    me.case_h(make_world)


def test_the_piece_the_cases_stand_around_is_the_kernels():
    """the sizes P - 1 .. 2 P + 1 come from the library (WEO_P), and the static LDS figure of the design holds for it: 192 items of 315 bytes"""
    from gubernator_amd import wire as gw
    assert gw.mesh_enc_piece() == 192
