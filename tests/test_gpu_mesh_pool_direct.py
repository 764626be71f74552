"""guber_wire_mesh_pool_set_direct on the GPU: the cases of tests/mesh_pool_direct_cases.py with every rank a logical rank of device 0.  A
lone small RPC is decoded by its caller's host transcoder, evaluated by guber_mesh_eval_small (k_mx_small: one launch per rank) and
marshalled by its caller; larger RPCs and RPCs that arrive while many calls are inside go through the stage sets as before.  The same
cases run on the CPU build of the engine in tests/test_mesh_pool_direct_cpu.py."""
import pytest

import gubernator_amd as ga
import mesh_pool_direct_cases as md
import support

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
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

    return lambda letter: md.run(letter, ga, support, new_engines, upload, lambda t: t.cpu().numpy())


@pytest.mark.parametrize("wrap", [0, 1])
def test_j_one_caller_walks_three_ranks_with_the_direct_path_on(run, wrap):
    """j: set_direct(4, 8): RPCs of 1, 2 and 4 items are served by their caller (stats.sets does not move), 5 items go through a set; local,
    forwarded, GLOBAL at and off its owner, every item error; every RPC's bytes against the oracles; sizes"""
    run("j%d" % wrap)


def test_k_refusals_with_the_path_on(run):
    """k: malformed, above max_per_rpc, a cap below the bound, len == 0: the codes of the path off, nothing evaluated"""
    run("k")


def test_l_direct_calls_and_sets_mix_under_concurrent_callers(run):
    """l: 16 threads, set_direct(4, 2): per-key conservation over all answers, both paths taken"""
    run("l")


def test_m_off_by_default_and_off_again(run):
    """m: nothing is served directly without set_direct; set_direct(0, 0) switches the path off again; one bucket whichever path"""
    run("m")
