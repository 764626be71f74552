"""guber_wire_mesh_pool_* on the GPU: the cases of tests/mesh_pool_cases.py with every rank a logical rank of device 0.  Caller threads hand
serialized GetRateLimitsReq bytes to any rank of a mesh and get serialized GetRateLimitsResp bytes back; decode (k_wire_*), the ring's owner
decision (k_mx_count<true> / k_mx_scan / k_mx_pack<true>), the evaluation on the owners' fronts, the answers' order (k_mx_apack / k_mx_out) and
the marshalling (k_wire_enc_owner) run on the device, for the first time under concurrent callers.  The same cases run on the CPU build of the
engine in tests/test_mesh_pool_cpu.py."""
import os
import subprocess

import pytest

import gubernator_amd as ga
import mesh_pool_cases as mp
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

    return lambda letter: mp.run(letter, ga, support, new_engines, upload, lambda t: t.cpu().numpy())


def test_a_one_caller_walks_three_ranks_with_every_class_of_item(run):
    """a: 60 RPCs of 0, 1, 3, P - 1, P, P + 1, 2 P + 1 and 1 000 items round robin over three ranks and a frozen clock that advances; local,
    forwarded, GLOBAL at and off its owner, rejected and error items; every RPC's bytes against the oracles; sets, host_rpcs, sizes"""
    run("a")


def test_b_the_golden_functional_scenarios_alternating_two_ranks(run):
    """b: tests/golden/functional_vectors.json through the pool at W = 2"""
    run("b")


@pytest.mark.parametrize("letter", ["c12", "c24"])
def test_c_concurrent_callers_share_sets_and_every_hit_is_applied_exactly_once(run, letter):
    """c: 12 callers and three sets, 24 callers and two, at W = 3: per-key conservation over all answers, the callers' own keys, the owner's
    address exactly where another rank owns the key, two callers turned away whole, sets < rpcs, items exact"""
    run(letter)


def test_d_stage_limits(run):
    """d: a stage of 2 048 items under 1 000-item RPCs (sealed_full), two RPCs per stage, a payload no stage can hold"""
    run("d")


def test_e_refusals_leave_everything_alone(run):
    """e: a short cap, rank = W, NULL arguments, bad addresses, max_items above the mesh's max_n, a call after close; cap = the bound"""
    run("e")


def test_f_one_rank_equals_the_one_device_pool(run):
    """f, W = 1: no metadata, guber_wire_pool's bytes"""
    run("f1")


def test_f_eight_ranks_of_which_two_receive_nothing(run):
    """f, W = 8: callers at ranks 0 - 5; ranks 6 and 7 own and answer keys"""
    run("f8")


def test_the_go_handlers_call_sequence_in_plain_c(tmp_path):
    """tests/hostsim/mesh_pool_abi_c99.c — the calls go/wire_server.go's getRateLimitsMeshRaw makes (and the set-up around them), compiled as
    C99 against the two public headers — on the GPU, the response bytes checked"""
    exe = str(tmp_path / "mesh_pool_abi_c99")
    libdir = os.path.join(support.ROOT, "gubernator_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(support.ROOT, "include"), "-o", exe,
                    os.path.join(support.ROOT, "tests", "hostsim", "mesh_pool_abi_c99.c"), "-L", libdir, "-lguber_hip", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MESH POOL ABI C99 OK" in r.stdout, (r.returncode, r.stdout, r.stderr)
