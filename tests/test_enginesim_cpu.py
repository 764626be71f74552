"""The ENGINE on a machine without a GPU: gubernator_amd/csrc/guber_engine.hip — host code and kernels — compiled for the host against
tests/hostsim/fakehip (the kernel language as cooperative fibers, the HIP runtime API as a stand-in whose launches run at once:
tests/hostsim/enginesim.cpp), driven through the C ABI exactly as the GPU suite drives the product library, against the oracle.
What this covers that tests/test_kernels_devsim.py cannot: the engine's HOST logic — launch groups of several tables, preludes and
maintenance, the eviction pre-pass around fused groups, and GUBER_FUSE_EP's held-back k_eval3 (launch_group / PendSet), which no GPU
has run yet.  Test infrastructure only: the cases run in processes of their own with GUBER_HIP_LIB pointing at the test library; the
product library is hipcc's, needs a device and has no CPU path (test_abi_cpu.py checks that it fails loudly without one).  The test library runs under AddressSanitizer."""
import os
import subprocess
import sys

import pytest

from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")
LIB = os.path.join(HS, "libenginesim_san.so")


@pytest.fixture(scope="module")
def enginesim():
    """the library under AddressSanitizer (make enginesim_lib builds it without, for a debugger): every "device" buffer is a host
    allocation here, so a KERNEL that reads or writes outside a table, a work array or a caller's column is reported, like the host code"""
    subprocess.run(["make", "-s", "-C", HS, "enginesim_san_lib"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    return LIB


def _runtime(name):
    return subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True, check=True).stdout.strip()


def run_case(lib, case, **env):
    san = dict(LD_PRELOAD=_runtime("libasan.so"), ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "enginesim_cases.py"), case], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, GUBER_HIP_LIB=lib, **san, **env))
    assert p.returncode == 0 and f"ENGINESIM CASE OK {case}" in p.stdout, (p.stdout + p.stderr)[-3000:]
    return p.stdout


@pytest.mark.parametrize("case", ["single_default", "single_part"])
def test_one_engine_through_the_host_pointer_entry(enginesim, case):
    """guber_eval_batch: stage, copies, the pipeline's launches, copies back — adversarial batches, counters"""
    run_case(enginesim, case)


@pytest.mark.parametrize("case,fuse_ep", [("routed4", "0"), ("routed4", "1"), ("routed6", "1")], ids=["4_tables-three_launches", "4_tables-fuse_ep", "6_tables-fuse_ep"])
def test_routed_batches_of_several_tables(enginesim, case, fuse_ep):
    """guber_eval_batches_routed_dev on four tables (one group per round) and six (two groups per round) of one stream: the default three
    launches per pass, and GUBER_FUSE_EP=1 — k_eval3 held back and launched with the same tables' next k_part (k_evalpart_multi), on
    its own when a group changes, takes the other pipeline, or the call ends; the launch counts say which path ran"""
    out = run_case(enginesim, case, GUBER_FUSE_EP=fuse_ep)
    assert ("k_evalpart_multi" in out) == (fuse_ep == "1"), out[-500:]


@pytest.mark.parametrize("fuse_ep", ["0", "1"], ids=["three_launches", "fuse_ep"])
def test_fused_groups_around_a_cache_that_binds(enginesim, fuse_ep):
    """batches that may overflow their table's cache leave the groups for the eviction pre-pass; answers equal the bounded-LRU oracle's"""
    run_case(enginesim, "routed_lru", GUBER_FUSE_EP=fuse_ep)



@pytest.mark.parametrize("case,fuse_ep,one_pair", [("front4", "1", "0"), ("front4", "1", None), ("front6x3_pieces", "0", None), ("front1", "1", None)],
                         ids=["front4-owner_partitioned", "front4-one_pair_of_launches", "front6x3_pieces", "front1"])
def test_a_front_routes_generations_on_the_device_and_answers_in_arrival_order(enginesim, case, fuse_ep, one_pair):
    """guber_front_eval_dev (guber_front.h, guber_kernels_front.h): ONE stream of requests in arrival order -> k_fr_count / k_fr_scatter
    (XXH64 + the placement's rule, workers.go:180-184) -> the engines' shares through the fused launches, on one, two and three streams,
    shares larger than an engine's max_batch in pieces, the k_eval3 of a generation held back for the next one's k_part (and the event the
    answers' way home waits for recorded behind whoever launches it) -> k_fr_out: every generation equals ONE oracle fed the generations
    in order (gubernator.go:203: a serial loop in request order), keys of one width and ragged ones, empty and tiny generations.
    Four tables of ONE stream twice: through the owner-partitioned pipeline in one group (the laboratory knob GUBER_FRONT_ONE_PAIR_MAX=0) and
    the way the product takes generations of that size — all tables in ONE pair of launches (launch_group_mem: k_front_multi_mem /
    k_eval2_multi_mem, the argument blocks through device memory)"""
    env = dict(GUBER_FUSE_EP=fuse_ep)
    if one_pair is not None:
        env["GUBER_FRONT_ONE_PAIR_MAX"] = one_pair
    run_case(enginesim, case, **env)


def test_a_front_at_key_width_tile_and_sixteen_engine_edges(enginesim):
    """tests/front_edges.py's scenarios a - d (packed key widths 1 .. 32 and single widths above, sizes around the thread stride and the
    tile, one odd / empty / over-long key in a generation of one width, skew, GLOBAL) on fronts of 16 and of 3 engines: answers, the
    engine every key is resident in, the host's hash against a plain-Python XXH64, sentinels behind the results.  The key buffers end
    exactly the 8 bytes behind their last key that include/guber_gpu.h promises: a kernel that reads further is AddressSanitizer's report"""
    run_case(enginesim, "front_edges")


def test_groups_of_stages_take_one_pair_of_launches(enginesim):
    """guber_stages_submit with aggregates off (tests/stage_groups_check.py): one stage, three and six of engines that share a stream, twice —
    every answer the oracle's, and the profile says which form each group took: k_front / k_eval2 for one stage, k_front_multi /
    k_eval2_multi for three (arguments by value) and for six (arguments through device memory), exactly one pair per group"""
    out = run_case(enginesim, "stage_groups")
    assert "launches {'k_front': 2, 'k_eval2': 2, 'k_front_multi': 4, 'k_eval2_multi': 4}" in out, out[-500:]


def test_a_front_sends_global_requests_to_the_global_engine(enginesim):
    """guber_route_rule_t.global_engine: Behavior_GLOBAL requests go to the device's GLOBAL engine, the rest by the placement"""
    run_case(enginesim, "front_global")


def test_the_front_over_binding_caches_is_the_references_worker_pool(enginesim):
    """three engines with CacheSize / 3 items each behind a front whose placement is the untouched worker rule == the oracle with three
    workers (workers.go:125-151,180-184): device routing, per-table eviction pre-passes, requests that change a list's length"""
    run_case(enginesim, "front_lru3", GUBER_FUSE_EP="1")


def test_the_benchs_own_sequence_under_the_address_sanitizer(enginesim):
    """bench.py in small on the CPU engine: residency pass, a pre-split stretch through guber_eval_batches_routed_dev, then the routed
    headline's guber_front_eval_dev calls, twelve engines over three streams — AddressSanitizer watches every kernel and copy (VERDICT r05
    item 2: the one GPU memory access fault of round 5 was never reproduced; this is the sequence it happened in)"""
    run_case(enginesim, "bench_sequence", GUBER_FUSE_EP="1")


def test_another_thread_on_tables_whose_evaluation_is_held_back(enginesim):
    """GUBER_FUSE_EP: while one routed call holds k_eval3 launches back, a second thread calls guber_size / guber_get_item on two of its
    tables — it launches what is held back for them before it looks (guber_engine::held), the call's answers stay the oracle's"""
    run_case(enginesim, "routed_threads", GUBER_FUSE_EP="1")


def test_the_gpu_suites_host_layer_and_wire_files_against_the_cpu_engine(enginesim):
    """tests/test_gpu_host_layer.py, tests/test_gpu_wire_dev.py and tests/test_gpu_wire_pool.py — the `-m gpu` tests of the pool on real
    engines (stages, routed stages, placement passes moving buckets, Store / Loader, GLOBAL engines, zones), of the wire front end, of the
    device wire decoder and of the payload stage (caller threads, the pool's two threads, the front) — run unchanged in a process of their
    own against the CPU build of the engine, under AddressSanitizer.  (The plain-C replica of the Go
    binding links the product library itself and stays a GPU test.)"""
    san = dict(LD_PRELOAD=_runtime("libasan.so"), ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_host_layer.py"), os.path.join(ROOT, "tests", "test_gpu_wire_dev.py"),
                        os.path.join(ROOT, "tests", "test_gpu_wire_pool.py"), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k", "not plain_c"], capture_output=True, text=True, timeout=2400, cwd=ROOT,
                       env=dict(os.environ, GUBER_HIP_LIB=enginesim, **san))
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0 and " passed" in p.stdout and "failed" not in p.stdout, tail
