"""A front that observes its own traffic and runs placement passes (guber_front_observe / guber_front_observation / guber_front_rebalance)
on a machine without a GPU: tests/front_placement_cases.py against the engine compiled for the host
(tests/hostsim/enginesim.cpp: host code and kernels against fakehip), in processes of their own with GUBER_HIP_LIB pointing at that
library and numpy arrays as device memory.  The placement's feed and the argument checks need no device at all and run in this process,
against the product library."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import gubernator_amd as ga
from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")
LIB = os.path.join(HS, "libenginesim.so")


@pytest.fixture(scope="module")
def enginesim():
    subprocess.run(["make", "-s", "-C", HS, "enginesim_lib"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    return LIB


def run_case(lib, case):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "front_placement_cases.py"), case], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, GUBER_HIP_LIB=lib))
    assert p.returncode == 0 and f"FRONT PLACEMENT CASE OK {case}" in p.stdout, (p.stdout + p.stderr)[-3000:]
    return p.stdout


@pytest.mark.parametrize("case", ["counts4", "counts16"])
def test_a_window_holds_exactly_what_numpy_counts(enginesim, case):
    """a: every = 1 on 4 and on 16 engines; generations of 1 .. 4 097 requests of one width, ragged and above 32 bytes, packed and in key rows 16
    and 40 bytes apart with non-zero padding; one key that is half of
    40 000 requests; a window over three generations; the window after one is empty.  slot_w element-wise, observed + skipped == n,
    dropped == 0, every key at or above the bar once with its count"""
    run_case(enginesim, case)


def test_what_the_rule_does_not_hash_is_not_observed(enginesim):
    """b: GLOBAL requests under a rule with a global_engine, empty keys, over-long keys: skipped, answered as ever; GLOBAL requests under a
    rule without one are observed"""
    run_case(enginesim, "not_observed")


def test_off_means_untouched(enginesim):
    """c: the launch counters of a front that never observed, and of one that turned it off, show none of the new kernels; every = 4: two of eight"""
    run_case(enginesim, "off")


def test_a_pass_moves_hot_buckets_and_pins_age(enginesim):
    """d, e: three hot keys behind engine 0: a pass moves at least two away, buckets and all; engine 0's share falls; three passes without
    them take the pins back and move the buckets home; every answer equals the oracle's"""
    run_case(enginesim, "pass_and_aging")


def test_a_refused_move_is_cancelled(enginesim):
    """f: destinations whose long-key arena is full give the bucket back: the pass cancels, the key follows its slot, answers stay exact"""
    run_case(enginesim, "refused_move")


@pytest.mark.parametrize("case", ["in_flight_3_streams", "in_flight_1_stream"])
def test_a_pass_between_calls_of_three_generations(enginesim, case):
    """g: depth 3, three generations per call, a pass in between — shares in pieces over three streams, one pair of launches over one —
    and a pass right after a probe nobody evaluated"""
    run_case(enginesim, case)


def test_a_pass_under_a_mesh(enginesim):
    """h: W = 2, two engines per rank: rank 0's front is rebalanced between mesh calls, a one-launch call follows"""
    run_case(enginesim, "mesh")


def test_refusals_with_engines(enginesim):
    """j: a one-engine front, a placement of another shape, a window that was never turned on"""
    run_case(enginesim, "refusals")


def test_the_placement_takes_a_window_as_it_takes_single_observations():
    """i: observe_aggregate against observe called `count` times per key: the same pins and the same moves, twice; a wrong n_slots"""
    import front_placement_cases as fp
    fp.placement_feed()


def test_argument_checks_need_no_device():
    """j: NULL arguments are refused before HIP is touched"""
    L = ga.lib()
    L.guber_front_observe.argtypes = [C.c_void_p, C.c_uint32]
    L.guber_front_observation.argtypes = [C.c_void_p, C.c_void_p]
    L.guber_front_rebalance.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    L.guber_placement_observe_aggregate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
    obs, st = ga.FrontObservation(), ga.FrontRebalanceStats()
    place = ga.Placement(4)
    E = ga.E_INVALID_ARG
    assert L.guber_front_observe(None, 1) == E and L.guber_front_observe(None, 0) == E
    assert L.guber_front_observation(None, C.byref(obs)) == E
    assert L.guber_front_rebalance(None, place.h, 0.125, C.byref(st)) == E
    assert L.guber_placement_observe_aggregate(None, None, 0, None, None, 0) == E
    assert L.guber_placement_observe_aggregate(place.h, None, place.n_slots(), None, None, 0) == E
    sw = (C.c_uint32 * place.n_slots())()
    assert L.guber_placement_observe_aggregate(place.h, sw, place.n_slots(), None, None, 1) == E
    assert L.guber_placement_observe_aggregate(place.h, sw, place.n_slots() - 1, None, None, 0) == E
    assert L.guber_placement_observe_aggregate(place.h, sw, place.n_slots(), None, None, 0) == 0
    place.close()


def test_struct_twins_match_the_header():
    assert C.sizeof(ga.FrontObservation) == 4 * 8 + 2 * 4 + 8 + 8 + 8 + 8 + 8 and C.sizeof(ga.FrontRebalanceStats) == 2 * 8 + 4 * 4
