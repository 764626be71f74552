"""The Store side channel of the device front (guber_front_probe_missing_dev / guber_front_eval_store_dev) on a machine without a GPU:
tests/front_store.py's scenarios, at reduced sizes, against the engine compiled for the host (tests/hostsim/enginesim.cpp: host code and
kernels against fakehip), in processes of their own with GUBER_HIP_LIB pointing at that library and numpy arrays as device memory
(tests/front_store_cases.py).  What this covers beyond the GPU test: nothing — it is the same code, where every machine can run it."""
import os
import subprocess
import sys

import pytest

from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")
LIB = os.path.join(HS, "libenginesim.so")


@pytest.fixture(scope="module")
def enginesim():
    subprocess.run(["make", "-s", "-C", HS, "enginesim_lib"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    return LIB


def run_case(lib, case):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "front_store_cases.py"), case], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, GUBER_HIP_LIB=lib))
    assert p.returncode == 0 and f"FRONT STORE CASE OK {case}" in p.stdout, (p.stdout + p.stderr)[-3000:]
    return p.stdout


@pytest.mark.parametrize("case", ["parity1", "parity4", "parity6x3", "parity6x3_pieces"])
def test_store_generations_through_a_front_match_the_oracle(enginesim, case):
    """random generations with a write-through mock store on 1 and 4 engines of one stream (one pair of launches for all tables) and on 6
    engines over three streams (owner-partitioned; once with shares in pieces): answers, events and every key's call sequence equal ONE
    oracle's; the launch counts say that the new kernels and the intended pipeline ran"""
    run_case(enginesim, case)


@pytest.mark.parametrize("case", ["probes3", "probes1"])
def test_the_probe_at_its_edges_matches_the_model(enginesim, case):
    """sizes around the wave, the tile and two tiles, packed and ragged keys, every key resident / missing, one hot key, everything to the
    last engine, cuts at 1, at a tile's edge and at the last request, the refusals of guber_front_eval_store_dev"""
    run_case(enginesim, case)


def test_the_host_decides_when_keys_share_a_hash(enginesim):
    """engines created with FLAG_TEST_WEAK_HASH: distinct keys share election cells, the collision word goes up, and the list and the cut
    come from the keys themselves"""
    run_case(enginesim, "collisions")


def test_global_requests_are_a_key_of_their_own(enginesim):
    """a front whose rule names a global_engine: a key's Behavior_GLOBAL requests are asked for, resident and cut in the GLOBAL engine's table,
    apart from the key's other requests"""
    run_case(enginesim, "global_engine")
