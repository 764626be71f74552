"""Engines created with FLAG_TEST_LAST_STAMPS (gubernator_amd/csrc/guber_test_flags.h): the next recency stamp starts 4 096 below 2^53, the end
of the 53 bits.  The call whose stamps would not fit renumbers the live items' stamps 1..live in their order first (k_lru_renumber) and goes on
from live + 1; every test puts that call where it wants it by arithmetic of its own and asserts through Engine.recency_info() that it happened
there (tests/stamp_end_cases.py has the cases and says what each one checks).  Every comparison is exact equality with the bounded-LRU
oracle.  The CPU twin is tests/test_stamp_end_cpu.py.

"Device" memory is torch's; against the CPU build of the engine (GUBER_HIP_LIB = tests/hostsim/libenginesim.so) it is numpy's."""
import numpy as np
import pytest

import gubernator_amd as ga
import stamp_end_cases as sec

pytestmark = pytest.mark.gpu

ON_CPU_ENGINE = "enginesim" in ga.LIB_PATH


class TorchDevice(sec.Device):
    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)

    def put(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        return t, t.data_ptr()

    def get(self, t):
        return t.cpu().numpy()

    def synchronize(self):
        self.torch.cuda.synchronize(self.dev)


def device():
    return sec.Device() if ON_CPU_ENGINE else TorchDevice()


def test_the_flag_and_its_start_value_are_the_headers():
    hv = sec.header_values()
    assert hv["GUBER_FLAG_TEST_LAST_STAMPS"] == sec.FLAG == ga.FLAG_TEST_LAST_STAMPS and hv["GUBER_TEST_LAST_SEQ_NEXT"] == sec.SEQ_NEXT == sec.END - 4096
    e = ga.Engine(cache_size=64, max_batch=256, flags=sec.FLAG | ga.FLAG_TEST_LATE_COUNTERS)       # with the epochs' flag this flag's stamp start wins
    assert e.recency_info() == {"next_stamp": sec.SEQ_NEXT, "renumbers": 0, "last_live": 0}
    e.close()


@pytest.mark.parametrize("flags", [f for f, _ in sec.PIPELINES], ids=[label for _, label in sec.PIPELINES])
def test_the_stamps_end_inside_a_small_binding_run_on_every_pipeline(flags):
    sec.case_pipeline(flags)


@pytest.mark.parametrize("one_call", [True, False], ids=["one_add_of_eleven", "item_by_item"])
def test_add_and_get_pick_the_reference_victims_across_the_end(one_call):
    sec.case_cache_sequence(one_call)


@pytest.mark.parametrize("remove", [False, True], ids=["get_item", "remove_item"])
def test_a_lookup_is_the_call_that_renumbers(remove):
    sec.case_lookup_triggers(remove)


def test_device_item_columns_are_the_call_that_renumbers():
    sec.case_add_items_dev(device())


def test_the_one_launch_path_renumbers_and_keeps_its_order():
    sec.case_one_launch()


def test_an_empty_table_starts_again_at_one():
    sec.case_empty_table()


def test_a_fused_group_lets_go_of_its_held_back_evaluation_to_renumber():
    sec.case_fused(device(), count_launches=ON_CPU_ENGINE)


def test_the_front_crosses_the_end_inside_one_call():
    sec.case_front(device())


def test_moved_in_buckets_keep_their_place_across_the_end():
    sec.case_moved_in()
