"""The cache operations on the GPU (tests/cache_ops_cases.py), one test per case on the product library: Add, Get, Remove, Each, the dump's
buffer protocol, a restart through dump and load, device item columns and moves between tables, at sizes where k_items_probe / k_items_commit
and k_items_take_by_hash / k_items_restore run more than one workgroup — what the CPU build, whose launches run a workgroup at a time,
cannot see.  Everything is compared bit-exactly with the oracle; nothing here is larger than 8 192 items."""
import pytest

import cache_ops_cases as co
import gubernator_amd as ga

pytestmark = pytest.mark.gpu


def factory(**kw):
    return ga.Engine(device=0, **kw)


@pytest.fixture(scope="module")
def columns():
    import torch
    dev = torch.device("cuda", 0)

    def upload(a):
        t = torch.from_numpy(a).to(dev)
        torch.cuda.synchronize(dev)
        return t, t.data_ptr()
    return upload, lambda t: t.cpu().numpy()


def test_a_add_across_workgroups():
    co.case_add_across_workgroups(factory)


def test_b_add_with_duplicates_under_colliding_tags():
    co.case_add_with_duplicates_under_colliding_tags(factory)


def test_c_a_binding_cache_a_small_table_and_the_rebuild():
    co.case_a_binding_cache_and_the_rebuild(factory)


def test_d_an_add_larger_than_the_cache():
    co.case_an_add_larger_than_the_cache(factory)


def test_e_extreme_fields():
    co.case_extreme_fields(factory)


def test_f_the_dump_protocol():
    co.case_the_dump_protocol(factory)


@pytest.mark.parametrize("compact_first", [False, True], ids=["as_it_is", "after_a_compact"])
def test_g_restart_through_dump_and_load(compact_first):
    co.case_restart(factory, compact_first)


def test_h_device_columns(columns):
    co.case_device_columns(factory, *columns)


@pytest.mark.parametrize("list_len", co.LIST_LENS, ids=[str(n or "all") for n in co.LIST_LENS])
def test_i_moves_into_a_table_with_shorter_keys(list_len):
    co.case_moves(factory, list_len)


def test_i_a_move_of_keys_too_long_to_stage():
    co.case_a_move_of_keys_too_long_to_stage(factory)


def test_i_a_move_into_a_table_without_room():
    co.case_a_move_into_a_table_without_room(factory)
