"""The table-full answer and the long-key arena on the GPU (tests/table_full_cases.py), one test per case and pipeline: the two-launch
pipeline, the radix sequence, the careful round, the owner-partitioned pipeline, the two-launch one with the owner-partitioned switched off,
and the one-launch path of batches of at most 256 requests.  Nothing here is larger than 8 192 slots or 1 024 requests per batch.  What the
engine counted over case 3's batch X (retries, cache hits, misses, over the limit) must be the same on every pipeline: each test compares
its figures with those of the pipelines that ran before it."""
import pytest

import gubernator_amd as ga
import table_full_cases as tf

pytestmark = pytest.mark.gpu

PIPES = pytest.mark.parametrize("pipeline", tf.PIPELINES, ids=[p[0] for p in tf.PIPELINES])
_figures = {}


def factory(**kw):
    return ga.Engine(device=0, **kw)


@PIPES
def test_churn_of_long_keys_over_a_small_cache_is_never_refused(pipeline):
    tf.case_churn_over_a_small_cache(factory, pipeline)


@PIPES
def test_a_cache_holds_its_size_in_long_keys(pipeline):
    tf.case_a_caches_worth_of_long_keys(factory, pipeline)


@PIPES
def test_a_full_arena_refuses_every_request_of_a_new_long_key_until_a_rebuild(pipeline):
    _figures[pipeline[0]] = tf.case_the_arena_refuses(factory, pipeline, store_channel=pipeline[0] == "two_launch")
    assert len({tuple(sorted(f.items())) for f in _figures.values()}) == 1, f"batch X was counted differently by the pipelines: {_figures}"


@PIPES
def test_keys_past_the_probe_bound_are_refused_and_take_no_slot(pipeline):
    tf.case_the_probe_bound(factory, pipeline)


@PIPES
def test_a_chain_across_the_tables_end(pipeline):
    tf.case_a_chain_across_the_tables_end(factory, pipeline, move=pipeline[0] == "two_launch")
