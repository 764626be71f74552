"""bench.py's host-side pieces (no GPU): what `roofline.traffic` is made of, and what a plain run leaves out without changing the timed work."""
import importlib.util
import json
import os
import sys

from support import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("guber_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_roofline_traffic_is_the_mix_of_pipelines_the_profile_segment_ran():
    """a batch goes through ONE pipeline: the step's PMC traffic is every kernel's bytes per batch weighted by the batches it carried,
    over the batches that entered a pipeline — not the sum over every kernel that appeared (which counted a batch twice)"""
    b = _bench()
    tj = {"token": {"k_front": 20, "k_eval2": 10, "k_part": 8, "k_own": 9, "k_eval3": 7}, "token_fused": {"k_part": 6, "k_own": 7, "k_eval3": 5}}
    B = 65536
    # one table, claims only
    assert b.pipeline_traffic(tj, "token", ["k_front", "k_eval2"], {"k_front": 4, "k_eval2": 4}, {}, B) == 30
    # fused owner-partitioned launches of 4 batches each + a few single claims launches: (2 x 30 + 12 x 18) / 14
    launches = {"k_front": 2, "k_eval2": 2, "k_part_multi": 3, "k_own_multi": 3, "k_eval3_multi": 3}
    per_launch = {k: 4 * B for k in ("k_part_multi", "k_own_multi", "k_eval3_multi")}
    assert b.pipeline_traffic(tj, "token", list(launches), launches, per_launch, B) == int((2 * 30 + 12 * 18) / 14)
    # GUBER_FUSE_EP: k_part_multi once, then k_evalpart_multi (one group's k_eval3 + the next group's k_part) per round, k_eval3_multi last
    launches = {"k_part_multi": 1, "k_own_multi": 3, "k_evalpart_multi": 2, "k_eval3_multi": 1}
    assert b.pipeline_traffic(tj, "token", list(launches), launches, {k: 4 * B for k in launches}, B) == 18
    # a kernel the file does not know: no figure rather than a wrong one
    assert b.pipeline_traffic(tj, "token", ["k_front", "k_eval2", "k_other"], {"k_front": 1, "k_eval2": 1, "k_other": 1}, {}, B) is None
    # the committed file carries every kernel of both pipelines
    real = json.load(open(os.path.join(ROOT, "profiles", "roofline_traffic.json")))
    assert set(real["token"]) >= {"k_front", "k_eval2", "k_part", "k_own", "k_eval3"} and set(real["token_fused"]) >= {"k_part", "k_own", "k_eval3"}
    got = b.pipeline_traffic(real, "token", list(launches), launches, per_launch, B)
    assert 149 * B < got < 4 * 149 * B


def test_segments_after_the_timed_region_leave_the_timed_batches_alone():
    """a plain run draws no profile or latency segment, --full draws both after the timed batches: the warm-up and timed batches,
    their generations and their clocks must come out the same either way (the same answers, the same --dump-outputs)"""
    import numpy as np
    import torch
    b = _bench()
    # the routed headline: one stream, drawn in chunks from the canonical generator and ranked on the device (here: the CPU)
    full = b.ZipfRanker(torch, "cpu", 5000, seed=1234).draw_dev(7000, chunk=1024)
    plain = b.ZipfRanker(torch, "cpu", 5000, seed=1234).draw_dev(3000, chunk=1024)
    assert torch.equal(full[:3000], plain)
    # ... cut into generations segment by segment
    rig = b.RoutedRig.__new__(b.RoutedRig)
    rig.GB = 16
    for warm, steps in ((48, 2048), (48, 100), (16, 1)):
        rig.warmup, rig.steps, rig.profile_steps, rig.latency_steps = warm, steps, 4096, 1024
        with_segments = rig._generations(warm + steps + 4096 + 1024)
        rig.profile_steps = rig.latency_steps = 0
        without = rig._generations(warm + steps)
        assert with_segments[:len(without)] == without and with_segments[len(without)] == warm + steps
    # the pre-split arrangement: the first `total` batches in flush order do not depend on how far past them the stream was drawn
    S, B = 4, 64
    ids = torch.from_numpy(np.random.default_rng(5).integers(0, 1000, (60 + 2 * S + 2) * B).astype(np.int64))
    sown = torch.from_numpy((np.arange(1000) % S).astype(np.uint8))
    long_ids, long_sh = b.split_stream(torch, ids, sown, S, B, 60)
    short_ids, short_sh = b.split_stream(torch, ids[:(20 + 2 * S + 2) * B], sown, S, B, 20)
    assert torch.equal(long_ids[:20], short_ids) and long_sh[:20] == short_sh


def test_the_plain_run_is_the_default():
    b = _bench()
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"]
        assert b.parse().full is False
        sys.argv.append("--full")
        assert b.parse().full is True
    finally:
        sys.argv = argv
