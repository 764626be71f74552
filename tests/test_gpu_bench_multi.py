"""bench.py's N > 1 path, rehearsed on a box with ONE GPU (the driver's SCALE run is the first time it sees 2, 4, 8):

  * `python bench.py --gpus 2 ...` invoked PLAINLY (no WORLD_SIZE: the shape of the driver's 1-GPU command) re-executes itself under
    torch.distributed.run, one rank per "GPU" (--one-device: both ranks on GPU 0, --backend gloo for the timing collectives);
  * with --full, every rank digest-checks its own timed stream against its own oracle — the ranks own disjoint keys on the reference's ring
    (replicated_hash.go:104-119) — and rank 0 prints `parity: "2/2 ranks, K/K timed batches each"`, a cpu_baseline and the roofline
    object; a line without a parity verdict is refused;
  * the aggregate of two ranks that SHARE one GPU is compared with the N = 1 run of the same flags (they time-slice one device: the
    aggregate is about the N = 1 value, never a multiple of it);
  * --global-sync (BASELINE config 5) with two PROCESSES: guber_comm_create_rank + the product's ncclSend / ncclRecv sequence through
    the test-only librccl for ranks that share a GPU (tests/hostsim/fake_rccl.cpp), replicas converged or no line.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAKE = os.path.join(HERE, "hostsim", "libfake_rccl.so")
COMMON = ["--full", "--keys", "2000000", "--min-batches", "256", "--steps", "256", "--warmup", "8", "--extras", "", "--latency-steps", "0", "--profile-steps", "32",
          "--cpu-threads", "8", "--cpu-seconds", "1"]


def _bench(extra, env=None, timeout=900):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, timeout=timeout, env=e, cwd=ROOT)
    if p.returncode != 0:
        print(p.stdout[-3000:]); print(p.stderr[-8000:])
    assert p.returncode == 0, "bench.py failed (its output is printed above)"
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_two_ranks_on_one_device_are_parity_gated_and_agree_with_one_rank():
    one = _bench(["--gpus", "1"] + COMMON)
    assert one["n_gpus"] == 1 and one["parity"] and one["parity"] != "FAILED" and one["steps"] == 256 and one["steps_requested"] == 256
    two = _bench(["--gpus", "2", "--one-device", "--backend", "gloo"] + COMMON)
    assert two["n_gpus"] == 2 and two["scaling"] == "weak"
    assert two["parity"].startswith("2/2 ranks, 256/256 timed batches each"), two["parity"]
    assert two["parity_batches_by_rank"] == [256, 256]
    assert two["cpu_baseline"] and two["cpu_baseline"]["value"] > 0 and two["cpu_baseline"]["kind"] == "port"
    assert two["roofline"] and two["roofline"]["bound"] == "hbm" and 0 < two["roofline"]["frac"] < 1
    assert two["config"]["ranks_seen_by_the_collective_backend"] == 2
    res = two["config"]["resident_items_by_rank"]
    # (--keys is per GPU — weak scaling — and the ring splits the 2 x K keys nearly evenly: replicated_hash.go:78-119, 512 vnodes per peer)
    assert len(res) == 2 and sum(res) == 4_000_000 and all(abs(r - 2_000_000) < 150_000 for r in res), res
    ratio = two["value"] / one["value"]
    print(f"bench.py --gpus 2 on ONE device: {two['value'] / 1e9:.2f} G/s against {one['value'] / 1e9:.2f} G/s for --gpus 1 (ratio {ratio:.2f})")
    # two processes time-slicing one GPU: the aggregate stays in the neighbourhood of one process's rate (a multiple would mean the
    # ranks' work or the clock is counted wrongly; a collapse, that the ranks serialise on something that is not the GPU)
    assert 0.5 < ratio < 1.4, ratio


def test_two_of_eight_ring_peers_share_the_device():
    """BASELINE config 4's shape with the hardware at hand (bench.py's default `two_ranks` extra): a ring of EIGHT peers over 8 x keys,
    two of them as processes on this GPU — each owns what the ring gives gpu<rank> (about --keys each: replicated_hash.go:78-119), is
    gated against its own oracle, and the line says what every rank held and how many ranks the backend saw"""
    out = _bench(["--gpus", "2", "--one-device", "--backend", "gloo", "--ring-peers", "8"] + [("500000" if a == "2000000" else a) for a in COMMON])
    assert out["n_gpus"] == 2 and out["config"]["ring_peers"] == 8
    assert out["parity"].startswith("2/2 ranks, 256/256 timed batches each"), out["parity"]
    assert out["config"]["ranks_seen_by_the_collective_backend"] == 2
    res = out["config"]["resident_items_by_rank"]
    assert len(res) == 2 and all(abs(r - 500_000) < 75_000 for r in res), res      # (two eighths of 4 M keys, +- the ring's imbalance)


def test_global_leg_with_two_processes_through_the_rccl_call_sequence():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "hostsim"), "fake_rccl"], check=True)
    out = _bench(["--gpus", "2", "--one-device", "--backend", "gloo", "--global-sync", "8", "--keys", "200000", "--steps", "32", "--warmup", "8"],
                 env={"GUBER_RCCL_LIB": FAKE})
    assert out["n_gpus"] == 2 and out["global_sync"]["replicas_converged"] is True and out["global_sync"]["host_fallbacks"] == 0
    assert out["parity"].startswith("2/2 ranks"), out["parity"]
    assert out["global_sync"]["syncs"] >= 4 and out["global_sync"]["avg_hits_rows_sent"] > 0 and out["value"] > 0
    # the same flags as two logical ranks of ONE process (device copies instead of the RCCL calls): the streams are seeded, so the replicas
    # end in the same state — the probe's answers add up to the same number.  (Converging is not enough: with wrong is_owner flags — a
    # race in bench.py's setup that two processes sharing a GPU lost in 4 runs of 10 — the replicas sometimes agreed on a wrong state.)
    one = _bench(["--gpus", "1", "--global-sync", "8", "--keys", "200000", "--steps", "32", "--warmup", "8"])
    assert one["global_sync"]["replicas_converged"] is True
    assert out["global_sync"]["probe_remaining_sum"] == one["global_sync"]["probe_remaining_sum"], (out["global_sync"], one["global_sync"])
