#!/usr/bin/env python
"""Groups of stages through guber_stages_submit (gubernator_amd/csrc/engine_stages.inl): which form of the two-launch pipeline a group
of 1, 3 and 6 stages takes, and that every answer is the oracle's.  Run as the case `stage_groups` of tests/enginesim_cases.py against
the CPU build of the engine, by tests/test_gpu_host_layer.py::test_groups_of_stages_take_one_pair_of_launches in a process of its own
against the product library, or by hand:
  python tests/stage_groups_check.py
Six engines on ONE stream with per-kernel timing on, a stage each, aggregates off.  A batch is 300 requests (above the 256 of the
one-launch small path: two tiles) over 220 keys, so some keys come more than once.  One stage, then three, then six (a stage per
engine) — twice, the second pass on resident keys.  One stage goes as k_front / k_eval2, three as k_front_multi / k_eval2_multi with
the argument blocks by value, six with the argument blocks through device memory (k_front_multi_mem / k_eval2_multi_mem, timed under
the same names)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import numpy as np

import gubernator_amd as ga
import streams
import support

WANT = {"k_front": 2, "k_eval2": 2, "k_front_multi": 4, "k_eval2_multi": 4}


def main():
    NE, K, N = 6, 220, 300
    tab = streams.key_table(K * NE)
    e0 = ga.Engine(cache_size=1 << 16, max_batch=4096)
    engs = [e0] + [ga.Engine(cache_size=1 << 16, max_batch=4096, stream=e0.stream_handle()) for _ in range(NE - 1)]
    orcs = [support.Oracle(cache_size=1 << 16) for _ in range(NE)]
    stages = [ga.Stage(e, 1024) for e in engs]
    for e in engs:
        e.profile(True)
    rng = np.random.default_rng(11)
    step = 0
    for rnd in range(2):
        for g in (1, 3, 6):
            hbs = []
            for j in range(g):
                hb = streams.bench_batch(tab, j * K + rng.integers(0, K, N), streams.NOW0 + step * 700, algorithm=(step + j) % 2, limit=4, duration=3000)
                assert len(np.unique(hb.key_off)) == N + 1 and len({bytes(hb.key_bytes[hb.key_off[i]:hb.key_off[i + 1]]) for i in range(N)}) < N   # duplicate keys
                stages[j].fill(hb)
                hbs.append(hb)
            assert ga.Stage.submit_many(stages[:g], aggregates=False) == g
            for j in range(g):
                stages[j].wait()
                support.assert_results_equal(stages[j].result(), orcs[j].eval(hbs[j]), f"pass {rnd}, group of {g}, table {j}")
            step += 1
    launches = {}
    for e in engs:
        for k, v in e.profile_read().items():
            launches[k] = launches.get(k, 0) + v[0]
    launches = {k: v for k, v in launches.items() if v}
    print("launches", launches)
    assert launches == WANT, (launches, WANT)
    for j, (e, o) in enumerate(zip(engs, orcs)):
        assert e.size() == o.size(), (j, e.size(), o.size())
    for s in stages:
        s.close()
    for e in reversed(engs):
        e.close()


if __name__ == "__main__":
    main()
    print("STAGE GROUPS CHECK OK")
