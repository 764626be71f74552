#!/usr/bin/env python3
"""First numbers for a front that observes its own traffic and runs placement passes (guber_front_observe / guber_front_rebalance):
writes profiles/front_observe_first_numbers.txt.  Needs a GPU; every section runs in a child process of its own, one after the other.

    python tools/front_observe_numbers.py [--resource-usage FILE] [--out FILE]     every section, then the report
    python tools/front_observe_numbers.py kernel | kernel_no_agg | sampling | passes  one section: prints its NUM lines

  kernel     k_fr_observe beside k_fr_count (guber_profile_read, microseconds per launch) for Zipf-1.1 and uniform generations of 65 536 and
             1 048 576 requests on a 12-table front; kernel_no_agg: the Zipf generations again on the laboratory build with the per-tile
             aggregation switched off (GUBER_FRONT_OBSERVE_NO_AGG)
  sampling   the routed rate of a 12-table front with every = 16 against every = 0, alternating runs in one process; the margin is the
             spread of the every = 0 runs
  passes     a 12-table front with the default rule on a Zipf-1.1 stream: largest share / mean share of the engines and the routed rate
             before any pass, after one and after three; the same front under a placement fitted offline the way bench.py fits it
--resource-usage: the output of hipcc -Rpass-analysis=kernel-resource-usage for guber_engine.hip; its k_fr_* kernels are quoted."""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAB = os.path.join(ROOT, "gubernator_amd", "libguber_hip_lab.so")
S, KEYS, W = 12, 1_000_000, 16
G_BIG = 1 << 20


def num(**kw):
    print("NUM " + json.dumps(kw), flush=True)


class World:
    def __init__(self, fitted=False, max_n=G_BIG):
        import torch
        import gubernator_amd as ga
        from bench import ZipfRanker
        self.torch, self.ga, self.ZipfRanker = torch, ga, ZipfRanker
        self.dev = torch.device("cuda", 0)
        rng = np.random.default_rng(5)
        self.table = rng.integers(33, 127, (KEYS, W), dtype=np.uint8)
        self.d_table = torch.from_numpy(self.table).to(self.dev)
        self.place = ga.Placement(S)
        if fitted:                                    # bench.py's offline fit: 2 M sampled requests of the same distribution, another seed
            ids = ZipfRanker(torch, self.dev, KEYS, s=1.1, seed=990_001, perm_seed=99).draw_dev(1 << 21).cpu().numpy()
            off = (np.arange(len(ids) + 1, dtype=np.int64) * W).astype(np.uint32)
            self.place.observe_keys(np.ascontiguousarray(self.table[ids]).reshape(-1), off)
            self.place.rebalance(0.125, True)
        self.strs = [torch.cuda.Stream(device=self.dev) for _ in range(3)]
        self.engs = [ga.Engine(cache_size=KEYS, max_batch=65536, stream=self.strs[j * 3 // S].cuda_stream) for j in range(S)]
        self.front = ga.Front(self.engs, self.place, max_n=max_n, depth=4)
        self.now = 1_700_000_000_000

    def stream(self, dist, G, ngen, seed):
        """ngen generations of G requests -> (GuberBatch array, GuberResult array, keep-alive)"""
        torch, ga, dev = self.torch, self.ga, self.dev
        n = G * ngen
        if dist == "zipf":
            ids = self.ZipfRanker(torch, dev, KEYS, s=1.1, seed=seed, perm_seed=99).draw_dev(n).long()
        else:
            ids = torch.from_numpy(np.random.default_rng(seed).integers(0, KEYS, n)).to(dev)
        keys = torch.zeros(n * W + 16, dtype=torch.uint8, device=dev)
        keys[:n * W] = self.d_table.index_select(0, ids).reshape(-1)
        off = torch.from_numpy((np.arange(G + 1, dtype=np.int64) * W).astype(np.int32)).to(dev)
        c = dict(hits=torch.ones(G, dtype=torch.int64, device=dev), limit=torch.full((G,), 100, dtype=torch.int64, device=dev),
                 duration=torch.full((G,), 60_000, dtype=torch.int64, device=dev), algorithm=torch.zeros(G, dtype=torch.uint8, device=dev),
                 behavior=torch.zeros(G, dtype=torch.int32, device=dev))
        r = dict(status=torch.empty(n, dtype=torch.uint8, device=dev), err=torch.empty(n, dtype=torch.uint8, device=dev), limit=torch.empty(n, dtype=torch.int64, device=dev),
                 remaining=torch.empty(n, dtype=torch.int64, device=dev), reset_time=torch.empty(n, dtype=torch.int64, device=dev))
        B, R = (ga.GuberBatch * ngen)(), (ga.GuberResult * ngen)()
        for g in range(ngen):
            self.now += 16
            B[g] = ga.GuberBatch(G, 0, keys.data_ptr() + g * G * W, off.data_ptr(), c["hits"].data_ptr(), c["limit"].data_ptr(), c["duration"].data_ptr(), None, None,
                                 c["algorithm"].data_ptr(), c["behavior"].data_ptr(), None, None, None, self.now)
            R[g] = ga.GuberResult(r["status"].data_ptr() + g * G, r["limit"].data_ptr() + g * G * 8, r["remaining"].data_ptr() + g * G * 8,
                                  r["reset_time"].data_ptr() + g * G * 8, r["err"].data_ptr() + g * G, 0, 0, 0, 0, 0)
        torch.cuda.synchronize(dev)
        return B, R, ngen, G, (keys, off, c, r)

    def run(self, st):
        B, R, ngen, G, _ = st
        self.torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        assert self.front.eval_dev(B, R, ngen) == ngen
        self.front.synchronize()
        return ngen * G / (time.perf_counter() - t0)

    def handled(self):
        out = []
        for e in self.engs:
            s = e.stats()
            out.append(s["cache_hits"] + s["cache_misses"])
        return np.array(out, np.float64)

    def run_shares(self, st):
        """-> (requests per second, largest share / mean share of the engines over the run)"""
        h0 = self.handled()
        rate = self.run(st)
        d = self.handled() - h0
        return rate, float(d.max() / d.mean())

    def close(self):
        self.front.close()
        for e in self.engs:
            e.close()
        self.place.close()


def section_kernel(no_agg):
    w = World()
    w.engs[0].profile(True)
    w.front.observe(1)
    for dist in (("zipf",) if no_agg else ("zipf", "uniform")):
        for G in (65536, G_BIG):
            st = w.stream(dist, G, 8, seed=100 + G % 97)
            w.run(st)                                 # (the keys become resident, the code objects are loaded)
            w.front.observation()
            w.engs[0].profile_read()
            w.run(st)
            ran = w.engs[0].profile_read()
            us = {k: ran[k][1] * 1e3 / ran[k][0] for k in ("k_fr_count", "k_fr_observe") if ran.get(k, (0, 0))[0]}
            obs = w.front.observation()
            num(section="kernel_no_agg" if no_agg else "kernel", dist=dist, requests=G, launches=ran["k_fr_observe"][0], k_fr_count_us=round(us["k_fr_count"], 2),
                k_fr_observe_us=round(us["k_fr_observe"], 2), ratio=round(us["k_fr_observe"] / us["k_fr_count"], 2), observed=obs["observed"], dropped=obs["dropped"],
                candidates=len(obs["candidates"]))
    w.close()


def section_sampling():
    w = World()
    st = w.stream("zipf", G_BIG, 32, seed=7)
    w.run(st)
    rates = {0: [], 16: []}
    for rnd in range(5):
        for every in (0, 16):
            w.front.observe(every)
            rates[every].append(w.run(st))
    off, on = rates[0], rates[16]
    num(section="sampling", generations_per_run=32, requests_per_generation=G_BIG, every0_G_per_s=[round(x / 1e9, 3) for x in off], every16_G_per_s=[round(x / 1e9, 3) for x in on],
        every0_median=round(float(np.median(off)) / 1e9, 3), every16_median=round(float(np.median(on)) / 1e9, 3),
        every0_spread=round((max(off) - min(off)) / 1e9, 3), difference_of_medians=round(float(np.median(on) - np.median(off)) / 1e9, 3))
    w.close()


def section_passes():
    w = World()
    st = w.stream("zipf", G_BIG, 16, seed=11)
    w.run(st)                                         # (the keys become resident)
    w.front.observe(4)
    rate, skew = w.run_shares(st)
    num(section="passes", rule="default", passes=0, G_per_s=round(rate / 1e9, 3), largest_over_mean_share=round(skew, 3))
    for k in range(3):
        ps = w.front.rebalance(w.place)
        rate, skew = w.run_shares(st)
        if k in (0, 2):
            num(section="passes", rule="default", passes=k + 1, G_per_s=round(rate / 1e9, 3), largest_over_mean_share=round(skew, 3), last_pass=ps)
    w.close()
    w = World(fitted=True)
    st = w.stream("zipf", G_BIG, 16, seed=11)
    w.run(st)
    rate, skew = w.run_shares(st)
    num(section="passes", rule="fitted offline (2 M sampled requests, slots and hot keys placed afresh)", passes=0, G_per_s=round(rate / 1e9, 3),
        largest_over_mean_share=round(skew, 3), keys_placed_individually=w.place.n_hot())
    w.close()


SECTIONS = {"kernel": lambda: section_kernel(False), "kernel_no_agg": lambda: section_kernel(True), "sampling": section_sampling, "passes": section_passes}


def main():
    args = sys.argv[1:]
    if args and args[0] in SECTIONS:
        SECTIONS[args[0]]()
        return
    out, usage = os.path.join(ROOT, "profiles", "front_observe_first_numbers.txt"), None
    while args:
        a = args.pop(0)
        if a == "--out":
            out = args.pop(0)
        elif a == "--resource-usage":
            usage = args.pop(0)
        else:
            raise SystemExit(__doc__)
    lines = ["# A front that observes its own traffic: first numbers, one box", "#",
             "# Written by tools/front_observe_numbers.py; every section a process of its own on one MI355X.  The figures of one section are comparable",
             "# with each other (one job, one box), not with another job's.", ""]
    for name in ("kernel", "kernel_no_agg", "sampling", "passes"):
        env = dict(os.environ)
        if name == "kernel_no_agg":
            if not os.path.exists(LAB):
                lines += [f"## {name}: not measured (the laboratory build is missing: make -C gubernator_amd/csrc lab)", ""]
                continue
            env.update(GUBER_HIP_LIB=LAB, GUBER_FRONT_OBSERVE_NO_AGG="1")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), name], capture_output=True, text=True, timeout=600, env=env)
        got = [json.loads(x[4:]) for x in p.stdout.splitlines() if x.startswith("NUM ")]
        lines.append(f"## {name}" + ("" if p.returncode == 0 else f": the section ended with status {p.returncode}; what it printed before:"))
        lines += [json.dumps(g) for g in got]
        if p.returncode:
            lines += ["# " + x for x in (p.stdout + p.stderr).splitlines()[-12:]]
        lines.append("")
        print("\n".join(lines[-len(got) - 2:]), flush=True)
        if p.returncode in (124, 134, 137, 139, -6, -9, -11):        # (nothing more is started on a GPU that has faulted or hung)
            break
    if not any(x.startswith("{") for x in lines):
        raise SystemExit("nothing was measured (no GPU?): " + out + " is left as it is")
    if usage:
        text = open(usage).read()
        lines += ["## registers, LDS and scratch (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)"]
        for m in re.finditer(r"Function Name: (\S*k_fr_\w+)(.*?)(?=Function Name:|\Z)", text, re.S):
            f = dict(re.findall(r"remark:\s+([A-Za-z][\w \[\]/]*?):\s+(\S+)", m.group(2)))
            lines.append(f"{m.group(1)}: VGPRs {f.get('VGPRs')}, SGPRs {f.get('TotalSGPRs')}, scratch {f.get('ScratchSize [bytes/lane]')} B/lane, "
                         f"LDS {f.get('LDS Size [bytes/block]')} B/block, occupancy {f.get('Occupancy [waves/SIMD]')} waves/SIMD")
        lines.append("")
    with open(out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", out)


if __name__ == "__main__":
    main()
