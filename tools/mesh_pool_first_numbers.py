"""First numbers of the payload stage over a mesh (guber_wire_mesh_pool_*) and its two reference points, measured in one session on one box:
  (a) guber_wire_mesh_pool at W = 8 logical ranks of ONE device with CALLERS caller threads (Python threads; the call releases the GIL)
  (b) guber_wire_dev_eval_mesh_enc driven by one thread over the same mesh (the decode is not in the figure)
  (c) guber_wire_pool over eight engines of the same device with the same caller counts
The configuration is profiles/mesh_enc_first_numbers.txt's: one engine per rank (cache 262 144, max_batch 131 072, max_key_bytes 32) on two
streams, 11-byte addresses "10.0.0.N:81", RPCs of up to 1 000 items, name "k", unique_key "%06d" drawn uniformly from 1 000 000, token and
leaky mixed by key, hits 1, limits never reached.  Prints the lines profiles/mesh_pool_first_numbers.txt holds.
    python tools/mesh_pool_first_numbers.py [seconds per run, default 3] [caller counts, default 64,192; "b": reference point (b) alone — what a
                                            library without the pool (GUBER_HIP_LIB) can run]"""
import ctypes as C
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import gubernator_amd as ga  # noqa: E402
from gubernator_amd import wire as gw  # noqa: E402
from gubernator_amd.mesh import Mesh  # noqa: E402
import wire_replay  # noqa: E402

W, NOW = 8, 1_700_000_000_000
SECONDS = float(sys.argv[1]) if len(sys.argv) > 1 else 3.0
ONLY_B = len(sys.argv) > 2 and sys.argv[2] == "b"
CALLERS = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 and not ONLY_B else [64, 192]
ADDRS = ["10.0.0.%d:81" % r for r in range(W)]


def payload(rng, n):
    ks = rng.integers(0, 1_000_000, n)
    return wire_replay.pb_request([dict(name="k", unique_key="%06d" % k, hits=1, limit=1 << 40, duration=3_600_000, algorithm=int(k) & 1, behavior=0) for k in ks])


def drive(call, bound, payloads_of, callers, seconds):
    """callers threads, each looping over its payloads until the time is up -> (items/s, latencies in us)"""
    lat, items, stop = [[] for _ in range(callers)], [0] * callers, [False]
    start = threading.Barrier(callers + 1)

    def run(t):
        mine = payloads_of(t)
        buf, n = C.create_string_buffer(max(bound(p) for p, _ in mine)), C.c_size_t(0)
        start.wait()
        q = 0
        while not stop[0]:
            p, k = mine[q % len(mine)]
            t0 = time.perf_counter()
            rc = call(t, p, buf, len(buf), n)
            lat[t].append(time.perf_counter() - t0)
            assert rc == 0, (rc, ga.lib().guber_last_error())
            items[t] += k
            q += 1

    th = [threading.Thread(target=run, args=(t,)) for t in range(callers)]
    for x in th:
        x.start()
    start.wait()
    t0 = time.perf_counter()
    time.sleep(seconds)
    stop[0] = True
    for x in th:
        x.join()
    dt = time.perf_counter() - t0
    return sum(items) / dt, np.array([x for l in lat for x in l]) * 1e6


def main():
    dev = torch.device("cuda", 0)
    strs = [torch.cuda.Stream(device=dev) for _ in range(2)]
    rng = np.random.default_rng(5)
    print("building payloads ...", flush=True)
    pool_payloads = [(payload(rng, 1000), 1000) for _ in range(256)]
    payloads_of = lambda t: [pool_payloads[(4 * t + j) % len(pool_payloads)] for j in range(4)]
    engs = [[ga.Engine(cache_size=262144, max_batch=131072, max_key_bytes=32, stream=strs[r % 2].cuda_stream)] for r in range(W)]
    fronts = [ga.Front(e, None, max_n=65536, depth=3) for e in engs]
    ring = ga.Ring(ADDRS, 512, "fnv1")
    mesh = Mesh(fronts, ring, 65536)
    L = gw._lib()

    # ---- (a) the payload stage over the mesh
    pool = gw.WireMeshPool(mesh, ADDRS) if not ONLY_B else None
    bound = lambda p: L.guber_wire_mesh_pool_response_bound(pool.h, p, len(p))
    if not ONLY_B:
        measure_pool(L, pool, bound, payloads_of, rng)
    measure_enc(L, engs, fronts, mesh, rng)
    if not ONLY_B:
        measure_one_device(L, payloads_of)


def measure_pool(L, pool, bound, payloads_of, rng):
    one = payload(rng, 1)
    buf, n = C.create_string_buffer(bound(one)), C.c_size_t(0)
    lone = []
    for q in range(2200):
        t0 = time.perf_counter()
        assert L.guber_wire_mesh_pool_get_rate_limits(pool.h, q % W, one, len(one), buf, len(buf), C.byref(n)) == 0
        lone.append(time.perf_counter() - t0)
    print("(a) guber_wire_mesh_pool, W = 8 logical ranks of one device, defaults (3 sets of 49 152 items per rank, BatchWait 500 us)")
    print("    a lone one-item RPC in an idle pool (2 000 after 200 untimed, rank round robin): p50 %.0f us  p99 %.0f us" % (np.percentile(lone[200:], 50) * 1e6, np.percentile(lone[200:], 99) * 1e6))
    for callers in CALLERS:
        s0 = pool.stats()
        rate, lat = drive(lambda t, p, b, cap, n_: L.guber_wire_mesh_pool_get_rate_limits(pool.h, t % W, p, len(p), b, cap, C.byref(n_)), bound, payloads_of, callers, SECONDS)
        s1 = pool.stats()
        d = {k: s1[k] - s0[k] for k in s1}
        print("    %3d callers: %6.1f M items/s   %d RPCs in %d sets (mean %.0f items per set; full %d, BatchWait %d, idle %d)   RPC latency p50 %.0f us  p99 %.0f us   "
              "per set: fill %.0f us, GPUs %.0f us   forwarded %.3f" % (callers, rate / 1e6, d["rpcs"], d["sets"], d["items"] / max(d["sets"], 1), d["sealed_full"], d["sealed_wait"],
                                                                           d["sealed_idle"], np.percentile(lat, 50), np.percentile(lat, 99), d["fill_us_sum"] / max(d["sets"], 1),
                                                                           d["gpu_us_sum"] / max(d["sets"], 1), d["forwarded"] / max(d["items"], 1)), flush=True)
    pool.close()


def measure_enc(L, engs, fronts, mesh, rng):
    # ---- (b) guber_wire_dev_eval_mesh_enc, one thread: 66 RPCs per rank (65 of 1 000 items, one of 536: 65 536 per rank), decoded once
    decs = [gw.DevWireDecoder(engs[r][0], max_items=65536, max_payload_bytes=4 << 20, max_rpcs=128) for r in range(W)]
    for r in range(W):
        status, _, _, n_items = decs[r].decode([payload(rng, 1000) for _ in range(65)] + [payload(rng, 536)], NOW, max_per_rpc=1000)
        assert n_items == 65536 and (status == 0).all()
    L.guber_wire_dev_eval_mesh_enc.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(gw.MeshResp)]
    addrs, arr = gw._addr_array(ADDRS)
    dv = (C.c_void_p * W)(*[d.h for d in decs])
    out, keep = (gw.MeshResp * W)(), []
    for r in range(W):
        cap = gw.mesh_enc_bound(decs[r], addrs)
        b, off, ln = np.zeros(cap, np.uint8), np.zeros(66, np.uint32), np.zeros(66, np.uint32)
        out[r] = gw.MeshResp(b.ctypes.data, cap, off.ctypes.data, ln.ctypes.data, None)
        keep.append((b, off, ln))
    for q in range(25):
        if q == 5:
            t0 = time.perf_counter()
        assert L.guber_wire_dev_eval_mesh_enc(dv, mesh.h, arr, 1, out) == 0
    dt = time.perf_counter() - t0
    print("(b) guber_wire_dev_eval_mesh_enc, one thread, 524 288 items per call in 528 RPCs, 5 untimed calls then 20: %.0f us per call   %.1f M items/s (decode not included)"
          % (dt / 20 * 1e6, 20 * 524288 / dt / 1e6), flush=True)
    for d in decs:
        d.close()
    mesh.close()
    for f in fronts:
        f.close()
    for e in engs:
        e[0].close()


def measure_one_device(L, payloads_of):
    # ---- (c) guber_wire_pool over eight engines of the device
    e0 = ga.Engine(cache_size=262144, max_batch=131072, max_key_bytes=32)
    tabs = [e0] + [ga.Engine(cache_size=262144, max_batch=131072, max_key_bytes=32, stream=e0.stream_handle()) for _ in range(7)]
    place = ga.Placement(8)
    one_dev = gw.WirePool(tabs, place)
    one_dev.set_clock(NOW)
    print("(c) guber_wire_pool, eight engines of the same device, defaults (12 stages of 49 152 items)")
    for callers in CALLERS:
        s0 = one_dev.stats()
        rate, lat = drive(lambda t, p, b, cap, n_: L.guber_wire_pool_get_rate_limits(one_dev.h, p, len(p), 1, 1, b, cap, C.byref(n_)),
                          lambda p: L.guber_wire_pool_response_bound(p, len(p)), payloads_of, callers, SECONDS)
        s1 = one_dev.stats()
        d = {k: s1[k] - s0[k] for k in s1}
        print("    %3d callers: %6.1f M items/s   %d RPCs in %d stages (mean %.0f items per stage)   RPC latency p50 %.0f us  p99 %.0f us"
              % (callers, rate / 1e6, d["rpcs"], d["stages"], d["items"] / max(d["stages"], 1), np.percentile(lat, 50), np.percentile(lat, 99)), flush=True)
    one_dev.close()
    for e in reversed(tabs):
        e.close()
    place.close()


if __name__ == "__main__":
    main()
