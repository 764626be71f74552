"""First numbers of the mesh's one-launch path (guber_mesh_eval_small), measured in one session on one box beside the two figures it is to
be held against:
  (a) a lone one-item RPC through guber_wire_mesh_pool (a stage set per RPC: the figure of profiles/mesh_pool_first_numbers.txt)
  (b) guber_mesh_eval_dev + guber_mesh_synchronize for the same small generations, already resident on the device (no copies in the figure)
  (c) guber_mesh_eval_small from host arrays, answers in host arrays on return
for totals of 1, 16 and 256 requests at W = 2 and W = 8 LOGICAL ranks of ONE device (one engine per rank, cache 262 144, max_batch
131 072, max_key_bytes 32, two streams — the shape of tools/mesh_pool_first_numbers.py), 2 000 calls after 200 untimed, the arrival rank
round robin (a total above 1 is spread evenly over the ranks), keys "%06d" drawn uniformly from 1 000 000, token and leaky mixed by key,
hits 1, limits never reached.  The figures say nothing about eight GPUs.  Prints the lines profiles/mesh_small_first_numbers.txt holds.
With set_direct(4, 8) the same lone RPCs of 1 and 4 items are evaluated by their caller through (c); at W = 8 the rates of 64 and 192 callers of
1 000-item RPCs with the path off and on (they should not differ: with that many callers everybody is in the sets).
    python tools/mesh_small_numbers.py [calls per figure, default 2000] [norates]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import gubernator_amd as ga  # noqa: E402
from gubernator_amd import wire as gw  # noqa: E402
from gubernator_amd.mesh import Mesh  # noqa: E402
import wire_replay  # noqa: E402

NOW = 1_700_000_000_000
CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
WARM = 200
RATES = "norates" not in sys.argv[2:]
SMALL = True


def columns(rng, n):
    ks = rng.integers(0, 1_000_000, n)
    keys = np.frombuffer(b"".join(b"%06d" % k for k in ks) + b"\0" * 8, np.uint8).copy()
    return dict(key_bytes=keys, key_off=(np.arange(n + 1) * 6).astype(np.uint32), hits=np.ones(n, np.int64), limit=np.full(n, 1 << 40, np.int64),
                duration=np.full(n, 3_600_000, np.int64), algorithm=(ks & 1).astype(np.uint8), behavior=np.zeros(n, np.uint32))


def answers(n):
    return dict(status=np.zeros(n, np.uint8), limit=np.zeros(n, np.int64), remaining=np.zeros(n, np.int64), reset_time=np.zeros(n, np.int64), err=np.zeros(n, np.uint8))


def structs(W, parts, ptr):
    """parts[r]: (columns, answers) or None -> (GuberBatch * W, GuberResult * W); ptr(array) -> the address the call is handed"""
    B, R = (ga.GuberBatch * W)(), (ga.GuberResult * W)()
    for r in range(W):
        if parts[r] is None:
            B[r] = ga.GuberBatch(0, 0, None, None, None, None, None, None, None, None, None, None, None, None, NOW)
            R[r] = ga.GuberResult(None, None, None, None, None, 0, 0, 0, 0, 0)
            continue
        c, a = parts[r]
        B[r] = ga.GuberBatch(len(c["hits"]), 0, ptr(c["key_bytes"]), ptr(c["key_off"]), ptr(c["hits"]), ptr(c["limit"]), ptr(c["duration"]), None, None,
                             ptr(c["algorithm"]), ptr(c["behavior"]), None, None, None, NOW)
        R[r] = ga.GuberResult(ptr(a["status"]), ptr(a["limit"]), ptr(a["remaining"]), ptr(a["reset_time"]), ptr(a["err"]), 0, 0, 0, 0, 0)
    return B, R


def timed(call, variants):
    lat = []
    for q in range(WARM + CALLS):
        v = variants[q % len(variants)]
        t0 = time.perf_counter()
        call(v)
        lat.append(time.perf_counter() - t0)
    lat = np.array(lat[WARM:]) * 1e6
    return "p50 %4.0f us  p99 %4.0f us" % (np.percentile(lat, 50), np.percentile(lat, 99))


def measure(W, dev, strs, rng):
    addrs = ["10.0.0.%d:81" % r for r in range(W)]
    engs = [[ga.Engine(cache_size=262144, max_batch=131072, max_key_bytes=32, stream=strs[r % 2].cuda_stream)] for r in range(W)]
    fronts = [ga.Front(e, None, max_n=65536, depth=3) for e in engs]
    ring = ga.Ring(addrs, 512, "fnv1")
    mesh = Mesh(fronts, ring, 65536)
    print("W = %d logical ranks of one device" % W)
    for total in ((1, 16, 256) if SMALL else ()):
        host_v, dev_v, keep = [], [], []
        for q in range(8):                                            # eight variants: the arrival rank of a lone request goes round
            parts = [None] * W
            for r in range(W):
                n = (1 if r == q % W else 0) if total == 1 else total // W + (1 if r < total % W else 0)
                if n:
                    parts[r] = (columns(rng, n), answers(n))
            host_v.append(structs(W, parts, lambda a: a.ctypes.data))
            dparts = [None if p is None else tuple({k: torch.from_numpy(v).to(dev) for k, v in d.items()} for d in p) for p in parts]
            dev_v.append(structs(W, dparts, lambda t: t.data_ptr()))
            keep.append((parts, dparts))
        torch.cuda.synchronize(dev)

        def general(v):
            mesh.eval_dev(*v)
            mesh.synchronize()
        print("    %3d requests per call:  (b) guber_mesh_eval_dev + synchronize, device-resident  %s   (c) guber_mesh_eval_small, host arrays  %s"
              % (total, timed(general, dev_v), timed(lambda v: mesh.eval_small(*v), host_v)), flush=True)
    if SMALL:
        print("    guber_mesh_small_stats: %s" % mesh.small_stats())
    lone_rpcs(W, mesh, addrs, rng)
    mesh.close()
    for f in fronts:
        f.close()
    for e in engs:
        e[0].close()
    ring.close()


def rpc_of(rng, n):
    return wire_replay.pb_request([dict(name="k", unique_key="%06d" % k, hits=1, limit=1 << 40, duration=3_600_000, algorithm=int(k) & 1, behavior=0)
                                   for k in rng.integers(0, 1_000_000, n)])


def lone_rpcs(W, mesh, addrs, rng):
    """(a) lone RPCs of 1 and 4 items in an idle pool, rank round robin: a stage set per RPC (the path off), then evaluated by their caller
    (set_direct(4, 8)); at W = 8 the rates of 64 and 192 callers of 1 000-item RPCs with the path off and on"""
    L = gw._lib()
    pool = gw.WireMeshPool(mesh, addrs)
    direct = True
    for items in (1, 4):
        variants = [(r, rpc_of(rng, items)) for r in range(W) for _ in range(2)]
        buf, n = C.create_string_buffer(max(L.guber_wire_mesh_pool_response_bound(pool.h, p, len(p)) for _, p in variants)), C.c_size_t(0)

        def rpc(v):
            assert L.guber_wire_mesh_pool_get_rate_limits(pool.h, v[0], v[1], len(v[1]), buf, len(buf), C.byref(n)) == 0
        line = "    (a) guber_wire_mesh_pool, a lone RPC of %d item(s) in an idle pool:  a stage set per RPC  %s" % (items, timed(rpc, variants))
        if direct:
            pool.set_direct(4, 8)
            d0 = pool.direct_stats()["direct_rpcs"]
            line += "   set_direct(4, 8): evaluated by its caller  %s" % timed(rpc, variants)
            assert pool.direct_stats()["direct_rpcs"] - d0 == WARM + CALLS
            pool.set_direct(0, 0)
        print(line, flush=True)
    if W == 8 and RATES:
        argv, sys.argv = sys.argv, sys.argv[:1]                       # (that tool reads its own arguments at import)
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from mesh_pool_first_numbers import drive
        sys.argv = argv
        payloads = [(rpc_of(rng, 1000), 1000) for _ in range(64)]
        payloads_of = lambda t: [payloads[(4 * t + j) % len(payloads)] for j in range(4)]
        bound = lambda p: L.guber_wire_mesh_pool_response_bound(pool.h, p, len(p))
        for callers in (64, 192):
            for on in ((False, True) if direct else (False,)):
                if direct:
                    pool.set_direct(4 if on else 0, 8)
                rate, lat = drive(lambda t, p, b, cap, n_: L.guber_wire_mesh_pool_get_rate_limits(pool.h, t % W, p, len(p), b, cap, C.byref(n_)), bound, payloads_of, callers, 2.0)
                print("    %3d callers of 1 000-item RPCs, the direct path %s: %6.1f M items/s   RPC latency p50 %.0f us  p99 %.0f us"
                      % (callers, "on (4, 8)" if on else "off", rate / 1e6, np.percentile(lat, 50), np.percentile(lat, 99)), flush=True)
    pool.close()


def main():
    dev = torch.device("cuda", 0)
    strs = [torch.cuda.Stream(device=dev) for _ in range(2)]
    rng = np.random.default_rng(6)
    print("%d calls per figure after %d untimed" % (CALLS, WARM))
    for W in (2, 8):
        measure(W, dev, strs, rng)


if __name__ == "__main__":
    main()
