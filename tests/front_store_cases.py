"""Cases of tests/test_front_store_cpu.py, run in a process of their own with GUBER_HIP_LIB pointing at tests/hostsim/libenginesim.so (the
engine's host code and kernels compiled for the CPU: tests/hostsim/enginesim.cpp): tests/front_store.py's scenarios at reduced sizes, numpy
arrays as device memory.
    GUBER_HIP_LIB=tests/hostsim/libenginesim.so python tests/front_store_cases.py <case>"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

import gubernator_amd as ga
import front_edges as fe
import front_store as fs
import support

assert "enginesim" in ga.LIB_PATH, "these cases are for the CPU build of the engine (GUBER_HIP_LIB)"


def make_dev_gen(hb):
    """every column a "device" array of exactly its size (the key buffer ends 8 bytes behind the last key)"""
    n = hb.n
    kb = np.ascontiguousarray(np.concatenate([hb.key_bytes[:int(hb.key_off[-1])], np.full(8, 0xA5, np.uint8)]))
    cols = dict(key_bytes=kb, key_off=hb.key_off, hits=hb.hits, limit=hb.limit, duration=hb.duration, burst=hb.burst, created_at=hb.created_at,
                algorithm=hb.algorithm, behavior=hb.behavior, is_owner=hb.is_owner)
    p = {k: (v.ctypes.data if v is not None else None) for k, v in cols.items()}
    r = fe.result_arrays(n)
    b = ga.GuberBatch(n, 0, p["key_bytes"], p["key_off"], p["hits"], p["limit"], p["duration"], p["burst"], p["created_at"], p["algorithm"], p["behavior"],
                      p["is_owner"], None, None, hb.now_ms)
    res = ga.GuberResult(r["status"].ctypes.data, r["limit"].ctypes.data, r["remaining"].ctypes.data, r["reset_time"].ctypes.data, r["err"].ctypes.data, 0, 0, 0, 0, 0)
    b._keep = res._keep = (cols, r)

    def fetch():
        for name, a in r.items():
            s = fe.SENTINEL_U8 if a.dtype == np.uint8 else fe.SENTINEL_I64
            assert (a[n:] == s).all(), f"{name} written behind the generation's end"
        return r
    return b, res, fetch


def setup(n_engines, n_streams, max_batch, flags=0, max_n=4096, global_engine=-1):
    place = ga.Placement(n_engines) if n_engines > 1 else None
    engs = []
    for j in range(n_engines):
        sj = j * n_streams // n_engines
        first = next((q for q in range(j) if q * n_streams // n_engines == sj), None)
        engs.append(ga.Engine(cache_size=1 << 14, max_batch=max_batch, flags=flags, stream=None if first is None else engs[first].stream_handle()))
    engs[0].profile(True)
    front = ga.Front(engs, place, max_n=max_n, depth=3, global_engine=global_engine)
    route = (lambda keys: place.route_keys(*fe.pack(keys))[0]) if place is not None else None
    return place, engs, front, route


def launches(engs):
    out = {}
    for e in engs:
        for k, v in e.profile_read().items():
            out[k] = out.get(k, 0) + v[0]
    return {k: v for k, v in out.items() if v}


def parity(n_engines, n_streams, max_batch, flags, want, steps=6, max_n=1400, resets=True):
    place, engs, front, _ = setup(n_engines, n_streams, max_batch, flags)
    for e in engs:
        e.profile(True)
    orc = support.Oracle(cache_size=1 << 20)
    count, cuts = fs.parity(front, engs, orc, make_dev_gen, support.MockStore, seed=300 + n_engines, steps=steps, max_n=max_n, resets=resets)
    ran = launches(engs)
    print("parity", n_engines, "engines:", count, "generations,", cuts, "cuts, launches", ran)
    assert (cuts > 0) == resets and all(ran.get(k, 0) > 0 for k in fs.NEW_KERNELS), ran
    if not resets:                                                  # (without pieces an engine takes at most one batch per generation)
        assert sum(e.stats()["batches"] for e in engs) > n_engines * count, [e.stats()["batches"] for e in engs]
    assert any(ran.get(k, 0) > 0 for k in want), (want, ran)
    front.close()
    for e in engs:
        e.close()


def probes(n_engines):
    place, engs, front, route = setup(n_engines, 1, 4096)
    p = fs.Probe(front, engs, make_dev_gen, route)
    for packed in (True, False):
        fs.probe_sizes_and_residency(p, packed, sizes=(0, 1, 64, 65, 1025))
        fs.probe_skew_and_cuts(p, packed, n=2049, n_engines=n_engines)
    orc = support.Oracle(cache_size=1 << 20)
    fs.probe_contract(p, orc)
    ran = launches(engs)
    assert ran.get("k_fr_out_store", 0) == 0 and ran.get("k_fr_elect", 0) > 0, ran
    front.close()
    for e in engs:
        e.close()


def global_engine():
    place, engs, front, route = setup(3, 1, 4096, global_engine=2)
    fs.probe_global(fs.Probe(front, engs, make_dev_gen, route), 2)
    front.close()
    for e in engs:
        e.close()


def collisions():
    place, engs, front, route = setup(3, 1, 4096, flags=ga.FLAG_TEST_WEAK_HASH)
    fs.probe_collisions(fs.Probe(front, engs, make_dev_gen, route))
    front.close()
    for e in engs:
        e.close()


CASES = {
    "parity1": lambda: parity(1, 1, 4096, 0, ("k_eval2", "k_eval3")),
    "parity4": lambda: parity(4, 1, 4096, 0, ("k_eval2_multi",)),
    "parity6x3_pieces": lambda: parity(6, 3, 256, ga.FLAG_TEST_FORCE_PART, ("k_eval3", "k_eval3_multi", "k_evalpart_multi"), steps=3, max_n=1400, resets=False),
    "parity6x3": lambda: parity(6, 3, 2048, ga.FLAG_TEST_FORCE_PART, ("k_eval3", "k_eval3_multi", "k_evalpart_multi"), steps=2, max_n=500),
    "probes3": lambda: probes(3),
    "probes1": lambda: probes(1),
    "collisions": collisions,
    "global_engine": global_engine,
}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("FRONT STORE CASE OK", sys.argv[1])
