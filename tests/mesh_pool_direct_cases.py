"""Scenarios for the payload stage over a mesh with lone small RPCs evaluated by their caller (guber_wire_mesh_pool_set_direct,
gubernator_amd/csrc/guber_wire_mesh_pool_direct.h: the host transcoder, guber_mesh_eval_small, wire_mesh_enc_host_rpc).  Shared by
tests/test_gpu_mesh_pool_direct.py (the product library, every rank a logical rank of device 0) and tests/test_mesh_pool_direct_cpu.py
(the same host code and kernels compiled for the CPU).  Built on mesh_pool_cases and mesh_enc_cases by import: expected bytes come from
the protobuf runtime over the per-rank oracles under the mesh's order rule.

Cases (the letters are the issue's): j one caller walking three ranks with set_direct(4, 8), wrap_errors 0 and 1; k refusals with the path
on; l 16 concurrent callers with set_direct(4, 2): both paths; m off by default, and off again."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):         # (run as a script by tests/test_mesh_pool_direct_cpu.py)
    if _p not in sys.path:
        sys.path.insert(0, _p)
import mesh_enc_cases as me
import mesh_pool_cases as mp
from mesh_cases import LONG_MS, NOW0, STEP_MS, Gen, by_ids
from mesh_enc_cases import E_ALGO, E_GREG, GLOBAL, addr_of
from mesh_pool_cases import MAX_N, NOW, POOL, parse, req


def shape(w, pop, mine, r, now, k, c):
    """the items of RPC c at rank r, shape k: keys 0..9 of every owner are plain, 10..19 GLOBAL, 20..29 the forced errors' own"""
    o, s = (r + 1) % w.W, c % 10
    local, fwd, g_own, g_non, other = int(mine[r][s]), int(mine[o][s]), int(mine[r][10 + s]), int(mine[o][10 + s]), int(mine[(r + 2) % w.W][s])
    if k == 0:                                                      # one local item
        return by_ids(pop, [local], now, 0)
    if k == 1:                                                      # forwarded, local
        return by_ids(pop, [fwd, local], now, 0)
    if k in (2, 3):                                                 # local, forwarded, GLOBAL at its owner, GLOBAL at a non-owner (k = 3: a fifth item — a set)
        g = by_ids(pop, [local, fwd, g_own, g_non] + ([other] if k == 3 else []), now, 0)
        g.behavior[2] = g.behavior[3] = GLOBAL
        return g
    if k == 4:                                                      # a forwarded item alone
        return by_ids(pop, [fwd], now, 0)
    if k in (5, 8):                                                 # local, an empty unique_key (k = 8: among five items — a set whose RPC its caller marshals)
        g = by_ids(pop, [local, local] + ([fwd, other, local] if k == 8 else []), now, 0)
        me.mark(g, 1, "k", "")
        return g
    if k == 6:                                                      # forwarded, an empty name, an over-long key, local
        g = by_ids(pop, [fwd, local, local, local], now, 0)
        me.mark(g, 1, "", "u")
        g.keys[2] = b"k_" + b"x" * (w.max_key - 1)                 # one byte more than the engines' max_key_bytes
        g.hits[2], g.limit[2], g.duration[2], g.algorithm[2], g.behavior[2] = 1, 10, LONG_MS, 0, 0
        return g
    # k == 7: Gregorian-invalid on a forwarded key, an invalid algorithm on a local one, Gregorian-invalid on a GLOBAL key at a non-owner, local
    g = by_ids(pop, [int(mine[o][20 + c % 5]), int(mine[r][20 + c % 5]), int(mine[o][25 + c % 5]), local], now, 0)
    g.behavior[2] = GLOBAL
    me.mark(g, 0, force=E_GREG); me.mark(g, 1, force=E_ALGO); me.mark(g, 2, force=E_GREG)
    return g


def case_j(make_world, wrap):
    """j: one caller, W = 3, rank = RPC number mod 3, set_direct(4, 8), a frozen clock that advances: RPCs of 1, 2 and 4 items are served
    directly (stats.sets does not move, direct_stats counts them), RPCs of 5 items go through a set; local, forwarded, GLOBAL at owner and
    at non-owner; an empty unique_key, an empty name, an over-long key, an invalid algorithm, Gregorian-invalid; every RPC's bytes"""
    import wire_replay
    from gubernator_amd import wire as gw
    addrs = [addr_of(n, r) for r, n in enumerate((11, 100, 264))]
    w = me.enc_world(make_world, addrs, W=3, n_engines=1, max_n=MAX_N, with_global=True, max_key=64)
    pop = w.spread(8, 150)
    mine = me.owned(w, pop)
    assert min(len(x) for x in mine) >= 100
    pool = gw.WireMeshPool(w.mesh, addrs, sets=3, wrap_errors=wrap, **POOL)
    pool.set_direct(4, 8)
    direct = sets = items = host_rpcs = 0
    for c in range(45):
        now, r, k = NOW0 + c * STEP_MS, c % 3, (c + c // 9) % 9
        pool.set_clock(now)
        g = shape(w, pop, mine, r, now, k, c)
        before = pool.stats()["sets"]
        got = pool.get_rate_limits(r, wire_replay.pb_request([me.item_of(g, i) for i in range(g.n)]))
        gens = [g if q == r else Gen([], now) for q in range(3)]
        want, _, routed = w.expected(gens)
        owner, _, kind = routed[r]
        exp = w.response(g, r, 0, g.n, want[r], owner, kind, bool(wrap))
        assert got == exp.SerializeToString(), f"j RPC {c} at rank {r} (shape {k}, {g.n} items, wrap_errors {wrap}): the bytes differ"
        direct += g.n <= 4; sets += g.n > 4; items += g.n; host_rpcs += k == 8
        assert pool.stats()["sets"] - before == int(g.n > 4) and pool.direct_stats()["direct_rpcs"] == direct, (c, k, pool.stats(), pool.direct_stats())
    st, ds = pool.stats(), pool.direct_stats()
    assert (st["sets"], st["items"], st["rpcs"], st["host_rpcs"]) == (sets, items, direct + sets, host_rpcs) and sets >= 8 and direct >= 30, (st, ds)
    assert st["forwarded"] == w.mesh.stats()["forwarded"] > 0 and ds["fallback_rpcs"] == 0, (st, ds, w.mesh.stats())
    assert w.mesh.small_stats()["calls"] == direct
    pool.close()
    w.check_residency(f"j wrap_errors {wrap}")
    w.close()


def case_k(make_cluster):
    """k: with the path on, a malformed payload, an RPC above max_per_rpc, a cap below the bound and len == 0 get the codes they get with
    it off, and nothing is evaluated"""
    import wire_replay
    from gubernator_amd import wire as gw
    ga = make_cluster.ga
    addrs = [addr_of(11, 0), addr_of(100, 1)]
    cl = make_cluster(2, addrs)
    pool = gw.WireMeshPool(cl.mesh, addrs, sets=2, wrap_errors=1, max_per_rpc=3, **POOL)
    pool.set_clock(NOW)
    good = wire_replay.pb_request([req("k", "a%04d" % (i * 37), 9) for i in range(2)])
    four = wire_replay.pb_request([req("k", "b%04d" % (i * 37), 9) for i in range(4)])
    bound = pool.response_bound(good)

    def codes():
        out = []
        for payload, cap in ((good[:-3], None), (four, None), (good, bound - 1)):
            try:
                pool.get_rate_limits(0, payload, cap=cap)
                out.append(0)
            except ga.GuberError as e:
                out.append((e.code, getattr(e, "needed", 0) if cap is not None else 0))
        out.append(pool.get_rate_limits(1, b""))
        return out
    off = codes()
    assert off == [(gw.E_WIRE_MALFORMED, 0), (gw.E_WIRE_TOO_LARGE, 0), (ga.E_NOMEM, bound), b""], off
    assert len(parse(pool.get_rate_limits(0, good)).responses) == 2
    sizes, stats, st0, ds0 = cl.sizes(), cl.mesh.stats(), pool.stats(), pool.direct_stats()
    pool.set_direct(4, 8)
    assert codes() == off
    st1 = pool.stats()
    assert cl.sizes() == sizes and cl.mesh.stats() == stats and cl.mesh.small_stats()["calls"] == 0 and pool.direct_stats() == ds0 == dict(direct_rpcs=0, fallback_rpcs=0)
    assert st1["items"] == st0["items"] and st1["sets"] == st0["sets"], (st0, st1)
    # ... and the same good RPC is now served directly
    assert [x.remaining for x in parse(pool.get_rate_limits(0, good)).responses] == [7, 7]
    assert pool.direct_stats()["direct_rpcs"] == 1 and pool.stats()["sets"] == st0["sets"]
    try:
        pool.set_direct(257, 0)
        raise AssertionError("k: set_direct took 257 items")
    except ga.GuberError as e:
        assert e.code == ga.E_INVALID_ARG
    pool.close()
    cl.close()


def case_l(make_cluster):
    """l: 16 threads send RPCs of one shared hot key and one key of their own with set_direct(4, 2), so direct calls and sets mix: per-key
    conservation over all answers (mesh_pool_cases.concurrent), and both paths were taken"""
    from gubernator_amd import wire as gw
    addrs = [addr_of(n, r) for r, n in enumerate((11, 100, 128))]
    cl = make_cluster(3, addrs, n_engines=2)
    pool = gw.WireMeshPool(cl.mesh, addrs, sets=3, batch_wait_us=300, **POOL)
    pool.set_direct(4, 2)
    callers, RPCS = 16, 20
    mp.concurrent(cl, pool, callers, [t % 3 for t in range(callers)], RPCS, ITEMS=2, KEYS=8, bad_callers=False)
    # (a caller that is alone inside the pool — the last ones to finish are — takes the direct path whatever the others did)
    import wire_replay
    for q in range(3):
        pool.get_rate_limits(q, wire_replay.pb_request([req("own", "tail%d" % q, 5)]))
    st, ds = pool.stats(), pool.direct_stats()
    assert ds["direct_rpcs"] >= 3 and st["sets"] >= 1 and st["rpcs"] == callers * RPCS + 3, (st, ds)
    assert cl.mesh.small_stats()["calls"] == ds["direct_rpcs"]
    pool.close()
    cl.close()


def case_m(make_cluster):
    """m: without set_direct nothing is served directly; set_direct(0, 0) switches the path off again"""
    import wire_replay
    from gubernator_amd import wire as gw
    addrs = [addr_of(11, 0), addr_of(100, 1)]
    cl = make_cluster(2, addrs)
    pool = gw.WireMeshPool(cl.mesh, addrs, sets=2, **POOL)
    pool.set_clock(NOW)
    one = wire_replay.pb_request([req("m", "only", 9)])
    want = []
    for phase, (arg, direct) in enumerate(((None, False), ((4, 0), True), ((0, 0), False), ((1, 1), True))):
        if arg is not None:
            pool.set_direct(*arg)
        for q in range(3):
            s0, d0 = pool.stats()["sets"], pool.direct_stats()["direct_rpcs"]
            x = parse(pool.get_rate_limits(q % 2, one)).responses[0]
            want.append(x.remaining)
            assert pool.stats()["sets"] - s0 == int(not direct) and pool.direct_stats()["direct_rpcs"] - d0 == int(direct), (phase, q)
    assert want == [8, 7, 6, 5, 4, 3, 2, 1, 0, 0, 0, 0]                  # one bucket, whichever path an RPC took
    assert cl.mesh.small_stats()["calls"] == 6
    pool.close()
    cl.close()


LETTERS = ("j0", "j1", "k", "l", "m")


def run(letter, ga, support, new_engines, upload, download):
    mw = me.world_maker(ga, support, mp.sized(new_engines), upload, download)
    mc_ = mp.cluster_maker(ga, new_engines)
    {"j0": lambda: case_j(mw, 0), "j1": lambda: case_j(mw, 1), "k": lambda: case_k(mc_), "l": lambda: case_l(mc_), "m": lambda: case_m(mc_)}[letter]()


# ---- on the CPU build of the engine (tests/test_mesh_pool_direct_cpu.py): GUBER_HIP_LIB=tests/hostsim/libenginesim.so python tests/mesh_pool_direct_cases.py <letter>
def _cpu_main(letter):
    import gubernator_amd as ga
    import support
    assert "enginesim" in ga.LIB_PATH, "this entry is for the CPU build of the engine (GUBER_HIP_LIB)"

    def new_engines(rank, flags, kw):
        e0 = ga.Engine(flags=flags[0], **kw)
        return [e0] + [ga.Engine(flags=f, stream=e0.stream_handle(), **kw) for f in flags[1:]]

    run(letter, ga, support, new_engines, lambda a: (a, a.ctypes.data), lambda a: a)
    print("MESH POOL DIRECT CASE OK", letter)


if __name__ == "__main__":
    _cpu_main(sys.argv[1])
