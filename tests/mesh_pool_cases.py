"""Scenarios for guber_wire_mesh_pool_* (gubernator_amd/csrc/guber_wire_mesh_pool.h): the payload stage over a mesh — caller threads hand the
serialized GetRateLimitsReq of their RPC to any rank and get serialized GetRateLimitsResp bytes back, with metadata{"owner": <address>} on every
answer another rank owns.  Shared by tests/test_gpu_mesh_pool.py (the product library, every rank a logical rank of device 0) and
tests/test_mesh_pool_cpu.py (the same host code and kernels compiled for the CPU).

Expected bytes come from the protobuf runtime over the per-rank oracles under the mesh's order rule: mesh_enc_cases.EncWorld.expected /
.response and mesh_cases.World, by import.  Where callers run at once no serial order exists to replay; what every serialisation implies is
checked per key over all answers (the recipe of test_concurrent_callers_share_stages_and_every_hit_is_applied_exactly_once).

Shapes: engines of cache_size 65 536, max_batch 8 192, max_key_bytes 64; mesh max_n 8 192; pool max_items 4 096, max_rpcs 16,
max_payload_bytes 256 KiB unless a case says otherwise.

Cases (the letters are the issue's): a one caller walking the ranks, b the golden functional scenarios at W = 2, c concurrent callers,
d stage limits, e refusals, f one rank and eight."""
import ctypes as C
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):         # (run as a script by tests/test_mesh_pool_cpu.py)
    if _p not in sys.path:
        sys.path.insert(0, _p)
import mesh_enc_cases as me
from mesh_cases import LONG_MS, NOW0, STEP_MS, Gen, by_ids
from mesh_enc_cases import E_ALGO, E_GREG, FILL, GLOBAL, TAIL, addr_of
from pb_schema import PB

ENGINE = dict(cache_size=1 << 16, max_batch=8192, max_key_bytes=64)
MAX_N = 8192
POOL = dict(max_items=4096, max_rpcs=16, max_payload_bytes=256 << 10)
NOW = 1_700_000_000_000
HOUR = 3_600_000


def sized(new_engines):
    """new_engines with this file's engine shape, whatever the world asks for"""
    return lambda rank, flags, kw: new_engines(rank, flags, dict(kw, **{k: v for k, v in ENGINE.items() if k != "max_key_bytes"}))


class Cluster:
    """W ranks without oracles: engines, front, the ring named `addrs`, the mesh"""

    def __init__(self, ga, new_engines, W, addrs, n_engines=1, max_key=64, max_n=MAX_N):
        from gubernator_amd.mesh import Mesh
        self.ga, self.W, self.addrs = ga, W, list(addrs)
        self.ring = ga.Ring(self.addrs, 512, "fnv1")
        self.engs, self.places, self.fronts = [], [], []
        for r in range(W):
            engs = new_engines(r, [0] * n_engines, dict(ENGINE, max_key_bytes=max_key))
            place = ga.Placement(n_engines) if n_engines > 1 else None
            self.engs.append(engs); self.places.append(place)
            self.fronts.append(ga.Front(engs, place, max_n=max_n, depth=3))
        self.mesh = Mesh(self.fronts, self.ring, max_n)

    def owners(self, keys):
        return self.ring.route(Gen(keys, NOW).packed())

    def sizes(self):
        return [[e.size() for e in engs] for engs in self.engs]

    def close(self):
        self.mesh.close()
        for f in self.fronts:
            f.close()
        for engs in self.engs:
            for e in engs:
                e.close()
        for p in self.places:
            if p is not None:
                p.close()


def parse(raw):
    m = PB["GetRateLimitsResp"]()
    m.ParseFromString(raw)
    return m


def req(name, ukey, limit, hits=1, duration=HOUR, algorithm=0, behavior=0):
    return dict(name=name, unique_key=ukey, hits=hits, limit=limit, duration=duration, algorithm=algorithm, behavior=behavior)


def join(parts, now):
    """generations one behind the other, with their marked names and forced errors"""
    g = Gen([k for p in parts for k in p.keys], now, hits=np.concatenate([p.hits for p in parts]), limit=np.concatenate([p.limit for p in parts]),
            duration=np.concatenate([p.duration for p in parts]), algorithm=np.concatenate([p.algorithm for p in parts]),
            behavior=np.concatenate([p.behavior for p in parts]))
    g.names, g.force, at = {}, {}, 0
    for p in parts:
        g.names.update({at + i: v for i, v in getattr(p, "names", {}).items()})
        g.force.update({at + i: v for i, v in getattr(p, "force", {}).items()})
        at += p.n
    return g


# ---- a: one caller walking the ranks ----------------------------------------------------------------------------------------------------------
def case_a(make_world):
    """a: one caller, W = 3, rank = RPC number mod 3, 60 RPCs over a frozen clock that advances 500 ms between RPCs (every third RPC's buckets
    last 300 ms).  Item counts 0, 1, 3, P - 1, P, P + 1, 2 P + 1 and 1 000 in turn; RPCs of P - 1 items and more carry every class of
    mesh_enc_cases' cases c and d — local, forwarded, GLOBAL at its owner and at a non-owner, and (every second one) an empty unique_key, an
    empty name, an over-long key, a Gregorian-invalid and an invalid-algorithm item on a forwarded, a local and a GLOBAL-non-owner key.
    Every RPC's bytes; stats.sets = the RPCs that held items; stats.host_rpcs = the RPCs with an item error; sizes equal the oracles'"""
    from gubernator_amd import wire as gw
    P = gw.mesh_enc_piece()
    S = [0, 1, 3, P - 1, P, P + 1, 2 * P + 1, 1000]
    addrs = [addr_of(n, r) for r, n in enumerate((11, 100, 264))]
    w = me.enc_world(make_world, addrs, W=3, n_engines=1, max_n=MAX_N, with_global=True, max_key=64)
    pop = w.spread(8, 150)
    mine = me.owned(w, pop)
    assert min(len(x) for x in mine) >= 100
    plain = np.concatenate([m[30:] for m in mine])                   # (numbers 0..9 plain class keys, 10..19 GLOBAL, 20..29 the forced errors' own)
    rng = np.random.default_rng(81)
    pool = gw.WireMeshPool(w.mesh, addrs, sets=3, wrap_errors=1, **POOL)
    sets = host_rpcs = items = 0
    for c in range(60):
        now, r, n = NOW0 + c * STEP_MS, c % 3, S[(c + c // 8) % 8]
        pool.set_clock(now)
        if n == 0:
            assert pool.get_rate_limits(r, b"") == b""
            continue
        bad = n >= P - 1 and c % 2 == 0
        parts = []
        if n >= P - 1:
            parts.append(me.class_gen(w, pop, mine, r, now, bad, c))
            if bad:
                f = by_ids(pop, [int(mine[(r + 1) % 3][20 + c % 5]), int(mine[r][20 + c % 5]), int(mine[(r + 1) % 3][25 + c % 5])], now, 0)
                f.behavior[2] = GLOBAL
                me.mark(f, 0, force=E_GREG); me.mark(f, 1, force=E_ALGO if c % 4 else E_GREG); me.mark(f, 2, force=E_GREG)
                parts.append(f)
        fill = n - sum(p.n for p in parts)
        ids = plain[np.where(rng.random(fill) < 0.5, rng.integers(0, 24, fill), rng.integers(0, len(plain), fill))]
        parts.insert(len(parts) // 2, by_ids(pop, ids, now, c))
        g = join(parts, now)
        assert g.n == n
        import wire_replay
        got = pool.get_rate_limits(r, wire_replay.pb_request([me.item_of(g, i) for i in range(n)]))
        gens = [g if q == r else Gen([], now) for q in range(3)]
        want, _, routed = w.expected(gens)
        owner, _, kind = routed[r]
        exp = w.response(g, r, 0, n, want[r], owner, kind, True)
        assert got == exp.SerializeToString(), f"a RPC {c} at rank {r} ({n} items, errors {bad}): the bytes differ"
        sets += 1; items += n; host_rpcs += bad
    st = pool.stats()
    assert (st["sets"], st["host_rpcs"], st["items"], st["rpcs"]) == (sets, host_rpcs, items, sets), (st, sets, host_rpcs, items)
    assert st["sealed_idle"] == sets and st["sealed_full"] == 0 and st["forwarded"] == w.mesh.stats()["forwarded"] > 0, st
    pool.close()
    w.check_residency("a")
    w.close()


# ---- b: the reference's golden functional scenarios -------------------------------------------------------------------------------------------
def case_b(make_cluster):
    """b: tests/golden/functional_vectors.json at W = 2, consecutive RPCs alternating ranks: request -> protobuf runtime -> the pool -> protobuf
    runtime -> the reference's expectations"""
    import scenarios
    import wire_replay
    from gubernator_amd import wire as gw
    n_checked = 0
    addrs = [addr_of(11, r) for r in range(2)]
    turn = 0
    for sc in scenarios.load("functional_vectors.json")["scenarios"]:
        cl = make_cluster(2, addrs, max_key=128)
        pool = gw.WireMeshPool(cl.mesh, addrs, sets=2, wrap_errors=1, max_items=2048, max_rpcs=8, max_payload_bytes=256 << 10)
        now = sc["start_ms"]
        steps = [([s["req"]], [s["expect"]], s["advance_ms"]) for s in sc.get("steps", [])]
        steps += [(s["reqs"], s["expect"], s["advance_ms"]) for s in sc.get("batch_steps", [])]
        for si, (reqs, expects, adv) in enumerate(steps):
            pool.set_clock(now)
            rows = wire_replay.rows_of(pool.get_rate_limits(turn % 2, wire_replay.pb_request(reqs)))
            turn += 1
            assert len(rows) == len(reqs)
            for j, (exp, row) in enumerate(zip(expects, rows)):
                where = f"{sc['name']} step {si}[{j}] ({sc['source']}) via the payload stage over a mesh"
                status, limit, remaining, reset_time, error = row
                if exp.get("error"):
                    assert error == exp["error"], f"{where}: {error!r}"
                    assert (status, limit, remaining, reset_time) == (0, 0, 0, 0), where
                else:
                    assert error == "", f"{where}: unexpected error {error!r}"
                    scenarios.check_expect(exp, (status, limit, remaining, reset_time, 0), now, where)
                n_checked += 1
            now += adv
        pool.close()
        cl.close()
    assert n_checked >= 80


# ---- c: concurrent callers --------------------------------------------------------------------------------------------------------------------
def concurrent(cl, pool, callers, ranks, RPCS, ITEMS, KEYS, LIMIT=40, bad_callers=True):
    """the recipe of test_concurrent_callers_share_stages_and_every_hit_is_applied_exactly_once over a mesh: caller t at rank ranks[t]; per key
    over ALL answers admitted <= limit, the admitted remainders sum to a L - a (a + 1) / 2, refusals only once the window is empty; the caller's
    own key counts down by one per RPC; the owner's address exactly on the answers another rank owns; -> the answers' owners seen"""
    import wire_replay
    W = cl.W
    pool.set_clock(NOW)
    own_of_key = cl.owners([b"conc_k%06d" % (37 * k) for k in range(KEYS)])   # (fnv1 keeps consecutive numbers with a handful of owners)
    plans = []
    for t in range(callers):
        rng = np.random.default_rng(100 + t)
        mine = []
        for q in range(RPCS):
            ks = rng.integers(0, KEYS, ITEMS)
            reqs = [req("conc", "k%06d" % (37 * k), LIMIT) for k in ks]
            pos = int(rng.integers(0, ITEMS))
            reqs[pos] = req("own", "caller%02d" % t, 1_000_000)
            mine.append((ks, pos, wire_replay.pb_request(reqs)))
        plans.append(mine)
    own_of_caller = cl.owners([b"own_caller%02d" % t for t in range(callers)])
    raw = [[None] * RPCS for _ in range(callers)]
    failures, turned_away = [], []
    n_bad = 2 if bad_callers else 0
    start = threading.Barrier(callers + n_bad)

    def caller(t):
        try:
            start.wait()
            for q, (_, _, payload) in enumerate(plans[t]):
                raw[t][q] = pool.get_rate_limits(ranks[t], payload)
        except Exception as e:  # noqa: BLE001
            failures.append((t, repr(e)))

    # two more callers whose messages are turned away whole, into the same sets: a truncated message and one of 1 001 items in turn (its keys are
    # the others' with a limit of 1: had any of it been evaluated, conservation below would not hold)
    rng_bad = np.random.default_rng(7)
    too_many = wire_replay.pb_request([req("conc", "k%06d" % (37 * k), 1) for k in rng_bad.integers(0, KEYS, 1001)])
    truncated = plans[0][0][2][:-5]

    def bad_caller(t):
        try:
            start.wait()
            for q in range(RPCS):
                try:
                    pool.get_rate_limits(t % W, too_many if (q + t) & 1 else truncated)
                    failures.append((t, "a message that must be turned away was answered"))
                except cl.ga.GuberError as e:
                    turned_away.append(e.code)
        except Exception as e:  # noqa: BLE001
            failures.append((t, repr(e)))

    th = [threading.Thread(target=caller, args=(t,)) for t in range(callers)] + [threading.Thread(target=bad_caller, args=(t,)) for t in range(n_bad)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not failures, failures[:3]
    if bad_callers:
        assert sorted(set(turned_away)) == [-21, -20] and len(turned_away) == 2 * RPCS and turned_away.count(-20) == RPCS, turned_away[:8]
    admitted = np.zeros(KEYS, np.int64); refused = np.zeros(KEYS, np.int64); sum_rem = np.zeros(KEYS, np.int64)
    seen_owners = set()
    for t in range(callers):
        r = ranks[t]
        for q, (ks, pos, _) in enumerate(plans[t]):
            xs = parse(raw[t][q]).responses
            assert len(xs) == ITEMS
            # the caller's own key: its RPCs are the only ones that touch it, one after the other -> remaining counts down by one per RPC
            assert (xs[pos].status, xs[pos].limit, xs[pos].remaining) == (0, 1_000_000, 1_000_000 - 1 - q), (t, q, xs[pos])
            for j, (k, x) in enumerate(zip(ks, xs)):
                o = int(own_of_caller[t]) if j == pos else int(own_of_key[k])
                meta = dict(x.metadata)
                assert meta == ({"owner": cl.addrs[o]} if o != r else {}), (t, q, j, r, o, meta)
                if o != r:
                    seen_owners.add(o)
                if j == pos:
                    continue
                assert x.error == "" and x.limit == LIMIT and x.status in (0, 1)
                if x.status == 0:
                    admitted[k] += 1; sum_rem[k] += x.remaining
                else:
                    refused[k] += 1
                    assert x.remaining == 0
    assert (admitted <= LIMIT).all()
    assert (sum_rem == admitted * LIMIT - admitted * (admitted + 1) // 2).all()
    assert (admitted[refused > 0] == LIMIT).all()
    assert (refused > 0).any() and (admitted < LIMIT).any()
    st = pool.stats()
    assert st["items"] == callers * RPCS * ITEMS and st["rpcs"] == (callers + n_bad) * RPCS and st["sets"] < st["rpcs"], st
    return seen_owners


def case_c(make_cluster, callers, sets):
    """c: callers at W = 3 (caller t at rank t mod 3), 15 RPCs of 200 items over shared keys of limit 40, one key of the caller's own per RPC;
    two more callers are turned away whole (-20, -21), 15 times each; stats.sets < stats.rpcs, stats.items exact"""
    from gubernator_amd import wire as gw
    addrs = [addr_of(n, r) for r, n in enumerate((11, 100, 128))]
    cl = make_cluster(3, addrs, n_engines=2)
    pool = gw.WireMeshPool(cl.mesh, addrs, sets=sets, batch_wait_us=300, **POOL)
    RPCS, ITEMS = 15, 200
    seen = concurrent(cl, pool, callers, [t % 3 for t in range(callers)], RPCS, ITEMS, KEYS=callers * RPCS * ITEMS // 37)
    assert seen == {0, 1, 2}
    pool.close()
    cl.close()


# ---- d: stage limits --------------------------------------------------------------------------------------------------------------------------
def at_once(pool, cl, jobs):
    """jobs: (rank, payload) per caller, all at once -> the answers"""
    out, failures = [None] * len(jobs), []
    start = threading.Barrier(len(jobs))

    def run(t):
        try:
            start.wait()
            out[t] = [pool.get_rate_limits(r, p) for r, p in jobs[t]]
        except Exception as e:  # noqa: BLE001
            failures.append((t, repr(e)))

    th = [threading.Thread(target=run, args=(t,)) for t in range(len(jobs))]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not failures, failures[:3]
    return out


def case_d(make_cluster):
    """d: max_items 2 048 and callers that send 1 000-item RPCs of keys of their own to ONE rank at once: two fit a stage, the third that asks
    seals it (sealed_full >= 1), and everybody gets the bytes its private keys imply.  (Three callers cannot all stand before one open set —
    a set leaves at once while none is on the GPUs, so one of the three is always on its way — so eight callers send four RPCs each.)
    max_rpcs 2 with six callers of one-item RPCs.  A payload longer than max_payload_bytes: GUBER_E_WIRE_FULL, nothing evaluated"""
    import wire_replay
    from gubernator_amd import wire as gw
    addrs = [addr_of(11, r) for r in range(2)]
    cl = make_cluster(2, addrs)
    pool = gw.WireMeshPool(cl.mesh, addrs, sets=3, max_items=2048, max_rpcs=16, max_payload_bytes=256 << 10, batch_wait_us=100_000)
    pool.set_clock(NOW)
    T, Q, N = 8, 4, 1000
    jobs = [[(1, wire_replay.pb_request([req("d", "c%d_%04d" % (t, i), 3) for i in range(N)])) for q in range(Q)] for t in range(T)]
    own = [cl.owners([b"d_c%d_%04d" % (t, i) for i in range(N)]) for t in range(T)]
    out = at_once(pool, cl, jobs)
    for t in range(T):
        for q in range(Q):                                            # limit 3: remaining 2, 1, 0, then OVER_LIMIT — whoever shared the set
            xs = parse(out[t][q]).responses
            assert len(xs) == N
            assert all((x.status, x.limit, x.remaining, x.error) == (int(q == 3), 3, max(2 - q, 0), "") for x in xs), (t, q)
            assert all(dict(x.metadata) == ({} if o == 1 else {"owner": addrs[0]}) for x, o in zip(xs, own[t])), (t, q)
    st = pool.stats()
    assert st["sealed_full"] >= 1 and st["items"] == T * Q * N and st["sets"] < T * Q, st
    pool.close()
    # two RPCs per stage
    pool = gw.WireMeshPool(cl.mesh, addrs, sets=2, max_items=2048, max_rpcs=2, max_payload_bytes=256 << 10)
    pool.set_clock(NOW)
    jobs = [[(0, wire_replay.pb_request([req("d2", "c%d" % t, 5)])) for q in range(5)] for t in range(6)]
    out = at_once(pool, cl, jobs)
    for t in range(6):
        assert [(x.status, x.remaining) for q in range(5) for x in parse(out[t][q]).responses] == [(0, 4 - q) for q in range(5)], t
    assert pool.stats()["rpcs"] == 30
    pool.close()
    # a payload no empty stage can hold
    pool = gw.WireMeshPool(cl.mesh, addrs, sets=2, max_items=2048, max_rpcs=16, max_payload_bytes=4096)
    sizes, stats = cl.sizes(), cl.mesh.stats()
    big = wire_replay.pb_request([req("d3", "k%04d" % i, 5) for i in range(200)])
    assert len(big) > 4096
    try:
        pool.get_rate_limits(0, big)
    except cl.ga.GuberError as e:
        assert e.code == gw.E_WIRE_FULL, e
    else:
        raise AssertionError("a payload longer than max_payload_bytes was taken")
    assert cl.sizes() == sizes and cl.mesh.stats() == stats and pool.stats()["items"] == 0 and pool.stats()["sets"] == 0
    pool.close()
    cl.close()


# ---- e: refusals ------------------------------------------------------------------------------------------------------------------------------
def case_e(make_cluster):
    """e: cap one below the bound (GUBER_E_NOMEM), rank = W, NULL arguments, an over-long, an empty and a NULL address and max_items above the
    mesh's max_n at create: each refused with sizes, guber_mesh_stats and the pool's items unchanged; a call after close is
    GUBER_E_WIRE_CLOSED; cap equal to the bound leaves the 64 fill bytes behind it alone"""
    import wire_replay
    from gubernator_amd import wire as gw
    ga = make_cluster.ga
    addrs = [addr_of(11, 0), addr_of(264, 1)]
    cl = make_cluster(2, addrs)
    pool = gw.WireMeshPool(cl.mesh, addrs, sets=2, wrap_errors=1, **POOL)
    pool.set_clock(NOW)
    L = pool.L
    keys = ["k%05d" % (i * 37) for i in range(300)]                      # (fnv1 keeps consecutive numbers with one owner)
    payload = wire_replay.pb_request([req("e", k, 9) for k in keys] + [req("e", "", 9), req("", "u", 9), req("e", "x" * 70, 9)])
    assert len(parse(pool.get_rate_limits(0, payload)).responses) == 303
    sizes, stats, items = cl.sizes(), cl.mesh.stats(), pool.stats()["items"]
    assert sum(map(sum, sizes)) == 300 and items == 303
    bound = pool.response_bound(payload)
    assert len(payload) < 8192                                          # (short enough for its records to be counted: the bound knows 303 items)
    longest = 1 + 2 + (1 + 1 + 5 + 1 + 2 + 264)                         # the suffix of the 264-byte address: tag, length, the map entry
    assert bound == 303 * (4 + 44 + 3 + 40 + 256 + 1 + longest) + len(payload), bound

    def unchanged(label):
        assert cl.sizes() == sizes and cl.mesh.stats() == stats and pool.stats()["items"] == items, label

    def refused(code, label, fn):
        try:
            fn()
        except ga.GuberError as e:
            assert e.code == code, (label, e)
        else:
            raise AssertionError(f"{label}: not refused")
        unchanged(label)

    def short():
        try:
            pool.get_rate_limits(0, payload, cap=bound - 1)
        except ga.GuberError as e:
            assert e.needed == bound
            raise

    refused(ga.E_NOMEM, "a cap one below the bound", short)
    refused(ga.E_INVALID_ARG, "rank = W", lambda: pool.get_rate_limits(2, payload))
    buf, n = C.create_string_buffer(bound), C.c_size_t(0)
    for label, args in (("a NULL pool", (None, 0, payload, len(payload), buf, bound, C.byref(n))), ("a NULL request", (pool.h, 0, None, len(payload), buf, bound, C.byref(n))),
                        ("a NULL response", (pool.h, 0, payload, len(payload), None, bound, C.byref(n))), ("a NULL resp_len", (pool.h, 0, payload, len(payload), buf, bound, None))):
        assert L.guber_wire_mesh_pool_get_rate_limits(*args) == ga.E_INVALID_ARG, label
        unchanged(label)
    assert L.guber_wire_mesh_pool_stats(pool.h, None) == ga.E_INVALID_ARG and L.guber_wire_mesh_pool_set_clock(None, 1) == ga.E_INVALID_ARG
    assert L.guber_wire_mesh_pool_response_bound(None, payload, len(payload)) == 0
    refused(ga.E_INVALID_ARG, "an over-long address", lambda: gw.WireMeshPool(cl.mesh, [addrs[0], "x" * 265], **POOL))
    refused(ga.E_INVALID_ARG, "an empty address", lambda: gw.WireMeshPool(cl.mesh, ["", addrs[1]], **POOL))
    refused(ga.E_INVALID_ARG, "a NULL address", lambda: gw.WireMeshPool(cl.mesh, [addrs[0], None], **POOL))
    refused(ga.E_INVALID_ARG, "max_items above the mesh's max_n", lambda: gw.WireMeshPool(cl.mesh, addrs, max_items=MAX_N + 1, max_rpcs=16, max_payload_bytes=256 << 10))
    out = C.c_void_p()
    assert L.guber_wire_mesh_pool_create(None, None, None, C.byref(out)) == ga.E_INVALID_ARG and L.guber_wire_mesh_pool_create(cl.mesh.h, None, None, None) == ga.E_INVALID_ARG
    unchanged("NULL arguments at create")
    # exactly the bound, the tail untouched: the RPC's second evaluation (every key admitted again, the three rejected items' texts, every
    # answer of rank 1's keys with the 264-byte address)
    buf = np.full(bound + TAIL, FILL, np.uint8)
    rc = L.guber_wire_mesh_pool_get_rate_limits(pool.h, 0, payload, len(payload), buf.ctypes.data, bound, C.byref(n))
    assert rc == 0 and 0 < n.value <= bound and (buf[n.value:] == FILL).all()
    m = parse(bytes(buf[:n.value]))
    own = cl.owners([("e_" + k).encode() for k in keys])
    assert [x.remaining for x in m.responses[:300]] == [7] * 300 and [bool(x.error) for x in m.responses[300:]] == [True] * 3
    assert [dict(x.metadata) for x in m.responses[:300]] == [({"owner": addrs[1]} if o == 1 else {}) for o in own] and (own == 1).any() and (own == 0).any()
    assert m.responses[300].error == "field 'unique_key' cannot be empty" and m.responses[301].error == "field 'namespace' cannot be empty"
    assert pool.stats()["host_rpcs"] == 2
    pool.close()
    refused_closed = False
    try:
        pool.get_rate_limits(0, payload)
    except ga.GuberError as e:
        refused_closed = e.code == gw.E_WIRE_CLOSED
    assert refused_closed
    cl.close()


# ---- f: one rank and eight --------------------------------------------------------------------------------------------------------------------
def case_f1(make_cluster, new_engines):
    """f, W = 1: no metadata anywhere; the bytes equal guber_wire_pool's for the same payloads on a twin engine"""
    import wire_replay
    from gubernator_amd import wire as gw
    addrs = [addr_of(11, 0)]
    cl = make_cluster(1, addrs)
    twin = new_engines(0, [0], dict(ENGINE))
    pool = gw.WireMeshPool(cl.mesh, addrs, sets=2, wrap_errors=1, **POOL)
    one = gw.WirePool(twin, None, stages=2, **POOL)
    rng = np.random.default_rng(86)
    for c, n in enumerate((1, 5, 191, 193, 1000, 64)):
        now = NOW + c * 700
        pool.set_clock(now); one.set_clock(now)
        reqs = [req("f", "k%03d" % k, 5 + k % 7, duration=1000 if k % 3 else HOUR, algorithm=k % 2) for k in rng.integers(0, 200, n)]
        if c in (3, 5):
            reqs[2] = req("f", "", 5)
            reqs[-1] = req("f", "y" * 80, 5)
        payload = wire_replay.pb_request(reqs)
        got = pool.get_rate_limits(0, payload)
        assert got == one.get_rate_limits(payload), (c, n)
        assert not any(x.metadata for x in parse(got).responses)
    assert pool.stats()["forwarded"] == 0 and pool.stats()["host_rpcs"] == 2
    assert cl.sizes()[0][0] == twin[0].size() > 0
    one.close(); pool.close()
    for e in twin:
        e.close()
    cl.close()


def case_f8(make_cluster):
    """f, W = 8: 16 callers at ranks 0 - 5 only, so ranks 6 and 7 receive nothing in every set — and still own and answer keys; conservation
    as in c on a smaller plan"""
    from gubernator_amd import wire as gw
    addrs = [addr_of(n, r) for r, n in enumerate(me.ADDR_LENS)]
    cl = make_cluster(8, addrs)
    pool = gw.WireMeshPool(cl.mesh, addrs, sets=3, batch_wait_us=300, **POOL)
    seen = concurrent(cl, pool, 16, [t % 6 for t in range(16)], RPCS=6, ITEMS=100, KEYS=16 * 6 * 100 // 37, bad_callers=False)
    assert seen == set(range(8)), seen
    sizes = cl.sizes()
    assert sizes[6][0] > 0 and sizes[7][0] > 0, sizes
    pool.close()
    cl.close()


def cluster_maker(ga, new_engines):
    def make_cluster(W, addrs, **kw):
        return Cluster(ga, new_engines, W, addrs, **kw)
    make_cluster.ga = ga
    return make_cluster


def run(letter, ga, support, new_engines, upload, download):
    mw = me.world_maker(ga, support, sized(new_engines), upload, download)
    mc_ = cluster_maker(ga, new_engines)
    {"a": lambda: case_a(mw), "b": lambda: case_b(mc_), "c12": lambda: case_c(mc_, 12, 3), "c24": lambda: case_c(mc_, 24, 2), "d": lambda: case_d(mc_),
     "e": lambda: case_e(mc_), "f1": lambda: case_f1(mc_, new_engines), "f8": lambda: case_f8(mc_)}[letter]()


LETTERS = ("a", "b", "c12", "c24", "d", "e", "f1", "f8")


# ---- the cases on the CPU build of the engine (tests/test_mesh_pool_cpu.py): GUBER_HIP_LIB=tests/hostsim/libenginesim.so python tests/mesh_pool_cases.py <letter>
def _cpu_main(letter):
    import gubernator_amd as ga
    import support
    assert "enginesim" in ga.LIB_PATH, "this entry is for the CPU build of the engine (GUBER_HIP_LIB)"

    def new_engines(rank, flags, kw):
        e0 = ga.Engine(flags=flags[0], **kw)
        return [e0] + [ga.Engine(flags=f, stream=e0.stream_handle(), **kw) for f in flags[1:]]

    run(letter, ga, support, new_engines, lambda a: (a, a.ctypes.data), lambda a: a)
    print("MESH POOL CASE OK", letter)


if __name__ == "__main__":
    _cpu_main(sys.argv[1])
