"""The peer RPCs on the payload stage (include/guber_wire.h guber_wire_pool_get_peer_rate_limits / guber_wire_pool_update_peer_globals):
V1Instance.GetPeerRateLimits (gubernator.go:462-539) and V1Instance.UpdatePeerGlobals (:425-459) on the SERIALIZED messages.  What the peer
RPC does differently from the client RPC — no per-item validation, DRAIN_OVER_LIMIT ORed into forwarded GLOBAL items, its own error texts —
is decided on the device (k_wire_fill, from the RPC's flag byte) for the stages and by the host transcoder for an RPC its caller evaluates.
Checked byte for byte against the peer host transcoder (tests/test_wire_peer_cpu.py pins it on a model of the reference's rules) around the
ORACLE, on a hand-written table of draining scenarios, and — with concurrent callers — by per-key conservation.  With 1 and 4 tables, with
and without a GLOBAL engine.  Runs unchanged against the CPU build of the engine under AddressSanitizer (tests/test_wire_peer_cpu.py)."""
import ctypes as C
import os
import subprocess
import threading
import zlib

import numpy as np
import pytest

import gubernator_amd as ga
import scenarios
import support
import wire_replay
import wire_shapes
from gubernator_amd import wire as gw
from pb_schema import PB
from test_wire_cpu import NOW, rand_reqs

pytestmark = pytest.mark.gpu

SMALL = dict(stages=3, max_items=8192, max_payload_bytes=1 << 20, max_rpcs=64)
# (tables the placement spreads keys over, a GLOBAL engine behind them or not)
CONFIGS = [(1, False), (4, False), (1, True), (4, True)]
IDS = ["1_table", "4_tables", "1_table+global_engine", "4_tables+global_engine"]


class Rig:
    """n plain tables of one stream (+ a GLOBAL engine), the payload stage over them, one oracle, one host batch"""

    def __init__(self, n_plain, with_global, max_key_bytes=256, **cfg):
        n = n_plain + (1 if with_global else 0)
        e0 = ga.Engine(cache_size=1 << 16, max_batch=8192, max_key_bytes=max_key_bytes)
        self.engs = [e0] + [ga.Engine(cache_size=1 << 16, max_batch=8192, max_key_bytes=max_key_bytes, stream=e0.stream_handle()) for _ in range(n - 1)]
        self.place = ga.Placement(n_plain) if n > 1 else None
        self.global_engine = n_plain if with_global else -1
        self.pool = gw.WirePool(self.engs, self.place, global_engine=self.global_engine, **(cfg or SMALL))
        self.o = support.Oracle(cache_size=1 << 20)
        self.wb = gw.WireBatch(4096, 1 << 20)

    def size(self):
        return sum(e.size() for e in self.engs)

    def expected(self, payload, now, peer, wrap=True):
        """the host transcoder — in the RPC's mode — around the oracle: the bytes the pool must return"""
        self.wb.reset(now)
        first, count = self.wb.decode(payload, max_per_rpc=1000, peer=peer)
        self.o.lib.oracle_eval_batch(self.o.h, C.byref(self.wb.view()), C.byref(self.wb.result()))
        return self.wb.encode(first, count, wrap_errors=wrap, peer=peer)

    def call(self, payload, now, peer, wrap=True):
        self.pool.set_clock(now)
        return self.pool.get_peer_rate_limits(payload) if peer else self.pool.get_rate_limits(payload, wrap_errors=wrap)

    def close(self):
        self.pool.close()
        for e in reversed(self.engs):
            e.close()
        if self.place:
            self.place.close()
        self.o.close(); self.wb.close()


def _global_by_key(reqs):
    """a key is either always GLOBAL or never (a GLOBAL engine keeps the GLOBAL ones in a table of its own: ONE oracle can follow only then)"""
    for r in reqs:
        g = zlib.crc32((r["name"] + "_" + r["unique_key"]).encode()) % 3 == 0
        r["behavior"] = (r["behavior"] & ~2) | (2 if g else 0)
    return reqs


def _req(name, uk, hits, limit=100, duration=3_600_000, algorithm=0, behavior=0):
    return dict(name=name, unique_key=uk, hits=hits, limit=limit, duration=duration, algorithm=algorithm, behavior=behavior, burst=0, created_at=0)


@pytest.mark.parametrize("n_plain,with_global", CONFIGS, ids=IDS)
def test_one_caller_gets_the_peer_transcoders_bytes_around_the_oracle(n_plain, with_global):
    """RPC after RPC from one thread, peer and client RPCs in turn on the same keys, 1 .. 4 requests (evaluated by their caller) and 5 .. 700
    (through the stages): every response equals the host transcoder's — in the RPC's mode — around ONE oracle.  A scripted part guarantees by
    construction (a) forwarded GLOBAL requests, token and leaky, that ask for more than remains: the answer before says remaining 40, the
    request asks for 50 — remaining must be 0 afterwards (gubernator.go:506-512), asserted on the response itself, not only through the
    oracle; (b) peer requests with an empty unique_key or name that hit the bucket an earlier request of the same key made: limit 10, the
    first hit left 9, the second must leave 8 (client.go:39: the key is name + "_" + unique_key, no validation on this path)."""
    rng = np.random.default_rng(131 + n_plain + 7 * with_global)
    rig = Rig(n_plain, with_global)
    # ---- the scripted items: (request, what its response must say or None, kind), spread over the RPCs below
    first_hits, second_hits = [], []
    for j in range(12):
        for algo in (0, 1):
            name, uk = "drain%d" % algo, "k%d" % j
            # (ten hours: a leaky bucket gains a token in six minutes, the run spans one)
            first_hits.append((_req(name, uk, 60, duration=36_000_000, algorithm=algo, behavior=2), (0, 100, 40), None))
            second_hits.append((_req(name, uk, 50, duration=36_000_000, algorithm=algo, behavior=2), (1, 100, 0), "over_ask"))
    for j in range(11):
        for name, uk in (("solo%d" % j, ""), ("", "lone%d" % j)):
            first_hits.append((_req(name, uk, 1, limit=10), (0, 10, 9), None))
            second_hits.append((_req(name, uk, 1, limit=10), (0, 10, 8), "empty_half"))
    first_hits.append((_req("", "", 1, limit=10), (0, 10, 9), None))
    second_hits.append((_req("", "", 1, limit=10), (0, 10, 8), "empty_half"))
    second_hits.append((_req("", "", 1, limit=10), (0, 10, 7), "empty_half"))
    order = rng.permutation(len(first_hits))
    first_hits = [first_hits[i] for i in order]
    rng.shuffle(second_hits)
    # the third ("_" again) must come after the second: keep the two "_" requests of second_hits in the order limit-2, limit-3
    both = [i for i, s in enumerate(second_hits) if s[0]["name"] == "" and s[0]["unique_key"] == ""]
    if second_hits[both[0]][1][2] < second_hits[both[1]][1][2]:
        second_hits[both[0]], second_hits[both[1]] = second_hits[both[1]], second_hits[both[0]]
    scripted = first_hits + second_hits                          # (every first hit is sent before any second one)
    now = NOW
    counted = dict(over_ask=0, empty_half=0)
    sizes = [1, 2, 3, 4] * 8 + [int(x) for x in rng.integers(5, 701, 40)]
    rng.shuffle(sizes)
    peer_rpcs = client_rpcs = errors_seen = 0
    client_invalid = False
    k = 0
    while scripted or k < len(sizes):
        n = sizes[k] if k < len(sizes) else 4
        peer = k % 3 != 2                                         # (two peer RPCs, then a client RPC; the scripted items travel in peer RPCs)
        take = [scripted.pop(0) for _ in range(min(len(scripted), n, 3))] if peer else []
        reqs = rand_reqs(rng, n - len(take), bad=(k % 2 == 0))
        for r in reqs:                                            # few keys: peer and client RPCs, stages and direct path meet on the same buckets
            if r["unique_key"].startswith("acct:"):
                r["unique_key"] = "acct:%d" % rng.integers(0, 40)
        _global_by_key(reqs)
        where = sorted(int(x) for x in rng.choice(n, len(take), replace=False)) if take else []
        for pos, t in zip(where, take):
            reqs.insert(pos, t[0])
        payload = wire_replay.pb_request(reqs, peer=peer)
        got = rig.call(payload, now, peer, wrap=bool(k & 1))
        want = rig.expected(payload, now, peer, wrap=bool(k & 1))
        assert got == want, f"RPC {k} ({'peer' if peer else 'client'}): {n} requests"
        rows = wire_replay.rows_of(got)
        assert len(rows) == n
        for pos, t in zip(where, take):
            assert rows[pos][:3] == t[1] and rows[pos][4] == "", (k, pos, t[0], rows[pos])
            if t[2]:
                counted[t[2]] += 1
        errors_seen += sum(1 for row in rows if row[4])
        if not peer:
            client_invalid = client_invalid or any(not r["name"] or not r["unique_key"] for r in reqs)
            assert not any("getLocalRateLimit" in row[4] for row in rows)
        else:
            assert all(row[4] == "" or row[4].startswith("Error in getLocalRateLimit: during workerPool.GetRateLimit: ") for row in rows)
        peer_rpcs += peer; client_rpcs += not peer
        now += int(rng.integers(0, 900))
        k += 1
    assert counted["over_ask"] >= 20 and counted["empty_half"] >= 20, counted
    assert peer_rpcs >= 30 and client_rpcs >= 15 and errors_seen > 50, (peer_rpcs, client_rpcs, errors_seen)
    st = rig.pool.stats()
    assert st["rpcs"] == k and st["host_decode_ns"] > 0          # (RPCs went through the stages and through their callers' own evaluation)
    # every key the peer RPCs made — "name_", "_ukey" and "_" among them — is a bucket; the client RPC's invalid items never reach one (the
    # oracle, handed the host transcoder's batch, gives those an empty-key bucket of their own)
    assert rig.size() == rig.o.size() - (1 if client_invalid else 0)
    rig.close()


@pytest.mark.parametrize("n_plain,with_global", CONFIGS, ids=IDS)
def test_the_draining_scenarios_table(n_plain, with_global):
    """tests/golden/peer_drain_vectors.json: forwarded GLOBAL over-asks drain, the same over-ask on the client RPC or without GLOBAL does not
    (tests/golden/global_vectors.json holds the reference's GLOBAL tests between whole instances; none of its rows is a single forwarded
    over-ask, so the table is a file of its own).  One-request RPCs (the caller's own evaluation) and the same among 7 fillers (a stage)."""
    n_checked = 0
    for pad in (0, 7):
        rig = Rig(n_plain, with_global)
        for si, sc in enumerate(scenarios.load("peer_drain_vectors.json")["scenarios"]):
            for ti, step in enumerate(sc["steps"]):
                reqs = [_req("filler", "f%d_%d_%d" % (si, ti, j), 1, behavior=2) for j in range(pad)]
                reqs.insert(pad // 2, _req("drain", "s%d" % si, step["hits"], limit=sc["limit"], duration=sc["duration"], algorithm=sc["algorithm"],
                                           behavior=step["behavior"]))
                got = rig.call(wire_replay.pb_request(reqs, peer=step["rpc"] == "peer"), NOW, step["rpc"] == "peer")
                row = wire_replay.rows_of(got)[pad // 2]
                where = f"{sc['name']} step {ti} ({sc['source']}), {pad} fillers"
                assert row[4] == "" and row[1] == sc["limit"], (where, row)
                assert (row[0], row[2]) == (step["expect"]["status"], step["expect"]["remaining"]), (where, row)
                n_checked += 1
        rig.close()
    assert n_checked >= 30


@pytest.mark.parametrize("n_plain,with_global", [(4, False), (4, True)], ids=["4_tables", "4_tables+global_engine"])
def test_peer_messages_that_are_turned_away_whole(n_plain, with_global):
    """1001 requests: GUBER_E_WIRE_TOO_LARGE (the caller answers "'PeerRequest.rate_limits' list too large", gubernator.go:465); a truncated
    message, short (its caller's own evaluation) and long (a stage): GUBER_E_WIRE_MALFORMED; nothing of either reaches a bucket"""
    rng = np.random.default_rng(9)
    rig = Rig(n_plain, with_global)
    rig.pool.set_clock(NOW)
    good = wire_replay.pb_request(_global_by_key(rand_reqs(rng, 50, bad=True)), peer=True)
    with pytest.raises(ga.GuberError) as ei:
        rig.pool.get_peer_rate_limits(wire_replay.pb_request(_global_by_key(rand_reqs(rng, 1001, bad=True)), peer=True))
    assert ei.value.code == -21
    for cut in (good[:-3], wire_replay.pb_request([_req("", "x", 1, behavior=2)], peer=True)[:-2]):
        with pytest.raises(ga.GuberError) as ei:
            rig.pool.get_peer_rate_limits(cut)
        assert ei.value.code == -20
    assert rig.size() == 0
    assert len(wire_replay.rows_of(rig.pool.get_peer_rate_limits(good))) == 50 and rig.size() > 0
    rig.close()


def test_unusual_but_valid_peer_messages_get_the_peer_transcoders_bytes():
    """tests/wire_shapes.py's well-formed payloads (unknown fields, groups, padded lengths; tests/test_gpu_wire_pool.py has the client RPC)
    through guber_wire_pool_get_peer_rate_limits with the default response buffer — among them the 300 requests of limit 2^62 behind an
    empty group, whose answers are longer than the request: the peer transcoder's bytes around the oracle, one row per top-level record"""
    rng = np.random.default_rng(77)
    rig = Rig(4, False)
    shapes = wire_shapes.well_formed()
    assert wire_shapes.GROUP_LED_300 in dict(shapes)
    now = NOW
    for k in rng.permutation(len(shapes)):
        label, payload = shapes[int(k)]
        try:
            got = rig.call(payload, now, True)
        except ga.GuberError as e:
            pytest.fail(f"{label}: turned away with {e.code} ({e})")
        assert got == rig.expected(payload, now, True), label
        assert len(wire_replay.rows_of(got)) == wire_shapes.n_records(label), label
        now += int(rng.integers(0, 900))
    assert rig.size() == rig.o.size()                            # (no validation on this path: "ws_" is a bucket like any other)
    rig.close()


def _broadcast(keys, rng, now):
    """UpdatePeerGlobalsReq of token and leaky globals + the CacheItems UpdatePeerGlobals makes of them (gubernator.go:428-451), built by hand"""
    m = PB["UpdatePeerGlobalsReq"]()
    items = []
    for i, key in enumerate(keys):
        algo = i & 1
        limit = int(rng.integers(5, 200)); remaining = int(rng.integers(0, limit + 1)); duration = int(rng.choice([60_000, 3_600_000]))
        status = int(remaining == 0 and algo == 0)
        reset = now + int(rng.integers(1000, duration))
        g = m.globals.add(key=key, algorithm=algo, duration=duration, created_at=now - 5)
        g.status.status = status; g.status.limit = limit; g.status.remaining = remaining; g.status.reset_time = reset
        if algo == 1:
            items.append(support.make_item(key, 1, limit=limit, duration=duration, remaining_f=float(remaining), burst=limit, stamp=now, expire_at=reset))
        else:
            items.append(support.make_item(key, 0, status=status, limit=limit, duration=duration, remaining=remaining, stamp=now, expire_at=reset))
    reads = []
    for i, (key, g) in enumerate(zip(keys, m.globals)):
        name, uk = key.split("_", 1)
        reads.append(_req(name, uk, 0, limit=g.status.limit, duration=g.duration, algorithm=g.algorithm, behavior=2))
    return m.SerializeToString(), items, reads


@pytest.mark.parametrize("n_plain,with_global", CONFIGS, ids=IDS)
def test_update_peer_globals_installs_a_broadcast_beside_traffic(n_plain, with_global):
    """a broadcast of 600 token and leaky globals: afterwards a hits = 0 read of every key — through the peer RPC and through the client RPC —
    says what the oracle says after the same CacheItems went through its cache-add entry (LRUCache.Add, as AddCacheItem does).  A malformed
    broadcast, and one with a global no table can hold, install nothing.  Then a second broadcast in four messages WHILE eight threads send
    peer and client RPCs into the same tables: the threads' keys keep per-key conservation (as tests/test_gpu_wire_pool.py's concurrent test:
    token bucket, hits 1, limit 40), and the second broadcast's keys read as the oracle's."""
    rng = np.random.default_rng(57 + n_plain + 7 * with_global)
    rig = Rig(n_plain, with_global, stages=3, max_items=8192, max_payload_bytes=1 << 20, max_rpcs=64, batch_wait_us=300)
    now = NOW
    rig.pool.set_clock(now)
    msg, items, reads = _broadcast(["upg_%d" % i for i in range(600)], rng, now)
    # turned away whole: truncated; an empty key among good ones; a key longer than the tables hold
    before = rig.size()
    for bad, code in ((msg[:-3], -20),):
        with pytest.raises(ga.GuberError) as ei:
            rig.pool.update_peer_globals(bad)
        assert ei.value.code == code
    for key, code in (("", -1), ("x" * 300, -7)):
        m = PB["UpdatePeerGlobalsReq"]()
        m.ParseFromString(msg)
        m.globals[len(m.globals) // 2].key = key
        with pytest.raises(ga.GuberError) as ei:
            rig.pool.update_peer_globals(m.SerializeToString())
        assert ei.value.code == code
    assert rig.size() == before == 0
    assert rig.pool.update_peer_globals(b"") == 0
    assert rig.pool.update_peer_globals(msg) == 600
    assert rig.size() == 600
    if with_global:
        assert rig.engs[rig.global_engine].size() == 600         # GLOBAL state lives in the GLOBAL engine
    elif n_plain > 1:
        assert min(e.size() for e in rig.engs) > 0               # ... or where XXH64 of the key says
    for it in items:
        rig.o.add_item(it, now)
    rows = wire_replay.rows_of(rig.call(wire_replay.pb_request(reads, peer=True), now, True))
    m = PB["UpdatePeerGlobalsReq"]()
    m.ParseFromString(msg)
    assert [(r[1], r[2], r[4]) for r in rows] == [(g.status.limit, g.status.remaining, "") for g in m.globals]   # (at the instant of the install: not only through the oracle)
    rig.expected(wire_replay.pb_request(reads, peer=True), now, True)        # (the oracle sees every RPC the pool sees)
    for peer in (True, False):
        now += 700                                                # (leaky buckets have leaked meanwhile)
        payload = wire_replay.pb_request(reads, peer=peer)
        assert rig.call(payload, now, peer) == rig.expected(payload, now, peer), "reads through the %s RPC" % ("peer" if peer else "client")
    # ---- the second broadcast beside eight callers
    CALLERS, RPCS, ITEMS, KEYS, LIMIT = 8, 12, 200, 8 * 70, 40
    plans = []
    for t in range(CALLERS):
        trng = np.random.default_rng(500 + t)
        mine = []
        for q in range(RPCS):
            ks = trng.integers(0, KEYS, ITEMS)
            reqs = [_req("conc", "k%04d" % k, 1, limit=LIMIT, behavior=2) for k in ks]
            mine.append((ks, bool((q + t) & 1), wire_replay.pb_request(reqs, peer=bool((q + t) & 1))))
        plans.append(mine)
    parts = [_broadcast(["upg2_%d" % i for i in range(150 * b, 150 * (b + 1))], rng, now) for b in range(4)]
    raw = [[None] * RPCS for _ in range(CALLERS)]
    failures = []
    start = threading.Barrier(CALLERS + 1)

    def caller(t):
        try:
            start.wait()
            for q, (_, peer, payload) in enumerate(plans[t]):
                raw[t][q] = rig.pool.get_peer_rate_limits(payload) if peer else rig.pool.get_rate_limits(payload)
        except Exception as e:  # noqa: BLE001
            failures.append((t, repr(e)))

    th = [threading.Thread(target=caller, args=(t,)) for t in range(CALLERS)]
    for x in th:
        x.start()
    start.wait()
    installed = sum(rig.pool.update_peer_globals(p[0]) for p in parts)
    for x in th:
        x.join()
    assert not failures, failures[:3]
    assert installed == 600
    admitted = np.zeros(KEYS, np.int64); refused = np.zeros(KEYS, np.int64); sum_rem = np.zeros(KEYS, np.int64)
    for t in range(CALLERS):
        for q, (ks, _, _) in enumerate(plans[t]):
            rows = wire_replay.rows_of(raw[t][q])
            assert len(rows) == ITEMS
            for kk, (status, limit, remaining, _, error) in zip(ks, rows):
                assert error == "" and limit == LIMIT and status in (0, 1)
                if status == 0:
                    admitted[kk] += 1; sum_rem[kk] += remaining
                else:
                    refused[kk] += 1
                    assert remaining == 0
    assert (admitted <= LIMIT).all()
    assert (sum_rem == admitted * LIMIT - admitted * (admitted + 1) // 2).all()      # the i-th admitted hit left LIMIT - i
    assert (admitted[refused > 0] == LIMIT).all()
    assert admitted.sum() + refused.sum() == CALLERS * RPCS * ITEMS
    assert rig.size() == 600 + 600 + int((admitted > 0).sum())
    o2 = support.Oracle(cache_size=1 << 20)                      # (the second broadcast's keys alone: the threads' traffic has no serial order to replay)
    rig.o.close(); rig.o = o2
    for p in parts:
        for it in p[1]:
            o2.add_item(it, now)
    for peer in (True, False):
        payload = wire_replay.pb_request([r for p in parts for r in p[2]], peer=peer)
        assert rig.call(payload, now, peer) == rig.expected(payload, now, peer), "second broadcast, reads through the %s RPC" % ("peer" if peer else "client")
    rig.close()


def test_the_peer_handlers_call_sequence_in_plain_c99(tmp_path):
    """tests/hostsim/peer_abi_c99.c makes the calls go/wire_server.go's getPeerRateLimits and updatePeerGlobals handlers make, with the
    binding's casts: gcc -std=c99 -pedantic -Werror takes it, it links against the product library and its answers are checked field by field"""
    exe = str(tmp_path / "peer_abi_c99")
    libdir = os.path.join(support.ROOT, "gubernator_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(support.ROOT, "include"), "-o", exe,
                    os.path.join(support.ROOT, "tests", "hostsim", "peer_abi_c99.c"), "-L", libdir, "-lguber_hip", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe, "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "peer handlers ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
