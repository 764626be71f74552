"""Scenarios for guber_wire_dev_eval_mesh_enc (gubernator_amd/csrc/guber_wire_dev.h): serialized GetRateLimitsReq payloads in at any rank of a
mesh, serialized GetRateLimitsResp bytes out — encoded on the device by k_wire_enc_owner (guber_kernels_wire.h) — with
metadata{"owner": <the owner's address>} on every answer another rank owns (k_mx_count's item_owner[], guber_kernels_mesh.h).  Shared by
tests/test_gpu_mesh_enc.py (the product library, every rank a logical rank of device 0) and tests/test_mesh_enc_cpu.py (the same host code
and kernels compiled for the CPU).

The expected bytes come from the protobuf runtime (tests/pb_schema.py: RateLimitResp with metadata["owner"]) out of three sources: the
per-rank oracles' answers under the mesh's order rule (mesh_cases.World's recipe, restated in EncWorld.expected because items with a forced
error are kept from the oracles: the oracle takes its calendar intervals from the host), the host ring's owners (Ring.route), and the texts
of include/guber_wire.h, written out here.

Cases (the letters are the issue's): a sizes around the encoder's piece, b the eight address lengths, c every class of item in one RPC,
d item errors, e a malformed payload between two good ones, r refusals."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):         # (run as a script by tests/test_mesh_enc_cpu.py)
    if _p not in sys.path:
        sys.path.insert(0, _p)
import mesh_cases as mc
import mesh_rows_cases as mr
from mesh_cases import LONG_MS, NOW0, STEP_MS, Gen, by_ids, draw
from gubernator_amd.abi import HostBatch
from pb_schema import PB

GLOBAL, GREGORIAN = 2, 4
E_ALGO, E_GREG, E_EMPTY, E_TOO_LONG = 1, 3, 4, 7
GREG = "behavior DURATION_IS_GREGORIAN is set; but `Duration` is not a valid gregorian interval"
ALGO = "Invalid rate limit algorithm '7'"
TOO_LONG = "rate limit key too long"
LOCAL = "Error in getLocalRateLimit: during workerPool.GetRateLimit: "
GLOBAL_PREFIX = "Error in getGlobalRateLimit: during in getLocalRateLimit: during workerPool.GetRateLimit: "
ADDR_LENS = (1, 11, 100, 118, 119, 127, 128, 264)
FILL = 0xEE
TAIL = 64
I64_MAX = (1 << 63) - 1


def addr_of(n, r):
    """an address of exactly n bytes that names rank r"""
    return (("%x" % r) + "h" * n)[:max(n - 5, 0)] + (":808%x" % r)[-min(n, 5):]


def eval_detail(decoders, mesh, owner_addr, wrap_errors=True, cap_delta=0):
    """guber_wire_dev_eval_mesh_enc through ctypes with buffers of the tests' making: every rank's buf is its bound + cap_delta bytes (cap
    says so) followed by TAIL more, all FILL before the call.  -> per rank (responses, owner_rank, (buf, off, len, bound))"""
    import ctypes as C
    from gubernator_amd import wire as gw
    L = gw._lib()
    L.guber_wire_dev_eval_mesh_enc.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(gw.MeshResp)]
    W = len(decoders)
    addrs, arr = gw._addr_array(owner_addr)
    decs = (C.c_void_p * W)(*[d.h if d is not None else None for d in decoders])
    out, keep = (gw.MeshResp * W)(), []
    for r, d in enumerate(decoders):
        nrpc, n = (getattr(d, "nrpc", 0), getattr(d, "n", 0)) if d is not None else (0, 0)
        bound = gw.mesh_enc_bound(d, addrs) if d is not None else 0
        cap = max(bound + cap_delta, 0)
        buf = np.full(max(cap + TAIL, 1), FILL, np.uint8)
        off, ln, own = np.zeros(max(nrpc, 1), np.uint32), np.zeros(max(nrpc, 1), np.uint32), np.full(max(n, 1), 0xFF, np.uint8)
        out[r] = gw.MeshResp(buf.ctypes.data, cap, off.ctypes.data, ln.ctypes.data, own.ctypes.data)
        keep.append((buf, off, ln, own, nrpc, n, bound))
    rc = L.guber_wire_dev_eval_mesh_enc(decs, mesh.h, arr, 1 if wrap_errors else 0, out)
    if rc:
        raise gw.GuberError(rc, gw.lib().guber_last_error().decode())
    return [([bytes(buf[int(off[q]):int(off[q]) + int(ln[q])]) for q in range(nrpc)], own[:n].copy(), (buf, off[:nrpc], ln[:nrpc], bound))
            for buf, off, ln, own, nrpc, n, bound in keep]


class _NamedRing:
    """the package with Ring() taking the case's peer names: RowsWorld names its peers itself"""

    def __init__(self, ga, names):
        self._ga, self._names = ga, names

    def __getattr__(self, k):
        return getattr(self._ga, k)

    def Ring(self, names, *a):
        assert len(names) == len(self._names)
        return self._ga.Ring(self._names, *a)


def mark(g, i, name=None, ukey=None, force=0):
    """request i of a generation: its name / unique_key as the payload carries them (a rejected item's key is empty for the world), or an
    error forced on it: E_GREG (DURATION_IS_GREGORIAN with a duration that is no interval), E_ALGO (algorithm 7)"""
    if not hasattr(g, "names"):
        g.names, g.force = {}, {}
    if name is not None:
        g.names[i] = (name, ukey)
        g.keys[i] = b""
        g.hits[i], g.limit[i], g.duration[i], g.algorithm[i], g.behavior[i] = 1, 10, LONG_MS, 0, g.behavior[i] & GLOBAL
    if force == E_GREG:
        g.force[i] = E_GREG
        g.behavior[i] |= GREGORIAN
        g.duration[i] = 99
    elif force == E_ALGO:
        g.force[i] = E_ALGO
        g.algorithm[i] = 7


def item_of(g, i):
    it = mr.item_of(g, i)
    if i in getattr(g, "names", {}):
        it["name"], it["unique_key"] = g.names[i]
    return it


class EncWorld(mr.RowsWorld):
    """RowsWorld through the wire with the ring's peers named `addrs`, and call() through eval_mesh_enc"""

    def __init__(self, ga, support, addrs, **kw):
        self.addrs = list(addrs)
        super().__init__(_NamedRing(ga, self.addrs), support, form="wire", **kw)
        self.support = support

    def expected(self, gens):
        """mesh_cases.World.expected with the forced errors kept from the oracles: -> (answers per rank, forwarded, (owner, stay, kind) per rank)"""
        W = self.W
        routed = [self.route(g) for g in gens]
        want = [dict(status=np.zeros(g.n, np.uint8), err=np.zeros(g.n, np.uint8), limit=np.zeros(g.n, np.int64), remaining=np.zeros(g.n, np.int64),
                     reset_time=np.zeros(g.n, np.int64)) for g in gens]
        forwarded = 0
        forced = [np.zeros(g.n, bool) for g in gens]
        for s, (g, (owner, stay, kind)) in enumerate(zip(gens, routed)):
            dest = np.where(stay, s, owner)
            for o in range(W):
                self.pairs[s, o] += int((dest == o).sum())
            forwarded += int((dest != s).sum())
            for i in np.nonzero(kind)[0]:
                row = self.errors["empty" if kind[i] == 1 else "too_long"]
                for name, v in zip(mr.NAMES, row):
                    want[s][name][i] = v
            for i, code in getattr(g, "force", {}).items():
                assert kind[i] == 0
                forced[s][i] = True
                want[s]["err"][i] = code
            for i in np.nonzero((kind == 0) & ~forced[s])[0]:
                assert self.seen[int(dest[i])].setdefault(g.keys[i], bool(g.behavior[i] & GLOBAL)) == bool(g.behavior[i] & GLOBAL)
        for o in range(W):
            keys, cols, back = [], {k: [] for k in ("hits", "limit", "duration", "algorithm", "behavior", "burst", "created_at", "is_owner")}, []
            for s, (g, (owner, stay, kind)) in enumerate(zip(gens, routed)):
                sel = np.nonzero((np.where(stay, s, owner) == o) & (kind == 0) & ~forced[s])[0]
                keys += [g.keys[i] for i in sel]
                for name in ("hits", "limit", "duration", "algorithm", "behavior"):
                    cols[name].append(getattr(g, name)[sel])
                cols["burst"].append(np.zeros(len(sel), np.int64) if g.burst is None else g.burst[sel])
                cols["created_at"].append(np.full(len(sel), g.now, np.int64) if g.created_at is None else g.created_at[sel])
                cols["is_owner"].append(np.where(stay[sel], owner[sel] == s, True).astype(np.uint8))
                back += [(s, int(i)) for i in sel]
            if not keys:
                continue
            c = {k: np.concatenate(v) for k, v in cols.items()}
            res = self.oracles[o].eval(HostBatch(keys, c["hits"], c["limit"], c["duration"], gens[0].now, burst=c["burst"], created_at=c["created_at"],
                                                 algorithm=c["algorithm"], behavior=c["behavior"], is_owner=c["is_owner"]))
            for j, (s, i) in enumerate(back):
                for name in mr.NAMES:
                    want[s][name][i] = getattr(res, name)[j]
        return want, forwarded, routed

    def response(self, g, r, a, b, want, owner, kind, wrap):
        """the GetRateLimitsResp of items [a, b) of rank r's generation, by the table of include/guber_wire.h"""
        m = PB["GetRateLimitsResp"]()
        for i in range(a, b):
            x = m.responses.add()
            it = item_of(g, i)
            key = it["name"] + "_" + it["unique_key"]
            err = int(want["err"][i])
            remote = kind[i] == 0 and int(owner[i]) != r
            glob = bool(g.behavior[i] & GLOBAL)
            if not it["unique_key"]:
                assert err == E_EMPTY
                x.error = "field 'unique_key' cannot be empty"
            elif not it["name"]:
                assert err == E_EMPTY
                x.error = "field 'namespace' cannot be empty"
            elif err:
                text = {E_GREG: GREG, E_ALGO: ALGO, E_TOO_LONG: TOO_LONG}[err]
                if remote:
                    word = ("Error in leakyBucket: " if g.algorithm[i] == 1 else "Error in tokenBucket: ") if err == E_GREG else ""
                    x.error = (GLOBAL_PREFIX if glob else LOCAL) + word + text
                else:
                    x.error = f"Error while apply rate limit for '{key}': {text}" if wrap else text
            else:
                x.status, x.limit, x.remaining, x.reset_time = (int(want[k][i]) for k in ("status", "limit", "remaining", "reset_time"))
            if remote:
                x.metadata["owner"] = self.addrs[int(owner[i])]
        return m

    def call(self, gens, sizes, label, wrap=True, no_decoder=(), junk=None, host_rpcs=None):
        """one guber_wire_dev_eval_mesh_enc.  gens[r]: rank r's generation (None: nothing arrived; its decoder decodes nothing — or, r in
        no_decoder, it has none); sizes[r]: the items of its RPCs, in order; junk: {r: {q: bytes}} a payload the decode turns away, put in
        front of RPC q.  Checks the bytes per RPC, owner_rank, the forwarded count, the regions and the sentinel bytes, and host_rpcs[r]
        (the RPCs of rank r the host transcoder wrote) where given.  -> (messages per rank per RPC, the call's detail)"""
        import wire_replay
        from gubernator_amd import wire as gw
        now = next(g.now for g in gens if g is not None)
        gens = [g if g is not None else Gen([], now) for g in gens]
        decs, status_want, spans, places = [], [], [], {}
        for r, g in enumerate(gens):
            assert sum(sizes[r]) == g.n, (label, r)
            if r in no_decoder:
                assert g.n == 0
                decs.append(None); status_want.append([]); spans.append([])
                continue
            payloads, st, sp, at, slots = [], [], [], 0, []
            for q, k in enumerate(sizes[r]):
                if junk and q in junk.get(r, {}):
                    bad, dead = junk[r][q] if isinstance(junk[r][q], tuple) else (junk[r][q], 0)
                    payloads.append(bad); st.append(gw.E_WIRE_MALFORMED); sp.append(None)
                    slots += [-1] * dead                           # (dead slots: they keep their places in the batch, empty keys)
                slots += list(range(at, at + k))
                payloads.append(wire_replay.pb_request([item_of(g, i) for i in range(at, at + k)]))
                st.append(0); sp.append((at, at + k))
                at += k
            status, first, count, n = self.decs[r].decode(payloads, now, max_per_rpc=4096)
            assert n == len(slots) and status.tolist() == st, (label, r, n, len(slots), status)
            decs.append(self.decs[r]); status_want.append(st); spans.append(sp); places[r] = np.array(slots, np.int64)
        before = self.mesh.stats()
        res = eval_detail(decs, self.mesh, self.addrs, wrap_errors=wrap)
        after = self.mesh.stats()
        want, forwarded, routed = self.expected(gens)
        msgs = []
        for r, g in enumerate(gens):
            resp, own, (buf, off, ln, bound) = res[r]
            owner, stay, kind = routed[r]
            assert len(resp) == len(spans[r]), (label, r)
            at = places.get(r, np.zeros(0, np.int64))
            assert len(own) == len(at) and (own[at < 0] == 0xFF).all(), f"{label}: rank {r}: a dead slot has an owner"
            assert np.array_equal(own[at >= 0], np.where(kind == 0, owner, 0xFF).astype(np.uint8)), f"{label}: rank {r}: owner_rank is not the host ring's"
            out, end = [], 0
            for q, sp in enumerate(spans[r]):
                assert int(off[q]) == end, f"{label}: rank {r} RPC {q}: the responses are not back to back"
                if sp is None:
                    assert ln[q] == 0 and resp[q] == b"", f"{label}: rank {r} RPC {q}: a payload that was turned away has an answer"
                    out.append(None)
                    continue
                m = self.response(g, r, sp[0], sp[1], want[r], owner, kind, wrap)
                assert resp[q] == m.SerializeToString(), f"{label}: rank {r} RPC {q} ({sp[1] - sp[0]} items): the bytes differ"
                end += int(ln[q])
                out.append(m)
            assert end <= bound and (buf[end:] == FILL).all() and len(buf) == max(bound + TAIL, 1), f"{label}: rank {r}: a byte behind the responses changed"
            if host_rpcs is not None and decs[r] is not None:
                assert gw.mesh_enc_host_rpcs(decs[r]) == host_rpcs[r], (label, r, gw.mesh_enc_host_rpcs(decs[r]), host_rpcs[r])
            msgs.append(out)
        assert after["calls"] - before["calls"] == 1 and after["requests"] - before["requests"] == sum(len(x) for x in places.values()), (label, before, after)
        assert after["forwarded"] - before["forwarded"] == forwarded, (label, after["forwarded"] - before["forwarded"], forwarded)
        self.calls += 1
        return msgs, res


class TwinWorld(mr.RowsWorld):
    """RowsWorld through the wire (guber_wire_dev_eval_mesh) over a ring of the same peer names"""

    def __init__(self, ga, support, addrs, **kw):
        super().__init__(_NamedRing(ga, list(addrs)), support, form="wire", **kw)


def enc_world(make_world, addrs, **kw):
    return make_world(cls=EncWorld, addrs=addrs, **kw)


def owned(w, pop):
    """the population's indices by owning rank"""
    owner = w.ring.route(Gen(pop, NOW0).packed())
    return [np.nonzero(owner == o)[0] for o in range(w.W)]


# ---- a: sizes ---------------------------------------------------------------------------------------------------------------------------
def case_a(make_world):
    """a: W = 3, RPCs of 0, 1, 3, 4, 5, 63, 64, 65, P - 1, P, P + 1 and 2 P + 1 items mixed across the ranks of a call (every call holds all
    twelve, moving one rank on from call to call), a rank without a decoder, a decoder that decoded nothing, a dozen calls over one
    population so that buckets run out; the bytes per RPC, owner_rank, forwarded, the regions and sentinels (EncWorld.call); then sizes and
    held keys against a twin world driven through eval_mesh"""
    from gubernator_amd import wire as gw
    P = gw.mesh_enc_piece()
    S = [0, 1, 3, 4, 5, 63, 64, 65, P - 1, P, P + 1, 2 * P + 1]
    addrs = [addr_of(11, r) for r in range(3)]
    w = enc_world(make_world, addrs, W=3, n_engines=2, max_n=1024)
    twin = make_world(cls=TwinWorld, addrs=addrs, W=3, n_engines=2, max_n=1024)
    pop, rng = w.spread(8, 200), np.random.default_rng(71)       # (consecutive numbers belong to a handful of owners: RowsWorld.spread)
    over = 0
    for c in range(12):
        now = NOW0 + c * STEP_MS
        sizes = [[S[(c + 3 * k + r) % 12] for k in range(4)] for r in range(3)]
        no_decoder = ()
        if c % 4 == 1:
            sizes[c % 3], no_decoder = [], (c % 3,)                 # nothing arrived, and there is no decoder
        elif c % 4 == 3:
            sizes[c % 3] = []                                      # a decoder that decoded nothing
        gens = [by_ids(pop, draw(rng, sum(s), len(pop)), now, c, full=(c + r) % 4 == 1, rng=rng) if sum(s) else None for r, s in enumerate(sizes)]
        msgs, _ = w.call(gens, sizes, f"a call {c} sizes {sizes}", no_decoder=no_decoder, host_rpcs=[0, 0, 0])
        over += sum(x.status for out in msgs for m in out if m is not None for x in m.responses)
        twin.call(gens, f"a twin call {c}")
    assert over > 100, over                                        # (buckets ran out)
    assert w.sizes() == twin.sizes() and w.held() == twin.held()
    w.assert_every_pair_used("a")
    w.check_residency("a")
    twin.close()
    w.close()


# ---- b: address lengths -----------------------------------------------------------------------------------------------------------------
def case_b(make_world):
    """b: W = 8, addresses of 1, 11, 100, 118, 119, 127, 128 and 264 bytes, one per rank; every rank receives items every other rank owns.
    Two keys of rank 2 (the 100-byte address: a suffix of 111 bytes) have limits 2^21 and 2^21 + 5: with a reset_time of six varint bytes
    their answers' fields take 16 and 17 bytes — bodies of 127 and 128; int64 limits 2^63 - 1 and -1 on keys of their own"""
    addrs = [addr_of(n, r) for r, n in enumerate(ADDR_LENS)]
    assert [len(a) for a in addrs] == list(ADDR_LENS) and len(set(addrs)) == 8
    w = enc_world(make_world, addrs, W=8, n_engines=1, max_n=512)
    pop = w.spread(8, 40)
    mine = owned(w, pop)
    assert min(len(x) for x in mine) >= 20
    rng = np.random.default_rng(72)
    k127, k128 = int(mine[2][0]), int(mine[2][1])
    extreme = {int(mine[o][2]): I64_MAX for o in range(8)}
    extreme.update({int(mine[o][3]): -1 for o in range(8)})
    bodies = set()
    for c in range(2):
        now = NOW0 + c * STEP_MS
        gens, sizes = [], []
        for r in range(8):
            ids = np.concatenate([[k127, k128], rng.permutation(list(extreme)), np.concatenate([rng.choice(m[4:], 12) for m in mine])])
            g = by_ids(pop, ids, now, 0)
            for i, k in enumerate(ids):
                if k == k127:
                    g.limit[i], g.algorithm[i] = 1 << 21, 0
                elif k == k128:
                    g.limit[i], g.algorithm[i] = (1 << 21) + 5, 0
                elif k in extreme:
                    g.limit[i], g.algorithm[i] = extreme[k], 0
            gens.append(g); sizes.append([5, g.n - 5])
        msgs, _ = w.call(gens, sizes, f"b call {c}", host_rpcs=[0] * 8)
        for r in range(8):
            if r != 2:
                bodies |= {x.ByteSize() for x in msgs[r][0].responses[:2]}
            seen = {x.metadata["owner"] for m in msgs[r] for x in m.responses if x.metadata}
            assert seen == set(addrs) - {addrs[r]}, (c, r)
    assert {127, 128} <= bodies, bodies
    w.assert_every_pair_used("b")
    w.close()


# ---- c: classes in one RPC --------------------------------------------------------------------------------------------------------------
def class_gen(w, pop, mine, r, now, rejected, salt):
    """a local item, a forwarded item, a GLOBAL item at its owner, a GLOBAL item at a non-owner (GLOBAL keys are numbers 10.. of every owner's
    keys, plain ones 0..9) and, `rejected`, an empty unique_key, an empty name and an over-long key, around a few plain items"""
    o = (r + 1) % w.W
    ids = [int(mine[r][salt % 10]), int(mine[o][salt % 10]), int(mine[r][10 + salt % 10]), int(mine[o][10 + salt % 10])] + [int(mine[(r + 2) % w.W][k]) for k in range(3)]
    g = by_ids(pop, np.array(ids + ([ids[0]] * 3 if rejected else [])), now, 0)
    g.behavior[2] = g.behavior[3] = GLOBAL
    if rejected:
        mark(g, 7, "k", "")
        mark(g, 8, "", "u")
        g.keys[9] = b"k_" + b"x" * (w.max_key - 1)                 # one byte more than the engines' max_key_bytes
        g.hits[9], g.limit[9], g.duration[9], g.algorithm[9], g.behavior[9] = 1, 10, LONG_MS, 0, 0
    return g


def case_c(make_world):
    """c: a world with a GLOBAL engine.  One RPC per rank mixes a local item, a forwarded one, a GLOBAL item at its owner, a GLOBAL item at a
    non-owner, an empty unique_key, an empty name and a key of max_key_bytes + 1: the rejected items are item errors, so the RPC is the
    host transcoder's (asserted) and its bytes are right; the same classes without the rejected items, in the same decode, are the device's"""
    addrs = [addr_of(n, r) for r, n in enumerate((11, 100, 128))]
    w = enc_world(make_world, addrs, W=3, n_engines=1, max_n=256, with_global=True)
    pop = w.spread(8, 40)
    mine = owned(w, pop)
    for c, wrap in enumerate((True, False)):
        now = NOW0 + c * STEP_MS
        gens, sizes = [], []
        for r in range(3):
            a, b = class_gen(w, pop, mine, r, now, True, c), class_gen(w, pop, mine, r, now, False, c + 5)
            g = Gen(a.keys + b.keys, now, hits=np.concatenate([a.hits, b.hits]), limit=np.concatenate([a.limit, b.limit]), duration=np.concatenate([a.duration, b.duration]),
                    algorithm=np.concatenate([a.algorithm, b.algorithm]), behavior=np.concatenate([a.behavior, b.behavior]))
            g.names, g.force = dict(a.names), {}
            gens.append(g); sizes.append([a.n, b.n])
        msgs, res = w.call(gens, sizes, f"c call {c} wrap {wrap}", wrap=wrap, host_rpcs=[1, 1, 1])
        for r in range(3):
            first, second = msgs[r]
            assert [bool(x.metadata) for x in first.responses] == [False, True, False, True, True, True, True, False, False, False], (c, r)
            assert [bool(x.error) for x in first.responses] == [False] * 7 + [True] * 3
            assert [bool(x.metadata) for x in second.responses] == [False, True, False, True, True, True, True] and not any(x.error for x in second.responses)
            assert res[r][1].tolist()[7:10] == [0xFF] * 3
    for r in range(3):
        assert w.engs[r][1].size() > 0                             # (the GLOBAL engine holds the GLOBAL keys of both kinds)
    w.check_residency("c")
    w.close()


# ---- d: errors --------------------------------------------------------------------------------------------------------------------------
def case_d(make_world):
    """d: one RPC per error shape — a forwarded, a local and a GLOBAL-non-owner Gregorian-invalid item (token and leaky in turn), a forwarded
    invalid algorithm — among error-free items, in an RPC of P + 1 items (the encoder looks first) and in one of 5; the two other RPCs of
    the same decode stay on the device"""
    from gubernator_amd import wire as gw
    P = gw.mesh_enc_piece()
    addrs = [addr_of(n, r) for r, n in enumerate((11, 119, 264))]
    w = enc_world(make_world, addrs, W=3, n_engines=1, max_n=512, with_global=True)
    pop = w.spread(8, 60)
    mine = owned(w, pop)
    rng = np.random.default_rng(74)
    shapes = [("forwarded gregorian", 1, 0, E_GREG), ("local gregorian", 0, 0, E_GREG), ("global non-owner gregorian", 1, GLOBAL, E_GREG), ("forwarded algorithm", 1, 0, E_ALGO)]
    for c, (name, hop, glob, code) in enumerate(shapes):
        for wrap in (True, False):
            now = NOW0 + (2 * c + wrap) * STEP_MS
            r0 = c % 3
            gens, sizes, hosts = [], [], []
            for r in range(3):
                sz = [P + 1, 5, 64, 5] if r == r0 else [5, 64]
                ids = np.concatenate([rng.choice(m[:30], sum(sz) // 3 + 1) for m in mine])[:sum(sz)]
                g = by_ids(pop, rng.permutation(ids), now, 0)
                if r == r0:
                    for at in (P // 2 + c, P + 1 + 3):             # inside the second piece's neighbourhood; the fourth of five
                        g.keys[at] = pop[int(mine[(r + hop) % 3][40 + c])]     # (a key of its own: keys 40.. are not drawn above)
                        g.algorithm[at] = (c + at) % 2
                        g.behavior[at] = glob
                        mark(g, at, force=code)
                gens.append(g); sizes.append(sz); hosts.append(2 if r == r0 else 0)
            msgs, _ = w.call(gens, sizes, f"d {name} wrap {wrap}", wrap=wrap, host_rpcs=hosts)
            errs = [x.error for m in msgs[r0] for x in m.responses if x.error]
            assert len(errs) == 2 and all((GLOBAL_PREFIX if glob else LOCAL if hop else "") in e for e in errs), errs
            if hop:
                assert all(x.metadata["owner"] == addrs[(r0 + 1) % 3] for m in msgs[r0] for x in m.responses if x.error)
    w.close()


# ---- e: a malformed payload between two good ones ------------------------------------------------------------------------------------------
def case_e(make_world):
    """e: a payload the decode turns away between two good ones — one malformed in its framing, one whose third record's body is malformed
    (its three items stay as dead slots in the batch) — len 0 for it, the neighbours' bytes are right (and back to back), the dead slots
    have owner 0xFF and are counted by the bound"""
    addrs = [addr_of(11, r) for r in range(2)]
    w = enc_world(make_world, addrs, W=2, n_engines=1, max_n=256)
    pop, rng = w.spread(8, 100), np.random.default_rng(75)
    import wire_replay
    bad = b"\x0a\x05abc"                                           # a record that says five bytes and has three
    # two records that parse and a third whose body ends inside a varint: the framing is good, so the decode has placed three items by
    # the time it turns the payload away — dead slots: no key, no owner, a gap in the batch in front of the next RPC's items
    part = (wire_replay.pb_request([dict(name="k", unique_key="dead%d" % i, hits=1, limit=10, duration=LONG_MS, algorithm=0, behavior=0) for i in range(2)])
            + b"\x0a\x02\x18\x80", 3)
    for c in range(2):
        now = NOW0 + c * STEP_MS
        gens = [by_ids(pop, draw(rng, 69, len(pop)), now, c) for _ in range(2)]
        msgs, res = w.call(gens, [[5, 64], [64, 5]], f"e call {c}", junk={0: {1: bad if c else part}, 1: {0: part if c else bad}}, host_rpcs=[0, 0])
        assert [m is None for m in msgs[0]] == [False, True, False] and [m is None for m in msgs[1]] == [True, False, False]
        assert len(res[c][1]) == 69 + 3 and len(res[1 - c][1]) == 69
    w.close()


# ---- r: refusals ------------------------------------------------------------------------------------------------------------------------
def case_r(make_world):
    """refusals, each before anything is enqueued: an empty, an over-long and a NULL address, a cap one below the bound (GUBER_E_NOMEM), a
    decode that carried a peer RPC, two now_ms; sizes, held keys and the mesh's counters are unchanged afterwards"""
    import wire_replay
    from gubernator_amd import wire as gw
    addrs = [addr_of(11, r) for r in range(2)]
    w = enc_world(make_world, addrs, W=2, n_engines=2, max_n=64, dec_items=256)
    ga_err, E_ARG, E_NOMEM = w.ga.GuberError, w.ga.E_INVALID_ARG, w.ga.E_NOMEM
    pop = mc.population(500)
    rng = np.random.default_rng(76)
    w.call([by_ids(pop, rng.integers(0, 300, 64), NOW0, 0) for _ in range(2)], [[64], [5, 59]], "r a call that is taken")
    sizes, held, stats = w.sizes(), w.held(), w.mesh.stats()
    assert sum(map(sum, sizes)) > 0
    d0, d1 = w.decs
    now = NOW0 + STEP_MS

    def fresh(k, n=8):
        g = by_ids(pop, np.arange(300 + k * 20, 300 + k * 20 + n), now, 1)
        return [mr.item_of(g, i) for i in range(n)]

    def refused(code, label, a=addrs, **kw):
        try:
            eval_detail([d0, d1], w.mesh, a, **kw)
        except ga_err as e:
            assert e.code == code, (label, e)
        else:
            raise AssertionError(f"{label}: not refused")
        assert w.sizes() == sizes and w.held() == held and w.mesh.stats() == stats, label

    d0.decode([wire_replay.pb_request(fresh(0))], now)
    d1.decode([wire_replay.pb_request(fresh(2))], now)
    refused(E_ARG, "an empty address", [addrs[0], ""])
    refused(E_ARG, "an over-long address", ["x" * 265, addrs[1]])
    refused(E_ARG, "a NULL address", [addrs[0], None])
    refused(E_NOMEM, "a cap one below the bound", cap_delta=-1)
    d0.decode([wire_replay.pb_request(fresh(0)), wire_replay.pb_request(fresh(1), peer=True)], now, is_owner=[gw.RPC_OWNER, gw.RPC_OWNER | gw.RPC_PEER])
    refused(E_ARG, "a GUBER_WIRE_RPC_PEER payload")
    d0.decode([wire_replay.pb_request(fresh(0))], now)
    d1.decode([wire_replay.pb_request(fresh(2))], now + 1)
    refused(E_ARG, "two now_ms")
    # ... and the same decoders are taken once nothing is wrong, at exactly the bound
    d1.decode([wire_replay.pb_request(fresh(2))], now)
    res = gw.eval_mesh_enc([d0, d1], w.mesh, addrs)
    for r in range(2):
        m = PB["GetRateLimitsResp"]()
        m.ParseFromString(res[r][0][0])
        assert len(m.responses) == 8 and not any(x.error for x in m.responses)
    assert w.mesh.stats()["calls"] == stats["calls"] + 1 and sum(map(sum, w.sizes())) == sum(map(sum, sizes)) + 16
    w.close()


# ---- h: one rank ------------------------------------------------------------------------------------------------------------------------
def case_h(make_world):
    """h: W = 1 — no routing runs (k_mx_owner_one writes the owner column): RPCs around the piece with an empty unique_key and an over-long
    key among them; owner_rank is 0 or 0xFF, no answer carries metadata, the bytes are the oracle's and the engines end as a twin world's
    driven through eval_mesh"""
    from gubernator_amd import wire as gw
    P = gw.mesh_enc_piece()
    addrs = [addr_of(11, 0)]
    w = enc_world(make_world, addrs, W=1, n_engines=2, max_n=1024)
    twin = make_world(cls=TwinWorld, addrs=addrs, W=1, n_engines=2, max_n=1024)
    pop, rng = mc.population(400), np.random.default_rng(77)
    for c, sizes in enumerate(([P + 1, 5, 64], [1, 2 * P + 1], [65])):
        now = NOW0 + c * STEP_MS
        g = by_ids(pop, draw(rng, sum(sizes), len(pop)), now, c)
        hosts = (2, 1, 0)[c]                                       # (the RPCs that hold a rejected item: call 1 has both in its second)
        if c < 2:
            mark(g, 3, "k", "")
            g.keys[sizes[0] + 1] = b"k_" + b"x" * (w.max_key - 1)
            g.hits[sizes[0] + 1], g.limit[sizes[0] + 1], g.duration[sizes[0] + 1], g.algorithm[sizes[0] + 1] = 1, 10, LONG_MS, 0
        msgs, res = w.call([g], [sizes], f"h call {c}", host_rpcs=[hosts])
        own = res[0][1]
        assert set(own.tolist()) <= {0, 0xFF} and (own == 0xFF).sum() == (2 if c < 2 else 0)
        assert not any(x.metadata for m in msgs[0] for x in m.responses)
        twin.call([g], f"h twin call {c}")
    assert w.sizes() == twin.sizes() and w.held() == twin.held()
    assert w.mesh.stats()["forwarded"] == 0
    twin.close()
    w.close()


CASES = dict(h=case_h, a=case_a, b=case_b, c=case_c, d=case_d, e=case_e, r=case_r)


def world_maker(ga, support, new_engines, upload, download):
    """make_world(cls=RowsWorld, **kw) over the caller's engines"""
    def make_world(cls=mr.RowsWorld, **kw):
        return cls(ga, support, new_engines=new_engines, upload=upload, download=download, **kw)
    return make_world


# ---- the cases on the CPU build of the engine (tests/test_mesh_enc_cpu.py): GUBER_HIP_LIB=tests/hostsim/libenginesim.so python tests/mesh_enc_cases.py <letter>
def _cpu_main(letter):
    import gubernator_amd as ga
    import support
    assert "enginesim" in ga.LIB_PATH, "this entry is for the CPU build of the engine (GUBER_HIP_LIB)"

    def new_engines(rank, flags, kw):
        e0 = ga.Engine(flags=flags[0], **kw)
        return [e0] + [ga.Engine(flags=f, stream=e0.stream_handle(), **kw) for f in flags[1:]]

    CASES[letter](world_maker(ga, support, new_engines, lambda a: (a, a.ctypes.data), lambda a: a))
    print("MESH ENC CASE OK", letter)


if __name__ == "__main__":
    _cpu_main(sys.argv[1])
