"""Scenarios for key ROWS through the mesh of fronts — guber_mesh_eval_rows_dev (the row instantiations of k_mx_count / k_mx_pack,
gubernator_amd/csrc/guber_kernels_mesh.h) and guber_wire_dev_eval_mesh on top of it (guber_wire_dev.h: serialized RPC payloads decoded on the
device, routed across ranks by the ring, answered where they arrived) — shared by tests/test_gpu_mesh_rows.py (the product library, every
rank a logical rank of device 0) and tests/test_mesh_rows_cpu.py (the same host code and kernels compiled for the CPU).

The oracle side is mesh_cases': RowsWorld is mesh_cases.World — one support.Oracle per rank fed what the order rule says, the host ring,
residency — with three things of its own: the engines' max_key_bytes (the decoder's row stride is max_key_bytes rounded up to 8, plus 8: 16
gives 24, below the 32 bytes a speculative read needs; 40 gives 48; 64 gives 72), a decoder per rank, and call(), which hands the
generations over in the world's FORM:
  "packed"  guber_mesh_eval_dev, as mesh_cases.World.call
  "rows"    guber_mesh_eval_rows_dev: rank r's keys in rows of forms(call)[r] bytes (0: that rank packed).  A rows buffer is exactly
            n x stride bytes — the last row ends at the allocation's last byte — and every byte behind a key is 0xA5
  "wire"    every rank's generation as serialized GetRateLimitsReq payloads (several RPCs per rank, one of them of a single item), decoded
            by the rank's decoder, through guber_wire_dev_eval_mesh; a rank without a generation has no decoder in one call and a
            decoder that decoded nothing in the next
so mesh_cases' scenario functions run unchanged over rows and over the wire.  HashKey = name + "_" + unique_key: "k_000123" is name "k",
unique_key "000123"; an item with an empty unique_key is pre-rejected by the decoder (gubernator.go:208-212), has an empty key row and must
earn the item error a plain engine gives an empty key, in its place, without being forwarded.

Cases (the letters are the issue's): through the wire — a sizes and residency, b key widths at strides 24 and 72, c the order across
sources, d GLOBAL, e an inflow larger than the front's max_n, r refusals; rows without the wire — f rows versus packed, g mixed forms in
one call, h one rank (and, on a GPU only, h16: sixteen ranks)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):         # (run as a script by tests/test_mesh_rows_cpu.py)
    if _p not in sys.path:
        sys.path.insert(0, _p)
import mesh_cases as mc
from mesh_cases import LONG_MS, NOW0, SENTINEL_I64, SENTINEL_U8, SIZES_A, STEP_MS, TAIL, Gen, by_ids, draw, result_arrays
from gubernator_amd.abi import GuberBatch, GuberResult, HostBatch, HostResult, assert_results_equal

PAD = 0xA5
NAMES = ("status", "limit", "remaining", "reset_time", "err")


def stride_of(max_key):
    """the device wire decoder's row stride for engines of max_key_bytes = max_key"""
    return (max_key + 7) // 8 * 8 + 8


def rows_of(g, stride):
    """(rows, key_len): key i at rows[i * stride:], every other byte PAD; the buffer is exactly n x stride bytes"""
    rows = np.full(g.n * stride, PAD, np.uint8)
    for i, k in enumerate(g.keys):
        k = k[:stride]
        rows[i * stride:i * stride + len(k)] = np.frombuffer(k, np.uint8)
    return rows, np.array([len(k) for k in g.keys], np.uint32)


def item_of(g, i):
    """request i of a generation as the fields of a RateLimitReq"""
    name, _, ukey = g.keys[i].partition(b"_")
    return dict(name=(name or b"k").decode(), unique_key=ukey.decode(), hits=int(g.hits[i]), limit=int(g.limit[i]), duration=int(g.duration[i]),
                algorithm=int(g.algorithm[i]), behavior=int(g.behavior[i]), burst=0 if g.burst is None else int(g.burst[i]),
                created_at=0 if g.created_at is None else int(g.created_at[i]))


def payloads_of(g, rng):
    """the generation as serialized GetRateLimitsReq payloads in arrival order: three random cut points and an RPC of one item"""
    import wire_replay
    n = g.n
    if n == 0:
        return []
    one = int(rng.integers(0, n))
    cut = sorted(set(rng.integers(0, n + 1, 3).tolist()) | {0, n, one, one + 1})
    flat = [item_of(g, i) for i in range(n)]
    rpcs = [flat[a:b] for a, b in zip(cut, cut[1:])]
    assert sum(len(r) for r in rpcs) == n and any(len(r) == 1 for r in rpcs)
    return [wire_replay.pb_request(r) for r in rpcs]


class RowsWorld(mc.World):
    """mesh_cases.World with engines of max_key_bytes = max_key, a device wire decoder per rank, and call() in the world's form"""

    def __init__(self, ga, support, W, n_engines, max_n, new_engines, upload, download, hash_kind="fnv1", front_max_n=None, with_global=False,
                 max_key=mc.MAX_KEY, form="rows", forms=None, dec_items=None):
        from gubernator_amd.mesh import Mesh
        from gubernator_amd import wire as gw
        self.ga, self.W, self.max_n, self.upload, self.download = ga, W, max_n, upload, download
        self.max_key, self.form = max_key, form
        self.forms = forms or (lambda call: [stride_of(max_key)] * W)
        self.ring = ga.Ring([f"gpu{r}" for r in range(W)], 512, hash_kind)
        self.engs, self.places, self.fronts, self.oracles, self.decs = [], [], [], [], []
        self.global_engine = n_engines if with_global else -1
        for r in range(W):
            flags = [0] * n_engines + ([ga.FLAG_GLOBAL] if with_global else [])
            engs = new_engines(r, flags, dict(cache_size=1 << 14, max_batch=4096, max_key_bytes=max_key))
            place = ga.Placement(n_engines) if (n_engines > 1 or with_global) else None
            self.engs.append(engs); self.places.append(place)
            self.fronts.append(ga.Front(engs, place, max_n=front_max_n or max_n, depth=3, global_engine=self.global_engine))
            self.oracles.append(support.Oracle(cache_size=1 << 20, workers=n_engines))
            if form == "wire":
                self.decs.append(gw.DevWireDecoder(engs[0], max_items=dec_items or max_n, max_payload_bytes=1 << 20, max_rpcs=16))
        self.mesh = Mesh(self.fronts, self.ring, max_n)
        scratch = new_engines(0, [0], dict(cache_size=64, max_batch=256, max_key_bytes=max_key))[0]
        self.errors = {}
        for kind, key in (("empty", b""), ("too_long", b"\x21" * (max_key + 1))):
            self.errors[kind] = scratch.eval(HostBatch([key], 1, 10, LONG_MS, NOW0, algorithm=0, behavior=0)).rows()[0]
        scratch.close()
        assert self.errors["empty"][4] == 4 and self.errors["too_long"][4] == 7, self.errors
        self.pairs = np.zeros((W, W), np.int64)
        self.seen = [dict() for _ in range(W)]
        self.calls = 0
        self.cut_rng = np.random.default_rng(977)

    def route(self, g):
        if g.n == 0:
            return np.zeros(0, np.uint32), np.zeros(0, bool), np.zeros(0, np.uint8)
        owner = self.ring.route(g.packed())
        lens = np.array([len(k) for k in g.keys])
        kind = np.where(lens == 0, 1, np.where(lens > self.max_key, 2, 0)).astype(np.uint8)
        return owner, ((g.behavior & mc.BEHAVIOR_GLOBAL) != 0) | (kind != 0), kind

    def _dev(self, gens, now, label):
        """packed or in rows: the columns uploaded as mesh_cases.World.call uploads them -> the answers per rank (sentinels checked)"""
        from gubernator_amd.mesh import MeshRows
        W = self.W
        forms = [0] * W if self.form == "packed" else self.forms(self.calls)
        B, R, RW, keep = (GuberBatch * W)(), (GuberResult * W)(), (MeshRows * W)(), []
        for r, g in enumerate(gens):
            rh = {k: self.upload(v) for k, v in result_arrays(g.n).items()}
            p = dict(key_bytes=None, key_off=None, key_len=None, hits=None, limit=None, duration=None, burst=None, created_at=None, algorithm=None, behavior=None)
            h = {}
            if g.n:
                src = dict(hits=g.hits, limit=g.limit, duration=g.duration, burst=g.burst, created_at=g.created_at, algorithm=g.algorithm,
                           behavior=g.behavior.view(np.int32))
                if forms[r]:
                    rows, klen = rows_of(g, forms[r])
                    assert rows.nbytes == g.n * forms[r]
                    src.update(key_bytes=rows, key_len=klen.view(np.int32))
                else:
                    kb, off = g.packed()
                    src.update(key_bytes=kb, key_off=off.view(np.int32))
                h = {k: self.upload(np.ascontiguousarray(v)) for k, v in src.items() if v is not None}
                p.update({k: v[1] for k, v in h.items()})
            B[r] = GuberBatch(g.n, 0, p["key_bytes"], p["key_off"], p["hits"], p["limit"], p["duration"], p["burst"], p["created_at"], p["algorithm"],
                              p["behavior"], None, None, None, now)
            RW[r] = MeshRows(forms[r] if g.n else 0, p["key_len"])
            R[r] = GuberResult(rh["status"][1], rh["limit"][1], rh["remaining"][1], rh["reset_time"][1], rh["err"][1], 0, 0, 0, 0, 0)
            keep.append((h, rh))
        if self.form == "packed":
            self.mesh.eval_dev(B, R)
        else:
            self.mesh.eval_rows_dev(B, RW, R)
        self.mesh.synchronize()
        out = []
        for r, g in enumerate(gens):
            arrays = {k: self.download(v[0]) for k, v in keep[r][1].items()}
            for name, a in arrays.items():
                s = SENTINEL_U8 if a.dtype == np.uint8 else SENTINEL_I64
                assert len(a) == g.n + TAIL and (a[g.n:] == s).all(), f"{label}: rank {r}: {name} was written behind its {g.n} answers"
            out.append({k: a[:g.n] for k, a in arrays.items()})
        return out

    def _wire(self, gens, absent, now, label):
        """through the decoders: -> the answers per rank"""
        from gubernator_amd import wire as gw
        decs = []
        for r, g in enumerate(gens):
            if absent[r] and self.calls % 2:
                decs.append(None)                                   # (nothing arrived: no decoder; in the other calls a decoder that decoded nothing)
                continue
            d = self.decs[r]
            status, first, count, n = d.decode(payloads_of(g, self.cut_rng), now, max_per_rpc=4096)
            assert n == g.n and (status == 0).all() and int(count.sum()) == g.n, (label, r, n, g.n, status)
            decs.append(d)
        res = gw.eval_mesh(decs, self.mesh)
        return [{k: getattr(res[r], k)[:g.n] for k in NAMES} for r, g in enumerate(gens)]

    def call(self, gens, label):
        """one call over gens[r] (None: nothing arrived at rank r) in the world's form; checks answers and the mesh's counts; -> answers per rank"""
        now = next(g.now for g in gens if g is not None)
        absent = [g is None for g in gens]
        gens = [g if g is not None else Gen([], now) for g in gens]
        assert all(g.now == now for g in gens)
        before = self.mesh.stats()
        arrays = self._wire(gens, absent, now, label) if self.form == "wire" else self._dev(gens, now, label)
        after = self.mesh.stats()
        want, forwarded = self.expected(gens)
        got_all = []
        for r, g in enumerate(gens):
            got, exp = HostResult(g.n), HostResult(g.n)
            for name in NAMES:
                getattr(got, name)[:g.n] = arrays[r][name]
                getattr(exp, name)[:g.n] = want[r][name]
            assert_results_equal(got, exp, f"{label}: rank {r} (n={g.n}, {self.form})")
            got_all.append(got)
        assert after["calls"] - before["calls"] == 1 and after["requests"] - before["requests"] == sum(g.n for g in gens), (label, before, after)
        assert after["forwarded"] - before["forwarded"] == forwarded, (label, after["forwarded"] - before["forwarded"], forwarded)
        self.calls += 1
        return got_all

    def spread(self, width, per_owner=150):
        """distinct keys "k_<digits>" of exactly `width` bytes of which every rank owns up to per_owner, owner by owner in turn (fnv1 moves
        keys that differ in their last digits only a few ring points: consecutive numbers belong to a handful of owners — these are picked
        from numbers 37 apart; width 3 has ten keys, they are what they are)"""
        top = 10 ** min(width - 2, 7)
        cand = [b"k_%0*d" % (width - 2, i) for i in range(0, top, 37 if top > 4000 else 1)][:6000]
        owner = self.ring.route(Gen(cand, NOW0).packed())
        mine = [np.nonzero(owner == o)[0][:per_owner] for o in range(self.W)]
        return [cand[mine[o][j]] for j in range(per_owner) for o in range(self.W) if j < len(mine[o])]

    def held(self):
        """the keys every engine of every rank holds"""
        return [[sorted(it["key"] for it in e.each()) for e in engs] for engs in self.engs]

    def sizes(self):
        return [[e.size() for e in engs] for engs in self.engs]

    def close(self):
        for d in self.decs:
            d.close()
        super().close()


def error_item(g, i, key):
    """request i becomes the request of World.errors with `key` (empty, or longer than max_key_bytes)"""
    g.keys[i] = key
    g.hits[i], g.limit[i], g.duration[i], g.algorithm[i], g.behavior[i] = 1, 10, LONG_MS, 0, 0
    if g.burst is not None:
        g.burst[i] = 0
    if g.created_at is not None:
        g.created_at[i] = g.now


# ---- through the wire ----------------------------------------------------------------------------------------------------------------
def wire(make_world, **fixed):
    return lambda **kw: make_world(form="wire", **fixed, **kw)


def case_a(make_world):
    """a: W = 3, two engines per rank, mesh_cases.SIZES_A (0, 1, 63, 64, 65, 1 023, 1 024, 1 025, 2 049 items mixed across the ranks of a
    call, a rank without a decoder, all ranks but one empty), a dozen calls over one population; answers, forwarded counts, every pair of
    ranks, residency"""
    assert mc.scenario_a(wire(make_world)) == len(SIZES_A)


def case_b(make_world):
    """b: HashKey widths 3, 8, 15, 16 at stride 24 (max_key_bytes 16: no speculative read) and 3, 8, 24, 31, 32, 33, 64 at stride 72; per
    stride a run of one width whose last key is a byte longer and a call of mixed widths; an item with an empty unique_key in every
    generation: error 4, in its place, not forwarded (World.call compares the forwarded count)"""
    for max_key, widths, ragged in ((16, (3, 8, 15, 16), 15), (64, (3, 8, 24, 31, 32, 33, 64), 31)):
        w = make_world(form="wire", W=3, n_engines=2, max_n=1025, max_key=max_key)
        assert stride_of(max_key) == (24 if max_key == 16 else 72)
        rng = np.random.default_rng(320 + max_key)
        runs = [(x, False) for x in widths] + [(ragged, True), (None, False)]
        for c, (width, odd) in enumerate(runs):
            now = NOW0 + c * STEP_MS
            pop = w.spread(width) if width else sum((w.spread(x, 14) for x in widths), [])
            gens = []
            for r in range(3):
                n = (300, 1025, 257)[(r + c) % 3]
                g = by_ids(pop, draw(rng, n, len(pop)), now, c)
                if odd:
                    g.keys[-1] = g.keys[-1] + b"x"
                error_item(g, int(rng.integers(0, n - 1)), b"")      # ("k" + "_" + an empty unique_key: pre-rejected, an empty key row)
                gens.append(g)
            got = w.call(gens, f"b stride {stride_of(max_key)} width {width or 'mixed'}{' ragged' if odd else ''}")
            assert all((x.err[:x.n] == 4).sum() == 1 for x in got)
        w.assert_every_pair_used(f"b {max_key}")
        w.check_residency(f"b {max_key}")
        w.close()


def case_c(make_world):
    """c: one hot token key in a payload at every rank in one call turns OVER_LIMIT exactly where source 0, 1, 2 in turn exhaust it"""
    mc.scenario_c(wire(make_world))


def case_d(make_world):
    """d: W = 2 with a GLOBAL engine per rank, half of the items Behavior_GLOBAL: none is forwarded, they are resident in the arrival
    rank's GLOBAL engine with is_owner from the ring"""
    mc.scenario_f(wire(make_world))


def case_e(make_world):
    """e: W = 4, every rank's payloads hold 2 049 items rank 2 owns; the front's max_n is 2 049"""
    mc.scenario_e(wire(make_world))


def case_r(make_world):
    """refusals of guber_wire_dev_eval_mesh, each before anything is enqueued: the engines' sizes and the mesh's counts stay"""
    import wire_replay
    from gubernator_amd import wire as gw
    w = make_world(form="wire", W=2, n_engines=2, max_n=64, dec_items=256)
    ga_err, E_ARG, E_LARGE = w.ga.GuberError, w.ga.E_INVALID_ARG, w.ga.E_BATCH_TOO_LARGE
    pop = mc.population(500)
    rng = np.random.default_rng(39)
    w.call([by_ids(pop, rng.integers(0, 300, 64), NOW0, 0) for _ in range(2)], "r a call that is taken")
    sizes, stats = w.sizes(), w.mesh.stats()
    assert sum(map(sum, sizes)) > 0

    def fresh(k, n=8):
        return [item_of(by_ids(pop, np.arange(300 + k * 20, 300 + k * 20 + n), NOW0 + STEP_MS, 1), i) for i in range(n)]

    def refused(decs, code, label):
        try:
            gw.eval_mesh(decs, w.mesh)
        except ga_err as e:
            assert e.code == code, (label, e)
        else:
            raise AssertionError(f"{label}: not refused")
        assert w.sizes() == sizes and w.mesh.stats()["calls"] == stats["calls"] and w.mesh.stats()["requests"] == stats["requests"], label

    d0, d1 = w.decs
    now = NOW0 + STEP_MS
    # a peer RPC among the payloads of a decode
    st, _, _, n = d0.decode([wire_replay.pb_request(fresh(0)), wire_replay.pb_request(fresh(1), peer=True)], now, is_owner=[gw.RPC_OWNER, gw.RPC_OWNER | gw.RPC_PEER])
    assert n == 16 and (st == 0).all()
    d1.decode([wire_replay.pb_request(fresh(2))], now)
    refused([d0, d1], E_ARG, "a GUBER_WIRE_RPC_PEER payload")
    # two decodes at different instants
    d0.decode([wire_replay.pb_request(fresh(0))], now)
    d1.decode([wire_replay.pb_request(fresh(2))], now + 1)
    refused([d0, d1], E_ARG, "two now_ms")
    # one decoder at two ranks
    refused([d0, d0], E_ARG, "a decoder twice")
    # more items than the mesh's generations hold
    st, _, _, n = d0.decode([wire_replay.pb_request(fresh(3, 65))], now)
    assert n == 65 and (st == 0).all()
    d1.decode([wire_replay.pb_request(fresh(2))], now)
    refused([d0, d1], E_LARGE, "n_items above the mesh's max_n")
    # ... and the same decoders are taken once nothing is wrong
    d0.decode([wire_replay.pb_request(fresh(0))], now)
    res = gw.eval_mesh([d0, d1], w.mesh)
    assert (res[0].err[:8] == 0).all() and (res[1].err[:8] == 0).all() and w.mesh.stats()["calls"] == stats["calls"] + 1
    assert sum(map(sum, w.sizes())) == sum(map(sum, sizes)) + 16
    w.close()


# ---- rows without the wire -----------------------------------------------------------------------------------------------------------
def case_f(make_world):
    """f: two identical worlds and the same generations — sizes of SIZES_A, one width per call of 3, 8, 31, 32, 33, 40, a key of
    max_key_bytes + 1 and an empty key in every generation of 64 requests or more — one called packed, the other in rows of stride 48
    with 0xA5 behind every key and the last row ending at its allocation's end: answers, forwarded counts and residency are equal"""
    wp = make_world(form="packed", W=3, n_engines=2, max_n=2049)
    wr = make_world(form="rows", W=3, n_engines=2, max_n=2049)
    assert stride_of(wr.max_key) == 48
    widths = (3, 8, 31, 32, 33, 40)
    for c, sizes in enumerate(SIZES_A):
        now, rng = NOW0 + c * STEP_MS, np.random.default_rng(600 + c)
        pop = wr.spread(widths[c % 6])
        gens = []
        for r, n in enumerate(sizes):
            if not n:
                gens.append(None)
                continue
            g = by_ids(pop, draw(rng, n, len(pop)), now, c, full=(c + r) % 4 == 1, rng=rng)
            if n >= 64:
                a, b = rng.choice(n, 2, replace=False)
                error_item(g, int(a), b"")
                error_item(g, int(b), b"\x21" * (mc.MAX_KEY + 1))
            gens.append(g)
        gp, gr = wp.call(gens, f"f packed call {c}"), wr.call(gens, f"f rows call {c}")
        for r, (x, y) in enumerate(zip(gp, gr)):
            for name in NAMES:
                assert np.array_equal(getattr(x, name)[:x.n], getattr(y, name)[:y.n]), (c, r, name)
            if sizes[r] >= 64:
                assert (y.err[:y.n] == 4).sum() == 1 and (y.err[:y.n] == 7).sum() == 1, (c, r)
        assert wp.mesh.stats()["forwarded"] == wr.mesh.stats()["forwarded"]
    assert wp.held() == wr.held() and wp.sizes() == wr.sizes()
    for w in (wp, wr):
        w.assert_every_pair_used("f")
        w.check_residency("f")
        w.close()


def case_g(make_world):
    """g: the forms mixed in one call over engines of max_key_bytes 16 — packed, rows of stride 48, rows of stride 24 (no speculative
    read) — moving one rank on from call to call; key widths 3, 8, 15, 16, a key of 17 bytes and an empty key in every generation"""
    base = (0, 48, 24)
    w = make_world(form="rows", W=3, n_engines=2, max_n=2049, max_key=16, forms=lambda call: [base[(r + call) % 3] for r in range(3)])
    one = [w.spread(x, 100) for x in (3, 8, 15, 16)]
    rng = np.random.default_rng(41)
    for c in range(6):
        now = NOW0 + c * STEP_MS
        pop = one[c] if c < 4 else sum((p[:80] for p in one), [])
        gens = []
        for r in range(3):
            n = (1025, 300, 2049)[(r + c) % 3]
            g = by_ids(pop, draw(rng, n, len(pop)), now, c, full=c == 5, rng=rng)
            a, b = rng.choice(n, 2, replace=False)
            error_item(g, int(a), b"")
            error_item(g, int(b), b"\x21" * 17)
            gens.append(g)
        got = w.call(gens, f"g call {c} forms {w.forms(c)}")
        assert all((x.err[:x.n] == 4).sum() == 1 and (x.err[:x.n] == 7).sum() == 1 for x in got)
    w.assert_every_pair_used("g")
    w.check_residency("g")
    w.close()


def case_h(make_world, plain_front, wire_front):
    """h: W = 1 does no exchange.  In rows it equals a plain front over a second set of engines fed the same generations (mesh_cases'
    scenario h: guber_front_eval_dev takes them packed — a front's rows arrive through a decoder), and through the wire it equals
    guber_wire_dev_eval_front over a second set of engines fed the same payloads, i.e. the same rows.
    wire_front(n_engines, max_n) -> (eval(payloads, now) -> HostResult, close)"""
    mc.scenario_h(lambda **kw: make_world(form="rows", **kw), plain_front)
    from gubernator_amd import wire as gw
    w = make_world(form="wire", W=1, n_engines=2, max_n=2049, front_max_n=1024)
    ref_eval, ref_close = wire_front(2, 2049)
    pop, rng = mc.population(), np.random.default_rng(42)
    for c, n in enumerate((1025, 2049, 1)):
        now = NOW0 + c * STEP_MS
        g = by_ids(pop, draw(rng, n, mc.POP), now, c)
        payloads = payloads_of(g, rng)
        _, _, _, got_n = w.decs[0].decode(payloads, now, max_per_rpc=4096)
        assert got_n == n
        got, ref = gw.eval_mesh([w.decs[0]], w.mesh)[0], ref_eval(payloads, now)
        for name in NAMES:
            assert np.array_equal(getattr(got, name)[:n], getattr(ref, name)[:n]), (c, name)
    assert w.mesh.stats()["forwarded"] == 0 and w.mesh.stats()["bytes_moved"] == 0 and w.mesh.stats()["inflow_pieces"] == 2 + 3 + 1
    ref_close()
    w.close()


def case_h16(make_world):
    """sixteen ranks of one engine, 1 025 rows per rank, the ring (64 KB) searched in global memory"""
    mc.scenario_g(lambda **kw: make_world(form="rows", **kw))


def wire_front_of(ga, new_engines):
    """-> wire_front(n_engines, max_n) for case_h"""
    from gubernator_amd import wire as gw

    def wire_front(n_engines, max_n):
        engs = new_engines(0, [0] * n_engines, dict(cache_size=1 << 14, max_batch=4096, max_key_bytes=mc.MAX_KEY))
        place = ga.Placement(n_engines)
        fr = ga.Front(engs, place, max_n=max_n, depth=3)
        dec = gw.DevWireDecoder(engs[0], max_items=max_n, max_payload_bytes=1 << 20, max_rpcs=16)

        def run(payloads, now):
            dec.decode(payloads, now, max_per_rpc=4096)
            return dec.eval_front(fr)

        def close():
            dec.close(); fr.close()
            for e in engs:
                e.close()
            place.close()
        return run, close
    return wire_front


# ---- the cases on the CPU build of the engine (tests/test_mesh_rows_cpu.py): GUBER_HIP_LIB=tests/hostsim/libenginesim.so python tests/mesh_rows_cases.py <letter>
def _cpu_main(letter):
    import gubernator_amd as ga
    import support
    assert "enginesim" in ga.LIB_PATH, "this entry is for the CPU build of the engine (GUBER_HIP_LIB)"

    def new_engines(rank, flags, kw):
        e0 = ga.Engine(flags=flags[0], **kw)
        return [e0] + [ga.Engine(flags=f, stream=e0.stream_handle(), **kw) for f in flags[1:]]

    def make_world(**kw):
        return RowsWorld(ga, support, new_engines=new_engines, upload=lambda a: (a, a.ctypes.data), download=lambda a: a, **kw)

    def plain_front(n_engines, max_n):
        engs = new_engines(0, [0] * n_engines, dict(cache_size=1 << 14, max_batch=4096, max_key_bytes=mc.MAX_KEY))
        place = ga.Placement(n_engines)
        fr = ga.Front(engs, place, max_n=max_n, depth=3)

        def run(g):
            kb, off = g.packed()
            hb = HostBatch((kb, off), g.hits, g.limit, g.duration, g.now, burst=g.burst, created_at=g.created_at, algorithm=g.algorithm, behavior=g.behavior)
            r = result_arrays(g.n)
            res = GuberResult(r["status"].ctypes.data, r["limit"].ctypes.data, r["remaining"].ctypes.data, r["reset_time"].ctypes.data, r["err"].ctypes.data, 0, 0, 0, 0, 0)
            assert fr.eval_dev((GuberBatch * 1)(hb.c), (GuberResult * 1)(res), 1) == 1
            fr.synchronize()
            return r

        def close():
            fr.close()
            for e in engs:
                e.close()
            place.close()
        return run, close

    cases = dict(a=case_a, b=case_b, c=case_c, d=case_d, e=case_e, r=case_r, f=case_f, g=case_g)
    if letter == "h":
        case_h(make_world, plain_front, wire_front_of(ga, new_engines))
    else:
        cases[letter](make_world)
    print("MESH ROWS CASE OK", letter)


if __name__ == "__main__":
    _cpu_main(sys.argv[1])
