"""Store generations for the device front (guber_front_probe_missing_dev / guber_front_eval_store_dev, include/guber_gpu.h "Config.Store for
a front"; gubernator_amd/csrc/guber_kernels_front_store.h) and the checks that go with them; shared by tests/test_gpu_front_store.py (the
product library on a GPU) and tests/test_front_store_cpu.py (the same kernels and host code compiled for the CPU).  numpy only, like
tests/front_edges.py: the front, the engines, the oracle and the device's side of a generation are handed in by the caller.

  model()          the two rules of the probe in ten lines: where a generation is cut, and which requests Store.Get is due for
  eval_store()     one generation the way a host with Config.Store drives a front: probe -> (a cut: the prefix, then the rest) ->
                   Store.Get per asked request -> add_items per engine -> eval_store_dev -> Remove, then OnChange, in arrival order
  parity()         random generations (the generator of test_gpu_parity.test_store_events_match_the_oracle_on_random_batches) through
                   eval_store() against ONE oracle with the same mock store
  probe_cases()    the probe alone at its edges, against model()"""
import ctypes as C

import numpy as np

from gubernator_amd.abi import GuberBatch, GuberResult, HostBatch, HostResult, assert_results_equal, item_dict, make_item

NOW0 = 1_700_000_000_000
RESET_REMAINING = 8
E_INVALID_ARG, E_NOMEM = -1, -6
PROBE_SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)
NEW_KERNELS = ("k_fr_elect", "k_fr_missing", "k_fr_ask", "k_fr_out_store")


def keys_of(hb):
    kb, off = hb.key_bytes.tobytes(), hb.key_off.tolist()
    return [kb[off[i]:off[i + 1]] for i in range(hb.n)]


def model(keys, behavior, resident):
    """(index, cut_at): cut_at = the smallest i with an earlier request of the same key that carries RESET_REMAINING; index = the first
    request of every non-empty key among [0, cut_at) that is not resident (resident: key -> bool)"""
    reset, cut = set(), len(keys)
    for i, k in enumerate(keys):
        if k in reset:
            cut = i
            break
        if int(behavior[i]) & RESET_REMAINING:
            reset.add(k)
    seen, index = set(), []
    for i, k in enumerate(keys[:cut]):
        if k not in seen and k and not resident(k):
            index.append(i)
        seen.add(k)
    return index, cut


_COLS = (("key_off", 4), ("hits", 8), ("limit", 8), ("duration", 8), ("burst", 8), ("created_at", 8), ("algorithm", 1), ("behavior", 4), ("is_owner", 1))
_RES = (("status", 1), ("limit", 8), ("remaining", 8), ("reset_time", 8), ("err", 1))


def piece(b, r, lo, hi):
    """requests [lo, hi) of a generation as a generation of their own, by pointer arithmetic on its columns (key_bytes stays: the offsets
    are absolute)"""
    sb, sr = GuberBatch(), GuberResult()
    C.memmove(C.byref(sb), C.byref(b), C.sizeof(GuberBatch))
    C.memmove(C.byref(sr), C.byref(r), C.sizeof(GuberResult))
    sb.n = hi - lo
    for name, w in _COLS:
        if getattr(b, name):
            setattr(sb, name, getattr(b, name) + lo * w)
    for name, w in _RES:
        setattr(sr, name, getattr(r, name) + lo * w)
    return sb, sr


def item_of(key, d):
    return make_item(key, d["algorithm"], limit=d.get("limit", 0), duration=d.get("duration", 0), remaining=d.get("remaining", 0),
                     remaining_f=d.get("remaining_f", 0.0), stamp=d.get("stamp", 0), burst=d.get("burst", 0), expire_at=d.get("expire_at", 0),
                     invalid_at=d.get("invalid_at", 0), status=d.get("status", 0))


def eval_store(front, engines, make_dev_gen, hb, store):
    """hb through the front with `store` (support.MockStore) -> HostResult.  make_dev_gen(hb) -> (GuberBatch, GuberResult, fetch): the
    generation's columns and result arrays on the device, fetch() -> {name: numpy} of the result arrays"""
    b, r, fetch = make_dev_gen(hb)
    keys = [k.decode() for k in keys_of(hb)]

    def run(lo, hi):
        sb, sr = piece(b, r, lo, hi)
        index, engine, cut = front.probe_missing_dev(sb)
        if cut < hi - lo:
            assert 0 < cut, (lo, hi, cut)
            run(lo, lo + cut)
            run(lo + cut, hi)
            return
        assert (np.diff(index.astype(np.int64)) > 0).all() and (len(index) == 0 or index[-1] < hi - lo), index
        per_engine = {}
        for i, e in zip(index.tolist(), engine.tolist()):
            d = store.get(lo + i, keys[lo + i])
            if d is not None:
                per_engine.setdefault(e, []).append(item_of(keys[lo + i], d))
        for e, items in per_engine.items():
            engines[e].set_clock(hb.now_ms)
            engines[e].add_items(items)
        flags, items = front.eval_store_dev(sb, sr)
        for i in range(hi - lo):
            if flags[i] & 2:
                store.remove(lo + i, keys[lo + i])
            if flags[i] & 1:
                assert not items[i].key and items[i].key_len == len(keys[lo + i].encode()), (i, items[i].key_len)
                store.on_change(lo + i, keys[lo + i], item_dict(items[i], key=keys[lo + i]))

    run(0, hb.n)
    got = HostResult(hb.n)
    out = fetch()
    for name in ("status", "limit", "remaining", "reset_time", "err"):
        getattr(got, name)[:hb.n] = out[name][:hb.n]
    return got


def random_generations(seed, steps=12, max_n=3000, resets=True):
    """the generator of tests/test_gpu_parity.py test_store_events_match_the_oracle_on_random_batches: valid algorithms, non-empty keys,
    400 keys, Zipf 1.3, mixed RESET_REMAINING / DRAIN_OVER_LIMIT, is_owner = 0 in every third step.  resets=False: the same without
    RESET_REMAINING, so that no generation is cut and the engines' shares are as large as the generation makes them"""
    rng = np.random.default_rng(seed)
    now = NOW0
    for step in range(steps):
        n = int(rng.integers(1, max_n))
        kid = rng.zipf(1.3, n) % 400
        shape = rng.integers(0, 6, 400)
        mixed = rng.random(n) < 0.15
        algo = np.where(mixed, rng.integers(0, 2, n), shape[kid] & 1).astype(np.uint8)
        beh = np.where(mixed, rng.choice([0, 8 if resets else 0, 32, 0, 0], n), np.where(shape[kid] == 5, 32, 0)).astype(np.uint32)
        hits = np.where(mixed, rng.integers(0, 4, n), 1).astype(np.int64)
        owner = np.where(rng.random(n) < 0.1, 0, 1).astype(np.uint8) if step % 3 == 2 else np.ones(n, np.uint8)
        keys = [b"st_k%d" % k for k in kid]
        yield step, HostBatch(keys, hits, 20 + (kid % 7), np.where(kid % 11 == 0, 3, 60_000), now, algorithm=algo, behavior=beh, is_owner=owner,
                              burst=np.zeros(n, np.int64), created_at=np.full(n, now))
        now += int(rng.choice([1, 2, 5, 4000]))


def parity(front, engines, orc, make_dev_gen, store_cls, seed, steps=12, max_n=3000, resets=True):
    """-> (generations, cuts seen).  Answers equal ONE oracle; the on_change / remove call list, items included, equals the oracle's in
    arrival order; per key the whole call sequence, get included, equals the oracle's; the engines hold as many items as the oracle"""
    so, se = store_cls(write_through=True), store_cls(write_through=True)
    count = 0
    for step, hb in random_generations(seed, steps, max_n, resets):
        for st in (so, se):
            st.calls.clear()
            st.now = hb.now_ms
        want = orc.eval_store(hb, so)
        got = eval_store(front, engines, make_dev_gen, hb, se)
        assert_results_equal(got, want, f"store generation {step} (n={hb.n})")
        pick = lambda st, kinds: [c for c in st.calls if c[0] in kinds]
        assert pick(se, ("on_change", "remove")) == pick(so, ("on_change", "remove")), f"generation {step}: the events differ"
        by_key = lambda st: {k: [c for c in st.calls if c[2] == k] for k in {c[2] for c in st.calls}}
        assert by_key(se) == by_key(so), f"generation {step}: a key's call sequence differs"
        count += 1
    sizes = [e.size() for e in engines]
    assert sum(sizes) == orc.size(), (sizes, orc.size())
    return count, front.store_stats()["cuts"]


# ---- the probe alone ------------------------------------------------------------------------------------------------------------
class Keys:
    """fresh keys — no key is handed out twice in a process — packed (every key 16 bytes) or ragged (2 bytes and more)"""
    next = 0

    def __init__(self, packed):
        self.packed = packed

    def take(self, count):
        ids = range(Keys.next, Keys.next + count)
        Keys.next += count
        return [(b"%016d" % i) if self.packed else (b"r%d" % i) for i in ids]


class Probe:
    """one front and what is resident behind it; route(keys) -> the engine of every key (None: one engine)"""

    def __init__(self, front, engines, make_dev_gen, route, now=NOW0):
        self.front, self.engines, self.make_dev_gen, self.route, self.now = front, engines, make_dev_gen, route, now
        self.resident = set()

    def engines_of(self, keys):
        if self.route is None or not keys:
            return [0] * len(keys)
        return [int(e) for e in self.route(keys)]

    def make_resident(self, keys):
        keys = [k for k in dict.fromkeys(keys) if k not in self.resident]
        per = {}
        for k, e in zip(keys, self.engines_of(keys)):
            per.setdefault(e, []).append(make_item(k, 0, limit=100, duration=600_000, remaining=50, expire_at=self.now + 600_000))
        for e, items in per.items():
            self.engines[e].set_clock(self.now)
            self.engines[e].add_items(items)
        self.resident.update(keys)

    def gen(self, keys, behavior=None):
        n = len(keys)
        hb = HostBatch(keys, 1, 100, 600_000, self.now, algorithm=0, behavior=np.zeros(n, np.uint32) if behavior is None else np.asarray(behavior, np.uint32))
        return hb, self.make_dev_gen(hb)

    def check(self, label, keys, behavior=None, cap=None):
        """probe the generation and compare with the model -> (index, cut_at, device side)"""
        n = len(keys)
        beh = np.zeros(n, np.uint32) if behavior is None else np.asarray(behavior, np.uint32)
        hb, side = self.gen(keys, beh)
        want_index, want_cut = model(keys, beh, lambda k: k in self.resident)
        index, engine, cut = self.front.probe_missing_dev(side[0], cap=cap)
        assert cut == want_cut, f"{label}: cut_at {cut}, the model's {want_cut}"
        assert index.tolist() == want_index, f"{label}: {len(index)} asked, the model {len(want_index)}; first difference at " \
            f"{next((q for q, (a, w) in enumerate(zip(index.tolist(), want_index)) if a != w), min(len(index), len(want_index)))}"
        assert engine.tolist() == self.engines_of([keys[i] for i in want_index]), f"{label}: the engines of the asked requests"
        return index, cut, (hb, side)


def probe_sizes_and_residency(p, packed, sizes=PROBE_SIZES):
    """every size x (every key resident; every key missing and distinct, then with one entry too few; half resident with repeats)"""
    K = Keys(packed)
    what = "packed" if packed else "ragged"
    rng = np.random.default_rng(5 + packed)
    for n in sizes:
        pool = K.take(max(1, n // 3))
        p.make_resident(pool)
        index, cut, _ = p.check(f"{what} n={n} every key resident", [pool[i] for i in rng.integers(0, len(pool), n)])
        assert len(index) == 0 and cut == n
        fresh = K.take(n)
        index, cut, (hb, side) = p.check(f"{what} n={n} every key missing and distinct", fresh)
        assert index.tolist() == list(range(n)) and cut == n
        if n:
            try:
                p.front.probe_missing_dev(side[0], cap=n - 1)
                raise AssertionError(f"{what} n={n}: cap = n - 1 was accepted")
            except RuntimeError as err:
                assert getattr(err, "code", None) == E_NOMEM and getattr(err, "needed", None) == n, (err, getattr(err, "needed", None))
        mix = pool + K.take(max(1, n // 3))
        p.check(f"{what} n={n} half resident, repeats", [mix[i] for i in rng.integers(0, len(mix), n)])


def probe_skew_and_cuts(p, packed, n=2049, n_engines=1):
    K = Keys(packed)
    what = "packed" if packed else "ragged"
    rng = np.random.default_rng(15 + packed)
    one = K.take(1)
    index, cut, _ = p.check(f"{what} one key {n} times", one * n)
    assert index.tolist() == [0] and cut == n
    if n_engines > 1:                                               # everything to the last engine
        cand = K.take(40 * n_engines)
        last = [k for k, e in zip(cand, p.engines_of(cand)) if e == n_engines - 1]
        assert len(last) >= 4, len(last)
        p.make_resident(last[:len(last) // 2])
        p.check(f"{what} everything to the last engine", [last[i] for i in rng.integers(0, len(last), n)])
    pool = K.take(300)
    p.make_resident(pool[:150])

    def draw(avoid):
        """n requests over the pool, none of the keys in `avoid`"""
        rest = [k for k in pool if k not in avoid]
        return [rest[i] for i in rng.integers(0, len(rest), n)]

    a, b = pool[200], pool[10]                                      # a missing, b resident
    for at in (1, 1024, n - 1):                                     # a cut at 1, at a tile's edge and at the last request
        keys, beh = draw({a, b}), np.zeros(n, np.uint32)
        keys[0], keys[at] = a, a
        beh[0] = RESET_REMAINING
        index, cut, _ = p.check(f"{what} a cut at {at}", keys, beh)
        assert cut == at
    keys, beh = draw({a, b}), np.zeros(n, np.uint32)                # a reset as the LAST request of its key: no cut
    keys[3], keys[700] = b, b
    beh[700] = RESET_REMAINING
    index, cut, _ = p.check(f"{what} a reset as the last request of its key", keys, beh)
    assert cut == n
    keys, beh = draw({a, b}), np.zeros(n, np.uint32)                # resets on two keys: the smaller cut wins
    keys[5], keys[1500] = a, a
    keys[6], keys[1100] = b, b
    beh[5] = beh[6] = RESET_REMAINING
    index, cut, _ = p.check(f"{what} resets on two keys", keys, beh)
    assert cut == 1100
    c = K.take(1)[0]                                                # an ask candidate behind cut_at is not reported
    keys, beh = draw({a, b}), np.zeros(n, np.uint32)
    keys[2], keys[40], keys[41] = b, b, c
    beh[2] = RESET_REMAINING
    index, cut, _ = p.check(f"{what} an ask candidate behind the cut", keys, beh)
    assert cut == 40 and 41 not in index.tolist()
    keys, beh = draw({a, b}), np.zeros(n, np.uint32)                # an empty key twice, the first with the bit: a cut like any other, never asked for
    keys[7], keys[900] = b"", b""
    beh[7] = RESET_REMAINING
    index, cut, _ = p.check(f"{what} an empty key", keys, beh)
    assert cut == 900 and 7 not in index.tolist()


def probe_contract(p, orc):
    """eval_store_dev after a cut report or with another generation is refused; a plain eval_dev afterwards still answers correctly"""
    K = Keys(True)
    keys = K.take(100)
    beh = np.zeros(100, np.uint32)
    keys[50] = keys[0]
    beh[0] = RESET_REMAINING
    _, cut, (hb, side) = p.check("contract: a cut", keys, beh)
    assert cut == 50

    def refused(b, r, why):
        try:
            p.front.eval_store_dev(b, r)
        except RuntimeError as err:
            assert getattr(err, "code", None) == E_INVALID_ARG, err
            return
        raise AssertionError(f"eval_store_dev {why} was accepted")
    refused(side[0], side[1], "after a cut report")
    keys2 = K.take(70)
    _, cut, (hb2, side2) = p.check("contract: no cut", keys2)
    assert cut == 70
    refused(side[0], side[1], "with another generation than the probed one")
    other = piece(side2[0], side2[1], 0, 69)
    refused(other[0], other[1], "with another n than the probed generation's")
    withb = piece(side2[0], side2[1], 0, 70)
    withb[0].burst = side2[0].hits
    refused(withb[0], withb[1], "with a burst column the probe did not route")
    # (the probed generation is still there: a plain call drops it and routes afresh)
    hb3 = HostBatch(K.take(300) + keys2, 1, 7, 60_000, p.now, algorithm=np.arange(370) % 2)
    b3, r3, fetch3 = p.make_dev_gen(hb3)
    assert p.front.eval_dev((GuberBatch * 1)(b3), (GuberResult * 1)(r3), 1) == 1
    p.front.synchronize()
    got = HostResult(hb3.n)
    out = fetch3()
    for name in ("status", "limit", "remaining", "reset_time", "err"):
        getattr(got, name)[:hb3.n] = out[name][:hb3.n]
    assert_results_equal(got, orc.eval(hb3), "a plain generation behind a probed one")
    refused(side2[0], side2[1], "after a plain call dropped the probed generation")
    st = p.front.store_stats()
    assert st["evaluations"] == 0 and st["cuts"] >= 1, st


def probe_global(p, global_engine, n=2049):
    """a front whose rule names a global_engine: a key's Behavior_GLOBAL requests are routed to that engine's table and are a key of their
    own there — asked for on their own, resident on their own, and neither cutting nor cut by the key's other requests (include/guber_gpu.h).
    The model is front_store.model() over (engine, key)"""
    GLOBAL = 2
    K = Keys(True)
    rng = np.random.default_rng(21)
    cand = K.take(400)
    pool = [k for k, e in zip(cand, p.engines_of(cand)) if e != global_engine][:120]      # keys whose own table is not the GLOBAL engine's
    home = dict(zip(pool, p.engines_of(pool)))
    a, b, c = pool[0], pool[1], pool[2]
    p.make_resident(pool[60:])                                      # resident in their own tables
    p.engines[global_engine].set_clock(p.now)                       # b and half of the pool: resident in the GLOBAL engine's table only / as well
    p.engines[global_engine].add_items([make_item(k, 0, limit=100, duration=600_000, remaining=50, expire_at=p.now + 600_000) for k in [b] + pool[30:90]])
    resident = {(home[k], k) for k in pool[60:]} | {(global_engine, k) for k in [b] + pool[30:90]}
    rest = pool[3:]
    keys = [rest[i] for i in rng.integers(0, len(rest), n)]
    beh = np.where(rng.random(n) < 0.5, GLOBAL, 0).astype(np.uint32)
    keys[0], beh[0] = a, RESET_REMAINING                            # a reset of a in its own table ...
    keys[10], beh[10] = a, GLOBAL                                   # ... does not cut a's GLOBAL request ...
    keys[11], beh[11] = b, GLOBAL                                   # (b is resident in the GLOBAL engine: not asked for ...
    keys[12], beh[12] = b, 0                                        #  ... but missing in its own table: asked for)
    keys[13], beh[13] = c, GLOBAL | RESET_REMAINING                 # a reset of c in the GLOBAL engine does not cut c's plain request ...
    keys[900], beh[900] = c, 0
    keys[1500], beh[1500] = c, GLOBAL                               # ... it cuts c's next GLOBAL request
    keys[1800], beh[1800] = a, 0                                    # (behind the cut)
    ids = [(global_engine if int(beh[i]) & GLOBAL else home[k], k) for i, k in enumerate(keys)]
    want_index, want_cut = model(ids, beh, lambda ident: ident in resident)
    assert want_cut == 1500 and {0, 10, 12, 13} <= set(want_index) and 11 not in want_index, (want_cut, want_index[:8])
    hb, side = p.gen(keys, beh)
    index, engine, cut = p.front.probe_missing_dev(side[0])
    assert cut == want_cut and index.tolist() == want_index, (cut, want_cut, len(index), len(want_index))
    assert engine.tolist() == [ids[i][0] for i in want_index]
    keys[1500], beh[1500] = a, 0                                    # a's plain request instead: cut by the reset at 0
    ids = [(global_engine if int(beh[i]) & GLOBAL else home[k], k) for i, k in enumerate(keys)]
    want_index, want_cut = model(ids, beh, lambda ident: ident in resident)
    assert want_cut == 1500
    hb, side = p.gen(keys, beh)
    index, engine, cut = p.front.probe_missing_dev(side[0])
    assert cut == want_cut and index.tolist() == want_index and engine.tolist() == [ids[i][0] for i in want_index]


def probe_collisions(p, n=2049, n_keys=300):
    """engines created with FLAG_TEST_WEAK_HASH: six bits of the hash reach the election, distinct keys share cells, the host decides"""
    K = Keys(False)
    rng = np.random.default_rng(99)
    pool = K.take(n_keys)
    p.make_resident(pool[::2])
    before = p.front.store_stats()["collisions"]
    keys = [pool[i] for i in rng.integers(0, n_keys, n)]
    beh = np.where(rng.random(n) < 0.001, RESET_REMAINING, 0).astype(np.uint32)
    beh[:n // 2] = 0                                                 # (a cut in the second half, if any: most of the list stays)
    p.check("collisions", keys, beh)
    p.check("collisions, no reset", keys)
    assert p.front.store_stats()["collisions"] == before + 2, p.front.store_stats()
