"""Cases for the cache operations — the calls that put items into a table and take them out without evaluating requests: guber_add_items,
guber_add_items_dev, guber_get_item, guber_remove_item, guber_dump, guber_move_items_by_hash, with guber_compact between them (kernels:
gubernator_amd/csrc/guber_kernels_ops.h, host side: engine_items.inl) — beyond one workgroup; shared by tests/test_gpu_cache_ops.py (the
product library on a GPU) and tests/test_cache_ops_cpu.py (the same kernels compiled for the CPU).  numpy plus support / streams only.
Every case takes an engine factory (keyword arguments of gubernator_amd.Engine -> engine); the case of the device columns also takes
upload(numpy array) -> (keepalive, pointer) and download(keepalive) -> numpy array, as the mesh cases do.

Every comparison is element-wise and bit-exact against support.Oracle: the `existed` flags of every Add, size() after every call, each()
sorted by key (its order is unspecified on both sides) with every field of item_dict — float fields by their bit pattern, so a NaN equals
itself —, unexpired_evictions where the cache binds.  No case skips or filters items.

  a  Add across workgroups: calls of 1, 255, 256, 257 and 3 000 items (k_items_probe / k_items_commit run 256 items per workgroup; the engine's
     max_batch is 256), a fifth of the keys 100 bytes; the same keys again with other values
  b  Add of 1 200 keys + 300 duplicates under GUBER_FLAG_TEST_WEAK_HASH: 64 tags, one wave of the host's resubmission per key of a tag
  c  a binding cache (900) over a small table (2 048): twelve rounds of 500 new items with Get and Remove between them, the rebuild runs
  d  an Add larger than the cache, then items one by one: each evicts the reference's victim
  e  extreme fields: int64 bounds, NaN, infinities, -0.0, denormals, under keys with NUL and 0xff bytes
  f  guber_dump's buffer protocol: sizes first, exact capacities, one short, an empty engine
  g  restart: dump -> load into an engine of another geometry -> continue the stream against the oracle that never restarted
  h  guber_add_items_dev: the columns of (a), with and without the optional ones; a call with duplicate keys
  i  guber_move_items_by_hash across workgroups, into a destination with a smaller max_key_bytes, and into one without room"""
import ctypes as C
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)                          # (run as a script: the package is importable from the repository tree)

import streams
import support
from support import GuberItem, HostBatch, Oracle

WEAK_HASH = 1
OK, E_TABLE_FULL, E_NOMEM = 0, -5, -6                 # include/guber_gpu.h
HOUR = 3_600_000
NOW = streams.NOW0
FIELDS = ("key", "algorithm", "status", "limit", "duration", "remaining", "remaining_f", "stamp", "burst", "expire_at", "invalid_at")


def _lib():
    import gubernator_amd as ga
    return ga.lib()


def xxh(key):
    return support.oracle_lib().oracle_xxhash64(key, len(key), 0)


def f64_bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def canon(d):
    """an item_dict as a tuple in the order of FIELDS, remaining_f by its bits"""
    return tuple(f64_bits(d[f]) if f == "remaining_f" else d[f] for f in FIELDS)


def listing(x):
    """each() of an engine or of the oracle, sorted by key"""
    return sorted(canon(d) for d in x.each())


def assert_listings_equal(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} items, the reference has {len(want)}"
    for a, b in zip(got, want):
        if a != b:
            if a[0] != b[0]:
                raise AssertionError(f"{what}: key {a[0][:40]!r} where the reference has {b[0][:40]!r}")
            f = [n for n, x, y in zip(FIELDS, a, b) if x != y]
            raise AssertionError(f"{what}: item {a[0][:40]!r} differs in {f}: got {a} want {b}")


def assert_same_items(e, o, what):
    assert_listings_equal(listing(e), listing(o), what)
    assert e.size() == o.size(), f"{what}: size {e.size()}, the reference has {o.size()}"


def mk(spec):
    return support.make_item(**spec)


def add_both(e, o, specs, now, what, want_existed=None):
    """one guber_add_items call and the reference's item-by-item Add: the existed flags element-wise, the sizes -> the flags"""
    items = [mk(s) for s in specs]
    e.set_clock(now)
    want = [o.add_item(it, now) for it in items]
    got = e.add_items(items)
    bad = [i for i in range(len(items)) if got[i] != want[i]]
    assert not bad, f"{what}: existed differs at {len(bad)} of {len(items)} items; first at {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"
    if want_existed is not None:
        assert all(x == want_existed for x in want), (what, want_existed)
    assert e.size() == o.size(), f"{what}: size {e.size()}, the reference has {o.size()}"
    return want


def get_both(e, o, key, now, what):
    ge, go = e.get_item(key, now), o.get_item(key, now)
    assert (ge is None) == (go is None) and (ge is None or canon(ge) == canon(go)), f"{what}: get_item({key[:40]!r}): got {ge} want {go}"
    return go


# ---- a ----------------------------------------------------------------------------------------------------------------------------
SIZES_A = (1, 255, 256, 257, 3000)


def items_a(n, base, salt, now=NOW):
    """items base .. base + n: a fifth of the keys 100 bytes, token / leaky / no Value mixed; `salt` changes every value but not the keys"""
    out = []
    for i in range(base, base + n):
        key = b"ca_%05d" % i
        if i % 5 == 0:
            key = key.ljust(100, b"L")
        out.append(dict(key=key, algorithm=(0, 1, 0, 1, 0, 1, 9)[i % 7], limit=1000 + i + 7919 * salt, duration=60_000 + i, remaining=(i * 7 + salt) % 1000,
                        remaining_f=(i + salt) * 0.25, stamp=now - i - salt, burst=i % 13 + salt, expire_at=now + HOUR + i + salt,
                        invalid_at=now + 2 * HOUR + i if i % 9 == 0 else 0, status=(i + salt) & 1))
    return out


def case_add_across_workgroups(factory):
    e, o = factory(cache_size=8192, max_batch=256), Oracle(cache_size=8192)
    for salt, existed in ((0, False), (1, True)):                          # new keys; the same keys with other values: the last value wins
        base = 0
        for n in SIZES_A:
            add_both(e, o, items_a(n, base, salt), NOW + salt, f"add of {n} items, values {salt}", want_existed=existed)
            assert_same_items(e, o, f"after the add of {n} items, values {salt}")
            base += n
    assert e.size() == sum(SIZES_A)
    e.close(); o.close()


# ---- b ----------------------------------------------------------------------------------------------------------------------------
def keys_b(n=1200):
    """ci_0 .. ci_<n-1>, padded to 0 / 0 / 63 / 64 / 200 bytes by i % 5 (62 bytes is the longest inline key)"""
    return [(b"ci_%d" % i).ljust((0, 0, 63, 64, 200)[i % 5], b"p") for i in range(n)]


def case_add_with_duplicates_under_colliding_tags(factory):
    import xxhash
    keys = keys_b()
    rng = np.random.default_rng(11)
    seq = keys + [keys[int(i)] for i in rng.choice(len(keys), 300, replace=False)]
    seq = [seq[int(i)] for i in rng.permutation(len(seq))]
    # the host resubmits a call's items in waves and gives up after 64.  Every wave settles one more entry of a tag — the key that inserted it is
    # applied in that wave if it is the lowest index at the entry, in the next one otherwise —, so a tag of m keys takes at most m + 1 waves:
    # the fullest tag (28 keys here) stays well below the bound
    per_tag = {}
    for k in keys:
        assert xxhash.xxh64(k, seed=0).intdigest() == xxh(k)
        per_tag.setdefault(xxh(k) & 0x1f80, []).append(k)
    fullest = max(len(v) for v in per_tag.values())
    assert len(per_tag) == 64 and fullest <= 48, (len(per_tag), fullest)
    e, o = factory(cache_size=4096, flags=WEAK_HASH), Oracle(cache_size=4096)
    specs = [dict(key=k, algorithm=j & 1, limit=10_000 + j, duration=HOUR, remaining=j % 97, remaining_f=j * 0.5, stamp=NOW - j, burst=j % 5,
                  expire_at=NOW + HOUR + j) for j, k in enumerate(seq)]            # (a limit of its own: the LAST item of a key is recognisable)
    want = add_both(e, o, specs, NOW, "1 200 keys + 300 duplicates under 64 tags")
    assert sum(want) == 300
    assert_same_items(e, o, "after the add under colliding tags")
    assert e.size() == 1200
    spread = [v[len(v) // 2] for _, v in sorted(per_tag.items())][:40]
    absent, i = [], 0
    while len(absent) < 5:                                                # (absent keys whose tag present keys have)
        k = (b"ci_absent_%d" % i).ljust((0, 63, 200)[i % 3], b"p")
        if xxh(k) & 0x1f80 in per_tag:
            absent.append(k)
        i += 1
    for k in spread:
        assert get_both(e, o, k, NOW + 1, "a key of every tag") is not None
    for k in absent:
        assert get_both(e, o, k, NOW + 1, "an absent key under a present tag") is None
    assert_same_items(e, o, "after the gets under colliding tags")
    e.close(); o.close()


# ---- c ----------------------------------------------------------------------------------------------------------------------------
def case_a_binding_cache_and_the_rebuild(factory):
    e, o = factory(cache_size=900, max_batch=128, table_slots=2048), Oracle(cache_size=900)
    now, seen = NOW, []
    for rnd in range(12):
        e.set_clock(now)
        specs = []
        for j in range(500):
            i = rnd * 500 + j
            key = (b"cc_%02d_%03d" % (rnd, j)).ljust(70 if i % 4 == 0 else 0, b"c")
            specs.append(dict(key=key, algorithm=i & 1, limit=100 + i, duration=HOUR, remaining=i % 100, remaining_f=i * 0.125, stamp=now,
                              expire_at=now + (50 if i % 6 == 0 else HOUR)))
            seen.append(key)
        add_both(e, o, specs, now, f"round {rnd}", want_existed=False)
        for k in seen[::37]:
            get_both(e, o, k, now, f"round {rnd}")
        for k in seen[::91]:
            e.remove_item(k); o.remove_item(k)
        assert_same_items(e, o, f"after round {rnd}")
        assert e.counters()[:4] == o.counters(), f"round {rnd}: (over the limit, hits, misses, unexpired evictions) {e.counters()[:4]}, the reference has {o.counters()}"
        now += 40
    st = e.stats()
    assert st["compactions"] > 0, st
    assert st["unexpired_evictions"] == o.counters()[3] > 0, (st, o.counters())
    e.close(); o.close()


# ---- d ----------------------------------------------------------------------------------------------------------------------------
def case_an_add_larger_than_the_cache(factory):
    e, o = factory(cache_size=300), Oracle(cache_size=300)

    def spec(i):
        return dict(key=(b"cd_%04d" % i).ljust(80 if i % 3 == 0 else 0, b"d"), algorithm=i & 1, limit=i, duration=HOUR, remaining=i % 10,
                    remaining_f=i * 0.5, stamp=NOW, expire_at=NOW + HOUR)
    add_both(e, o, [spec(i) for i in range(1000)], NOW, "1 000 items into a cache of 300", want_existed=False)
    assert_same_items(e, o, "after 1 000 items into a cache of 300")
    assert sorted(d["limit"] for d in e.each()) == list(range(700, 1000))          # (the last 300 survive)
    for i in range(1000, 1050):                                                    # one per call: each evicts exactly the reference's victim
        add_both(e, o, [spec(i)], NOW + 1, f"item {i}", want_existed=False)
        assert_same_items(e, o, f"after item {i}")
    assert e.counters()[3] == o.counters()[3] == 750, (e.counters(), o.counters())
    e.close(); o.close()
    # the same with keys that come twice: the host applies such a call in several launches, and the order among the call's keys stays that
    # of the CALL — row 4 q + 3 is followed by the key of row 4 q once more, with another value; the first of them are among those that leave
    e, o = factory(cache_size=300), Oracle(cache_size=300)
    rows = []
    for i in range(400):
        rows.append(spec(2000 + i))
        if i % 4 == 3:
            rows.append(dict(spec(2000 + i - 3), limit=-i))
    want = add_both(e, o, rows, NOW, "500 rows, 100 of them a key once more, into a cache of 300")
    assert sum(want) == 100
    assert_same_items(e, o, "after 500 rows into a cache of 300")
    assert 0 < sum(d["limit"] < 0 for d in e.each()) < 100
    e.close(); o.close()


# ---- e ----------------------------------------------------------------------------------------------------------------------------
INTS = (0, 1, -1, 2 ** 63 - 1, -2 ** 63, 2 ** 53, 2 ** 62)
FLOATS = (float("nan"), float("inf"), float("-inf"), -0.0, 5e-324, 0.0, 1.5, -1.7976931348623157e308, 2.2250738585072014e-308)


def items_e():
    out = []
    for algo in (0, 1, 9):
        for rot in range(len(INTS)):
            for fi, f in enumerate(FLOATS):
                idx = len(out)
                v = [INTS[(rot + q + fi) % len(INTS)] for q in range(5)]
                length = 4 + idx * 96 // (3 * len(INTS) * len(FLOATS) - 1)          # 4 .. 100 bytes
                key = (b"e\x00" + bytes([idx]) + b"\xff" + b"\x00\xff\x00k" * 24)[:length]
                out.append(dict(key=key, algorithm=algo, limit=v[0], duration=v[1], remaining=v[2], stamp=v[3], burst=v[4], remaining_f=f,
                                expire_at=NOW + HOUR, invalid_at=NOW + HOUR if idx % 4 == 0 else 0, status=idx & 1))
    assert len({s["key"] for s in out}) == len(out) == 189 and {len(out[0]["key"]), len(out[-1]["key"])} == {4, 100}
    return out


def case_extreme_fields(factory):
    e, o = factory(cache_size=1024, max_batch=256), Oracle(cache_size=1024)
    specs = items_e()
    add_both(e, o, specs, NOW, "extreme fields", want_existed=False)
    assert_same_items(e, o, "extreme fields")
    nan = [d for d in e.each() if d["remaining_f"] != d["remaining_f"]]
    assert len(nan) == len(INTS), len(nan)                                         # (the leaky items keep their NaN: the comparison was not vacuous)
    for s in specs:
        assert get_both(e, o, s["key"], NOW + 1, "extreme fields") is not None
    assert_same_items(e, o, "extreme fields, after the gets")
    e.close(); o.close()


# ---- f ----------------------------------------------------------------------------------------------------------------------------
GUARD = 0xA5


def dump_raw(e, cap, arena_cap, with_buffers=True, guard_items=4, guard_bytes=64):
    """guber_dump into buffers of exactly cap items / arena_cap bytes with a guard pattern behind both -> (rc, n_out, arena_out, items, guards intact)"""
    L = _lib()
    n, a = C.c_uint64(0), C.c_uint64(0)
    if not with_buffers:
        return L.guber_dump(e.h, None, 0, None, 0, C.byref(n), C.byref(a)), n.value, a.value, [], True
    items = (GuberItem * (cap + guard_items))()
    arena = (C.c_uint8 * (arena_cap + guard_bytes))()
    C.memset(items, GUARD, C.sizeof(items))
    C.memset(arena, GUARD, C.sizeof(arena))
    rc = L.guber_dump(e.h, items, cap, arena, arena_cap, C.byref(n), C.byref(a))
    tail_i = C.string_at(C.addressof(items) + cap * C.sizeof(GuberItem), guard_items * C.sizeof(GuberItem))
    tail_a = C.string_at(C.addressof(arena) + arena_cap, guard_bytes)
    intact = tail_i == bytes([GUARD]) * len(tail_i) and tail_a == bytes([GUARD]) * len(tail_a)
    got = [support.item_dict(items[i]) for i in range(n.value)] if rc == OK else []
    return rc, n.value, a.value, got, intact


def case_the_dump_protocol(factory):
    e, o = factory(cache_size=4096, max_batch=256), Oracle(cache_size=4096)
    assert dump_raw(e, 0, 0, with_buffers=False)[:3] == (OK, 0, 0)                  # an empty engine
    assert dump_raw(e, 0, 0)[:3] == (OK, 0, 0)
    specs = [dict(key=(b"cf_%03d" % i).ljust(100 if i % 3 == 0 else 0, b"f"), algorithm=i & 1, limit=i, duration=HOUR, remaining=i, remaining_f=i * 0.5,
                  stamp=NOW, expire_at=NOW + HOUR) for i in range(700)]
    add_both(e, o, specs, NOW, "700 items", want_existed=False)
    need = sum(len(s["key"]) for s in specs)
    assert dump_raw(e, 0, 0, with_buffers=False)[:3] == (E_NOMEM, 700, need)        # sizes first
    rc, n, a, got, intact = dump_raw(e, 700, need)                                  # exactly enough
    assert (rc, n, a) == (OK, 700, need) and intact, (rc, n, a, intact)
    assert_listings_equal(sorted(canon(d) for d in got), listing(o), "the dump into buffers that are exactly enough")
    for cap, acap in ((699, need), (700, need - 1), (699, need - 1), (0, 0)):       # one short
        rc, n, a, _, intact = dump_raw(e, cap, acap)
        assert (rc, n, a) == (E_NOMEM, 700, need) and intact, (cap, acap, rc, n, a, intact)
    assert_same_items(e, o, "after the dumps")
    e.close(); o.close()


# ---- g ----------------------------------------------------------------------------------------------------------------------------
def case_restart(factory, compact_first):
    a, o = factory(cache_size=4096, max_batch=1024, max_key_bytes=300), Oracle(cache_size=4096)
    batches = list(streams.adversarial_batches(5, 12, 700, greg_fn=support.gregorian))
    for j, b in enumerate(batches[:8]):
        support.assert_results_equal(a.eval(b), o.eval(b), f"batch {j} before the restart")
    now = batches[7].now_ms
    if compact_first:
        a.compact(now)
    assert_same_items(a, o, "before the restart")                                  # (expired and reset items included)
    dump = sorted(a.each(), key=lambda d: d["key"])
    a.close()
    b2 = factory(cache_size=2048, table_slots=8192, max_batch=1024, max_key_bytes=300)
    b2.set_clock(now)
    assert b2.add_items([mk(d) for d in dump]) == [False] * len(dump)
    assert_same_items(b2, o, "after the reload")
    for j, b in enumerate(batches[8:]):
        support.assert_results_equal(b2.eval(b), o.eval(b), f"batch {8 + j}, after the restart")
    assert_same_items(b2, o, "at the end")
    b2.close(); o.close()


# ---- h ----------------------------------------------------------------------------------------------------------------------------
class GuberItemsDev(C.Structure):                                              # guber_items_dev_t
    _fields_ = [("n", C.c_uint32), ("reserved", C.c_uint32), ("key_bytes", C.c_void_p), ("key_off", C.c_void_p),
                ("algorithm", C.c_void_p), ("status", C.c_void_p), ("limit", C.c_void_p), ("duration", C.c_void_p),
                ("remaining", C.c_void_p), ("remaining_f", C.c_void_p), ("stamp", C.c_void_p), ("burst", C.c_void_p),
                ("expire_at", C.c_void_p), ("invalid_at", C.c_void_p)]


OPTIONAL = ("status", "burst", "invalid_at")


def add_dev(e, specs, now, optional, upload, download):
    """one guber_add_items_dev call over the specs as device columns (the optional columns NULL unless `optional`) -> result bytes"""
    L = _lib()
    L.guber_add_items_dev.argtypes = [C.c_void_p, C.POINTER(GuberItemsDev), C.c_void_p]
    n = len(specs)
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(s["key"]) for s in specs])
    cols = dict(key_bytes=np.frombuffer(b"".join(s["key"] for s in specs) + b"\0" * 8, np.uint8).copy(), key_off=off)
    for name, dt in (("algorithm", np.uint8), ("status", np.uint8), ("limit", np.int64), ("duration", np.int64), ("remaining", np.int64),
                     ("remaining_f", np.float64), ("stamp", np.int64), ("burst", np.int64), ("expire_at", np.int64), ("invalid_at", np.int64)):
        cols[name] = np.array([s.get(name, 0) for s in specs], dtype=dt)
    up = {k: upload(v) for k, v in cols.items() if optional or k not in OPTIONAL}
    res = upload(np.full(n, 0xEE, np.uint8))
    it = GuberItemsDev(n, 0, *[up[f][1] if f in up else None for f, _ in GuberItemsDev._fields_[2:]])
    e.set_clock(now)
    rc = L.guber_add_items_dev(e.h, C.byref(it), res[1])
    assert rc == OK, (rc, L.guber_last_error())
    e.synchronize()
    return np.asarray(download(res[0])).astype(np.uint8)


def without_optional(spec):
    return dict(spec, status=0, burst=0, invalid_at=0)


def case_device_columns(factory, upload, download):
    for optional in (True, False):
        e, o = factory(cache_size=8192, max_batch=256), Oracle(cache_size=8192)
        for salt in (0, 1):
            for n, base in ((257, 0), (3000, 1000)):
                specs = items_a(n, base, salt)
                fed = specs if optional else [without_optional(s) for s in specs]
                want = np.array([o.add_item(mk(s), NOW + salt) for s in fed], np.uint8)
                got = add_dev(e, specs, NOW + salt, optional, upload, download)
                assert np.array_equal(got, want), f"{n} rows, optional columns {optional}, values {salt}: results differ at {np.nonzero(got != want)[0][:5]}: {got[got != want][:5]}"
                assert (want == salt).all()
                assert_same_items(e, o, f"{n} rows, optional columns {optional}, values {salt}")
        e.close(); o.close()
    # 20 new keys twice in one call, among 300 rows; the second occurrences right behind the first (one wavefront), 100 rows on (another
    # wavefront of the workgroup) and in the next workgroup.  include/guber_gpu.h: the first occurrence of a new key is applied, every later one reports 0xFF and
    # changes nothing; resubmitted, it finds the key resident — the last value wins, as in the reference
    e, o = factory(cache_size=8192, max_batch=256), Oracle(cache_size=8192)
    first = items_a(300, 5000, 0)
    rows, second = list(first), {}
    for q in range(20):
        src = (3 * q, 3 * q, 130 + q, 7 + q)[q % 4]                               # (twenty different rows of `first`)
        dup = items_a(1, 5000 + src, 1)[0]                                        # the same key with other values
        behind = (1, 100, 150, len(rows))[q % 4]
        rows.insert(min(len(rows), rows.index(first[src]) + behind), dup)
    seen = set()
    for i, s in enumerate(rows):
        if s["key"] in seen:
            second[i] = s
        seen.add(s["key"])
    assert len(rows) == 320 and len(second) == 20 and len(seen) == 300
    want = [o.add_item(mk(s), NOW) for s in rows]
    got = add_dev(e, rows, NOW, True, upload, download)
    for i in range(len(rows)):
        if i in second:
            assert got[i] == 0xFF, f"row {i}, the second occurrence of its key: result {got[i]:#x}"
            assert want[i] is True
        else:
            assert got[i] == int(want[i]) == 0, f"row {i}: result {got[i]:#x}, the reference's existed is {want[i]}"
    assert e.size() == o.size() == 300
    again = [rows[i] for i in sorted(second)]
    got = add_dev(e, again, NOW, True, upload, download)
    assert (got == 1).all(), got
    assert_same_items(e, o, "after the 0xFF rows were resubmitted")
    e.close(); o.close()
    # the same over entries that exist and hold no item: of 350 keys in a cache of 300 the first 50 are evicted, 100 more are removed, the table
    # is not rebuilt; one call holds ten keys of either kind twice — side by side, and some thirty rows on — among 30 new ones
    e, o = factory(cache_size=300, max_batch=256), Oracle(cache_size=300)
    old = items_a(350, 7000, 0)
    add_both(e, o, old[:300], NOW, "300 items", want_existed=False)
    add_both(e, o, old[300:], NOW + 1, "50 more: the first 50 leave", want_existed=False)
    for s in old[100:200]:
        e.remove_item(s["key"]); o.remove_item(s["key"])
    assert e.size() == o.size() == 200
    gone = old[0:50:5] + old[100:200:10]
    for s in gone:
        assert get_both(e, o, s["key"], NOW + 1, "an evicted or removed key") is None
    back = [dict(s, limit=-1 - j) for j, s in enumerate(gone)]
    rows = items_a(30, 9000, 0)
    for j, s in enumerate(back):
        rows.insert(2 * j, s)
        rows.insert(2 * j + (1 if j % 2 else 32), dict(s, limit=-100 - j, remaining=j))
    seen, second = set(), set()
    for i, s in enumerate(rows):
        if s["key"] in seen:
            second.add(i)
        seen.add(s["key"])
    assert len(rows) == 70 and len(second) == 20 and len(seen) == 50
    want = [o.add_item(mk(s), NOW + 2) for s in rows]
    got = add_dev(e, rows, NOW + 2, True, upload, download)
    assert e.stats()["compactions"] == 0                                            # (the entries of the keys that had left were still there)
    for i in range(len(rows)):
        assert got[i] == (0xFF if i in second else 0), f"row {i} ({'second' if i in second else 'first'} occurrence of a key that had left, or a new key): result {got[i]:#x}"
        assert want[i] == (i in second)
    assert e.size() == o.size() == 250, (e.size(), o.size())
    got = add_dev(e, [rows[i] for i in sorted(second)], NOW + 2, True, upload, download)
    assert (got == 1).all(), got
    assert_same_items(e, o, "after the 0xFF rows of keys that had left were resubmitted")
    e.close(); o.close()


# ---- i ----------------------------------------------------------------------------------------------------------------------------
NOTHING = 0x1234567890abcdef                                                       # a hash that names no key
TO_KEY = 128


def keys_i(n=200):
    """mv_000 .. padded to 0 / 70 / 128 / 129 / 200 bytes by i % 5: 128 is the longest key the destination holds, 129 still fits the
    move's staging row (min(max_key_bytes) + 16, rounded up to a multiple of 8 — 144 here: the destination refuses it and it goes back), 200
    does not (it never leaves)"""
    ks = [(b"mv_%03d" % i).ljust((0, 70, 128, 129, 200)[i % 5], b"m") for i in range(n)]
    assert all(xxh(k) != NOTHING for k in ks)
    return ks


def move(frm, to, hashes):
    """guber_move_items_by_hash -> (rc, moved)"""
    L = _lib()
    L.guber_move_items_by_hash.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32)]
    arr = (C.c_uint64 * max(len(hashes), 1))(*[int(h) for h in hashes])
    moved = C.c_uint32(0xEEEE)
    return L.guber_move_items_by_hash(frm.h, to.h, arr, len(hashes), C.byref(moved)), moved.value


def specs_i(keys):
    return [dict(key=k, algorithm=i & 1, limit=100, duration=HOUR, remaining=50 + i % 7, remaining_f=40.5 + i % 5, stamp=NOW, burst=100 if i & 1 else 0,
                 expire_at=NOW + HOUR) for i, k in enumerate(keys)]


def pair(factory, **to_kw):
    frm = factory(cache_size=4096, max_batch=256, max_key_bytes=256)
    to = factory(stream=frm.stream_handle(), **dict(dict(cache_size=4096, max_batch=256, max_key_bytes=TO_KEY), **to_kw))
    return frm, to


def check_move(frm, to, before, what):
    """the two tables after a move: disjoint, together what they held before, item by item -> (listing of frm, listing of to)"""
    lf, lt = listing(frm), listing(to)
    both = {x[0] for x in lf} & {x[0] for x in lt}
    assert not both, f"{what}: {len(both)} keys are in both tables; first {sorted(both)[0][:40]!r}"
    assert_listings_equal(sorted(lf + lt), before, what)
    return lf, lt


def case_moves(factory, list_len):
    """a list of list_len hashes (0 = all 200 keys and three more entries) from a table with max_key_bytes 256 into one with 128"""
    keys = keys_i()
    frm, to = pair(factory)
    o = Oracle(cache_size=8192)
    add_both(frm, o, specs_i(keys), NOW, "200 items", want_existed=False)
    before = listing(frm)
    if list_len == 1:
        listed, hashes = keys[:1], [xxh(keys[0])]
    else:
        listed = keys[:list_len - 2] if list_len else keys
        hashes = [xxh(k) for k in listed]
        hashes.insert(3, hashes[2])                                               # one hash twice, side by side: two lanes of one wavefront
        hashes.insert(len(hashes) // 2, NOTHING)
        if not list_len:
            hashes.append(hashes[0])                                              # and once more, three workgroups apart
    assert list_len in (0, len(hashes))
    rc, moved = move(frm, to, hashes)
    what = f"a list of {len(hashes)} hashes"
    lf, lt = check_move(frm, to, before, what)
    want_in_to = sorted(k for k in listed if len(k) <= TO_KEY)
    assert [x[0] for x in lt] == want_in_to, f"{what}: {len(lt)} keys in the destination, {len(want_in_to)} of the list fit it"
    assert moved == len(lt), (what, moved, len(lt))
    assert frm.size() == len(lf) and to.size() == len(lt) and frm.size() + to.size() == 200, (what, frm.size(), to.size())
    # include/guber_gpu.h: a bucket the destination refused is back in its table and the call says GUBER_E_TABLE_FULL
    went_back = [k for k in listed if TO_KEY < len(k) <= TO_KEY + 16]
    assert rc == (E_TABLE_FULL if went_back else OK), (what, rc, len(went_back))
    # one batch over all 200 keys, split by where each key lives, against ONE oracle
    in_to = {x[0] for x in lt}
    for eng, part in ((to, [i for i, k in enumerate(keys) if k in in_to]), (frm, [i for i, k in enumerate(keys) if k not in in_to])):
        if part:
            b = HostBatch([keys[i] for i in part], 1, 100, HOUR, NOW + 5, algorithm=[i & 1 for i in part], burst=[100 if i & 1 else 0 for i in part])
            support.assert_results_equal(eng.eval(b), o.eval(b), f"{what}: the batch after the move, {len(part)} keys")
    assert_listings_equal(sorted(listing(frm) + listing(to)), listing(o), f"{what}: after the batch")
    to.close(); frm.close(); o.close()


def case_a_move_of_keys_too_long_to_stage(factory):
    """only keys of 200 bytes: they never leave their table, nothing is refused"""
    keys = keys_i()
    frm, to = pair(factory)
    o = Oracle(cache_size=8192)
    add_both(frm, o, specs_i(keys), NOW, "200 items", want_existed=False)
    rc, moved = move(frm, to, [xxh(k) for k in keys if len(k) == 200])
    assert (rc, moved) == (OK, 0), (rc, moved)
    assert to.size() == 0 and to.each() == []
    assert_same_items(frm, o, "after a move of keys too long to stage")
    to.close(); frm.close(); o.close()


def case_a_move_into_a_table_without_room(factory):
    """the destination: 256 slots, 60 items of its own; of 200 listed keys (all of a length it holds) it takes what it has entries for, the others
    go back through k_items_restore.  Counted in the listings: guber_size would bring the destination down to its cache_size of 64."""
    keys = [(b"mr_%03d" % i).ljust((0, 70, 128)[i % 3], b"r") for i in range(200)]
    frm, to = pair(factory, table_slots=256, cache_size=64)
    o, o_to = Oracle(cache_size=8192), Oracle(cache_size=8192)
    add_both(frm, o, specs_i(keys), NOW, "200 items", want_existed=False)
    add_both(to, o_to, specs_i([b"own_%02d" % i for i in range(60)]), NOW, "the destination's own 60", want_existed=False)
    before = sorted(listing(frm) + listing(to))
    rc, moved = move(frm, to, [xxh(k) for k in keys])
    lf, lt = check_move(frm, to, before, "a destination without room")
    assert rc == E_TABLE_FULL, rc
    assert 0 < moved < 200 and moved == len(lt) - 60 and len(lf) == 200 - moved, (moved, len(lf), len(lt))
    assert len(lt) <= 256
    assert frm.size() == len(lf), (frm.size(), len(lf))
    assert to.size() == 64                                                        # (now the destination's cache binds: the oldest leave, as after any Add)
    to.close(); frm.close(); o.close(); o_to.close()


LIST_LENS = (1, 63, 64, 65, 0)


def run_all(factory, upload, download):
    def step(name, fn, *a):
        fn(*a)
        print(f"{name}: ok", flush=True)
    step("a", case_add_across_workgroups, factory)
    step("b", case_add_with_duplicates_under_colliding_tags, factory)
    step("c", case_a_binding_cache_and_the_rebuild, factory)
    step("d", case_an_add_larger_than_the_cache, factory)
    step("e", case_extreme_fields, factory)
    step("f", case_the_dump_protocol, factory)
    for compact_first in (False, True):
        step(f"g (compact first: {compact_first})", case_restart, factory, compact_first)
    step("h", case_device_columns, factory, upload, download)
    for n in LIST_LENS:
        step(f"i ({n or 'all'})", case_moves, factory, n)
    step("i (too long to stage)", case_a_move_of_keys_too_long_to_stage, factory)
    step("i (no room)", case_a_move_into_a_table_without_room, factory)


if __name__ == "__main__":
    import gubernator_amd as ga
    assert "enginesim" in ga.LIB_PATH, "this entry is for the CPU build of the engine (GUBER_HIP_LIB): device arrays are numpy buffers there"
    run_all(lambda **kw: ga.Engine(**kw), upload=lambda a: (a, a.ctypes.data), download=lambda a: a)
    print("CACHE OPS CASES OK")
