"""tests/front_edges.py itself: its XXH64 against known answers, its keys, its tight key buffers, and that its generations visit what they
are there for.  No engine and no GPU."""
import collections

import numpy as np

import front_edges as fe
import scenarios


def test_the_plain_python_xxh64_has_the_known_answers():
    """tests/golden/kat_vectors.json "xxh64": the published values for four texts, and every length at which XXH64 takes another path
    (below and from 32 bytes; tails of 8, 4 and 1 bytes) with two seeds"""
    k = scenarios.load("kat_vectors.json")["xxh64"]
    assert fe.xxh64(b"") == 0xEF46DB3751D8E999 and fe.xxh64(b"abc") == 0x44BC2CF5AD770999      # (xxHash's own test values)
    for v in k["text"]:
        assert fe.xxh64(v["text"].encode(), v["seed"]) == v["xxh64"], v
    pat = bytes((37 * i + 11) % 251 + 1 for i in range(80))
    assert {v["len"] for v in k["vectors"]} >= {0, 1, 3, 4, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 40, 64}
    for v in k["vectors"]:
        assert fe.xxh64(pat[:v["len"]], v["seed"]) == v["xxh64"], v


def test_keys_and_tight_buffers():
    rng = np.random.default_rng(3)
    for W, count in ((1, 200), (2, 1500), (7, 600), (33, 600)):
        keys = fe.keys_of_width(W, count, rng)
        assert len(keys) == len(set(keys)) == count and all(len(k) == W and 0 not in k for k in keys)
    keys = [b"abc", b"", b"defgh"]
    kb, off = fe.pack(keys)
    assert off.dtype == np.uint32 and off.tolist() == [0, 3, 3, 8] and len(kb) == 8 + 8 and kb.base is None and bytes(kb[:8]) == b"abcdefgh"
    assert len(fe.pack(keys, slack=0)[0]) == 8 and len(fe.pack([])[0]) == 8


def test_the_generations_visit_every_width_size_and_position():
    gens = list(fe.generations(1, None, np.random.default_rng(5), depth=3))
    assert len(gens) == 69
    sizes_of, visits = collections.defaultdict(set), collections.Counter()
    for label, hb, full in gens:
        assert len(hb.key_bytes) == int(hb.key_off[-1]) + 8                      # exactly the promised 8 bytes behind the last key
        lens = np.diff(hb.key_off.astype(np.int64))
        if label.startswith("a "):
            assert len(set(lens.tolist())) == 1
            sizes_of[int(lens[0])].add(hb.n)
            visits[hb.n] += 1
        assert (hb.limit >= 5).all() and (hb.limit <= 30).all() and (hb.hits == 1).all() and set(hb.algorithm.tolist()) <= {0, 1}
        assert hb.n < 200 or set(hb.algorithm.tolist()) == {0, 1}
    assert set(sizes_of) == set(fe.PACKED_WIDTHS + fe.ONE_WIDTH_NOT_PACKED)
    assert all(2049 in s and len(s) >= 2 for s in sizes_of.values())
    assert set(visits) == set(fe.SIZES) and min(visits.values()) >= 2
    assert [full for _, _, full in gens] == [g % 2 == 1 for g in range(69)]
    assert {int(hb.duration[-2 if hb.n > 1 else 0]) for _, hb, _ in gens[2::3]} == {fe.SHORT_MS}     # (every third generation: keys expire)
    odd = [(hb.odd, hb) for _, hb, _ in gens if hb.odd is not None]
    assert sorted((kind, pos) for (pos, kind), _ in odd) == sorted((k, p) for k in ("neighbour", "empty", "too_long") for p in fe.ODD_POSITIONS)
    for (pos, kind), hb in odd:
        lens = np.diff(hb.key_off.astype(np.int64))
        assert hb.n == 2049 and (np.delete(lens, pos) == 15).all() and lens[pos] in {"neighbour": (14, 16), "empty": (0,), "too_long": (1025,)}[kind]
    idx = {id(hb): g for g, (_, hb, _) in enumerate(gens)}
    for _, hb in odd:                                                            # three generations later, in the same slot: one width again
        later = gens[idx[id(hb)] + 3][1]
        assert later.odd is None and set(np.diff(later.key_off.astype(np.int64)).tolist()) == {15}
    glob = [hb for label, hb, _ in gens if label.startswith("d ")]
    assert sorted({int(np.diff(hb.key_off.astype(np.int64))[0]) for hb in glob}) == list(fe.GLOBAL_WIDTHS)
    assert all(0.25 < ((hb.behavior & 2) != 0).mean() < 0.75 for hb in glob)
