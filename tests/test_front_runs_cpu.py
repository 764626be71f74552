"""tests/front_runs.py itself: that its plans are the engine distributions they claim, that the keys it chooses go where the plan says
under the placement's untouched rule (the reference's getWorker) — by an XXH64 written in plain Python, not by the router that chose them —
and that its generations visit every size, width and plan, with a packed generation in every ragged one's slot.  No engine and no GPU."""
import collections

import numpy as np
import pytest

import gubernator_amd as ga
import front_edges as fe
import front_runs as frn


@pytest.mark.parametrize("E", frn.ENGINE_COUNTS)
def test_the_plans_are_the_distributions_they_claim(E):
    T, mid, lone = frn.TILE, E // 2, frn.lone_engine(E)
    for n in frn.SIZES:
        tiles = [slice(t, min(t + T, n)) for t in range(0, n, T)]
        p = {kind: frn.plan(kind, n, E) for kind in frn.PLANS}
        assert all(len(v) == n and v.dtype == np.uint32 and v.max() < E for v in p.values())
        assert (p["one"] == mid).all() and (p["last"] == E - 1).all()
        assert set(p["ends"].tolist()) <= {0, E - 1} and (n < 4 or set(p["ends"].tolist()) == {0, E - 1})
        assert (p["mod"] == np.arange(n) % E).all()
        for kind, at in (("single_first", tiles[-1].start), ("single_last", tiles[0].stop - 1)):
            assert p[kind][at] == lone
            if E > 1:
                assert (p[kind] == lone).sum() == 1
                assert n < 2 * E or set(p[kind].tolist()) == set(range(E))           # (the others share the rest)
        last = tiles[-1]
        if last.stop - last.start < T:                                               # a last partial tile: only the middle engine
            assert (p["tail_middle"][last] == mid).all()
            assert (p["tail_middle"][:last.start] == np.arange(last.start) % E).all()
        else:
            assert (p["tail_middle"] == np.arange(n) % E).all()
        at = frn.run_end(p["mod"])
        e = p["mod"][at]
        assert at < T and not (p["mod"][at + 1:T] == e).any()                         # the last of its engine in the first tile: a run's end


@pytest.mark.parametrize("E", frn.ENGINE_COUNTS)
def test_the_generations_go_where_their_plans_say_and_visit_everything(E):
    place = ga.Placement(E) if E > 1 else None
    route = (lambda keys: place.route_keys(*fe.pack(keys))[0]) if place is not None else None
    gens = list(frn.generations(E, route, np.random.default_rng(11 + E), depth=3))
    assert len(gens) == len(frn.SIZES) * (1 + len(frn.PLANS))
    seen, widths, ragged_at = collections.Counter(), set(), []
    cache, keys_of_engine = {}, collections.defaultdict(set)
    for g, (label, hb, full, engines) in enumerate(gens):
        assert full == (g % 2 == 1) and (hb.burst is not None) == full and (hb.created_at is not None) == full and (hb.is_owner is not None) == full
        assert len(hb.key_bytes) == int(hb.key_off[-1]) + 8 and hb.odd is None and hb.for_oracle is hb
        kb, off = hb.key_bytes.tobytes(), hb.key_off.tolist()
        lens = np.diff(hb.key_off.astype(np.int64))
        kind = label.split()[2]
        seen[(hb.n, kind)] += 1
        odd = np.nonzero(lens != np.bincount(lens).argmax())[0]
        if len(odd):                                                                 # ragged: ONE key of another width, at a run's end
            assert kind == "mod" and len(odd) == 1 and lens[odd[0]] == frn.ODD_WIDTH and odd[0] == frn.run_end(engines)
            ragged_at.append(g)
        else:
            widths.add(int(lens[0]))
        assert set(lens.tolist()) <= set(frn.WIDTHS) | {frn.ODD_WIDTH}
        for i in range(hb.n):                                                        # every key's engine by the plain-Python hash
            k = kb[off[i]:off[i + 1]]
            if k not in cache:
                cache[k] = place.shard(fe.xxh64(k)) if place is not None else 0
                keys_of_engine[cache[k]].add(k)
            assert cache[k] == engines[i], (label, i, k)
        assert (engines == frn.plan(kind, hb.n, E)).all()
    assert widths == set(frn.WIDTHS)
    assert set(seen) == {(n, kind) for n in frn.SIZES for kind in frn.PLANS} and all(seen[(n, "mod")] == 2 for n in frn.SIZES)
    assert len(ragged_at) == sum(n > 1 for n in frn.SIZES)
    for g in ragged_at:                                                              # three generations later, in the same slot: packed, same size
        later = gens[g + 3][1]
        assert later.n == gens[g][1].n and len(set(np.diff(later.key_off.astype(np.int64)).tolist())) == 1
        assert set(np.diff(later.key_off.astype(np.int64)).tolist()) < set(np.diff(gens[g][1].key_off.astype(np.int64)).tolist())
    # the caches of the GPU test bind: every engine is offered more keys than it holds
    assert min(len(v) for v in keys_of_engine.values()) > frn.CACHE_PER_ENGINE and len(keys_of_engine) == E
    if place is not None:
        place.close()
