// guber_wire_pool_peer.h — guber_wire_pool_update_peer_globals: the payload stage's entry for the owner's broadcast of GLOBAL buckets.
// Part of guber_engine.hip's translation unit, behind guber_wire_pool.h (it uses the pool's host rule and the engines' internals; kept apart
// from guber_wire_pool.h because that header is also compiled on its own, against stand-ins for the device, by the pool's race harness).
#pragma once

// V1Instance.UpdatePeerGlobals (gubernator.go:425-459) on the serialized message: the owner's broadcast of GLOBAL buckets, installed where this
// pool keeps GLOBAL state — the choice k_fr_count and wpl_direct make for a GLOBAL request: the GLOBAL engine when the rule has one, else the
// table XXH64 of the key picks.  The decode is the host transcoder's (a broadcast is at most 1000 items per sync interval); the install is ONE
// guber_add_items per engine touched.  guber_add_items takes the engine's mutex (engine_items.inl) — the lock launch_group holds for a stage's
// launches and guber_eval_batch for a caller's own RPC —, so a broadcast may arrive beside stages in flight and callers on the direct path: per
// engine it is applied before or after their batch, never in between.
extern "C" int guber_wire_pool_update_peer_globals(guber_wire_pool_t* p, const uint8_t* msg, size_t len, uint32_t* installed) {
    if (!p || (!msg && len)) return fail(GUBER_E_INVALID_ARG, "null argument");
    if (installed) *installed = 0;
    if (len == 0) return GUBER_OK;                                     // no globals
    if (p->closed.load(std::memory_order_acquire)) return fail(GUBER_E_WIRE_CLOSED, "guber_wire_pool: closed");
    const uint32_t bound = std::max(1u, wpl_count_records(msg, len));   // (exact for a well-formed message; the decoder refuses what does not fit)
    guber_wire_items_t* w = nullptr;
    int rc = guber_wire_items_create(bound, (uint32_t)std::min<size_t>(len, 0xffffffffu), &w);   // (the keys are part of the message)
    if (rc != GUBER_OK) return fail(rc, "guber_wire_items_create");
    std::unique_ptr<guber_wire_items_t, void (*)(guber_wire_items_t*)> hold(w, guber_wire_items_destroy);
    const guber_item_t* items = nullptr; uint32_t n = 0;
    rc = guber_wire_decode_globals(w, msg, len, wpl_now_ms(p), &items, &n);
    if (rc != GUBER_OK) return fail(rc, "guber_wire_pool: the message is turned away whole");
    // everything that could turn one item away is looked at before the first one is installed
    uint32_t max_key = p->eng[0]->max_key;                             // (the shortest max_key_bytes among the engines)
    for (guber_engine* e : p->eng) max_key = std::min(max_key, e->max_key);
    for (uint32_t i = 0; i < n; ++i) {
        if (items[i].key_len == 0) return fail(GUBER_E_INVALID_ARG, "guber_wire_pool: a global without a key (nothing was installed)");
        if (items[i].key_len > max_key) return fail(GUBER_E_KEY_TOO_LONG, "guber_wire_pool: a global's key is longer than max_key_bytes (nothing was installed)");
    }
    const uint32_t ne = (uint32_t)p->eng.size();
    std::vector<std::vector<guber_item_t>> per(ne);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t e = 0;
        if (ne > 1) {
            if (p->hrule.global_engine >= 0) e = (uint32_t)p->hrule.global_engine;
            else if (p->hrule.n_shards > 1) e = wpl_route_host(p->hrule, guber_xxhash64(items[i].key, items[i].key_len, 0));
            if (e >= ne) e = 0;
        }
        per[e].push_back(items[i]);                                    // (the message's order is kept per engine: LRUCache.Add is applied item by item)
    }
    for (uint32_t e = 0; e < ne; ++e) {
        if (per[e].empty()) continue;
        rc = guber_add_items(p->eng[e], per[e].data(), (uint32_t)per[e].size(), nullptr);
        if (rc != GUBER_OK) return rc;                                 // (the device's own failure; what earlier engines took stays)
        if (installed) *installed += (uint32_t)per[e].size();
    }
    return GUBER_OK;
}
