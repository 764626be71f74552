// guber_wire_mesh_pool_direct.h — the payload stage over a mesh: lone small RPCs evaluated by their caller (guber_wire_mesh_pool_set_direct).
// Included behind guber_wire_mesh_pool.h, which reaches it through guber_wire_mesh_pool::direct alone — that file goes on compiling against
// stand-ins that know nothing of the mesh's one-launch call (tests/hostsim/mesh_pool_tsan.cpp); this one needs one more of them,
// wire_mesh_pool_eval_small (guber_wire_dev.h; tests/hostsim/mesh_pool_direct_tsan.cpp has its own).
//
// A stage set costs a lone one-item RPC a decode, the mesh's general call, an encoder and the dispatcher's waits
// (profiles/mesh_pool_first_numbers.txt: 218 us).  With the path on, an RPC whose item bound (wpl_item_bound) is at most max_items, arriving
// while at most max_calls calls are inside the pool and the pool is open, is served by its caller instead:
//   the host transcoder decodes it into the thread's batch (the one the pool keeps for RPCs with item errors) at the pool's clock;
//   guber_mesh_eval_small evaluates it, with only gens[rank] non-empty — the ring's and the fronts' decisions are the devices', as in a set;
//   wire_mesh_enc_host_rpc writes the response: the bytes of guber_wire_encode_responses_owner, error texts and metadata{"owner"} included.
// Everything a set checks at the door has been checked before this is reached (guber_wire_mesh_pool_get_rate_limits); a malformed or too
// large message gets the codes a set gives it, from the host transcoder, and nothing is evaluated.  The call is synchronous under the mesh's
// mutex, so "a call that has returned was evaluated before any call that starts later" holds across both paths.
#pragma once

namespace {
int mpl_direct(guber_wire_mesh_pool* p, uint32_t rank, const uint8_t* req, size_t len, guber_wire_batch_t* wb, uint8_t* resp, size_t cap, size_t* resp_len) {
    { std::lock_guard<std::mutex> lk(p->mu); if (p->closed) return fail(GUBER_E_WIRE_CLOSED, "guber_wire_mesh_pool: closed"); }
    const int64_t c = p->clock_ms.load(std::memory_order_relaxed);
    const int64_t now_ms = c ? c : std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::system_clock::now().time_since_epoch()).count();
    guber_wire_batch_reset(wb, now_ms);
    uint32_t first = 0, count = 0;
    int rc = guber_wire_decode_requests(wb, req, len, p->max_per_rpc, 1, &first, &count);
    if (rc) { p->st_rpcs.fetch_add(1, std::memory_order_relaxed); return fail(rc, "guber_wire_mesh_pool: the message is turned away whole"); }   // GUBER_E_WIRE_MALFORMED / GUBER_E_WIRE_TOO_LARGE
    size_t used = 0;
    if (count) {
        if (count > 256u) return fail(GUBER_E_HIP, "guber_wire_mesh_pool: an RPC above its item bound");
        // the answers and the owners outside the batch: wire_mesh_enc_host_rpc decodes into it once more
        thread_local struct { uint8_t status[256], err[256], owner[256]; int64_t limit[256], remaining[256], reset_time[256]; } a;
        std::vector<guber_batch_t> gens(p->W); std::vector<guber_result_t> res(p->W); std::vector<uint8_t*> own(p->W, nullptr);
        for (uint32_t r = 0; r < p->W; ++r) { gens[r] = guber_batch_t{}; gens[r].now_ms = now_ms; res[r] = guber_result_t{}; }
        gens[rank] = *guber_wire_batch_view(wb);
        gens[rank].n = count; gens[rank].is_owner = nullptr; gens[rank].greg_expire = nullptr; gens[rank].greg_duration = nullptr;   // (the ring decides; the calendar is the device's, as in a set)
        gens[rank].now_ms = now_ms;
        res[rank].status = a.status; res[rank].err = a.err; res[rank].limit = a.limit; res[rank].remaining = a.remaining; res[rank].reset_time = a.reset_time;
        own[rank] = a.owner;
        uint64_t forwarded = 0, fallbacks = 0;
        rc = wire_mesh_pool_eval_small(p->mesh, gens.data(), res.data(), own.data(), &forwarded, &fallbacks);
        if (rc) return rc;
        p->st_forwarded.fetch_add(forwarded, std::memory_order_relaxed);
        if (fallbacks) p->st_direct_fallback.fetch_add(1, std::memory_order_relaxed);
        rc = wire_mesh_enc_host_rpc(wb, req, len, now_ms, 0, count, res[rank], a.owner, rank, p->addr_ptr.data(), p->W, p->wrap_errors, resp, cap, &used);
        if (rc) return rc;
        p->st_items.fetch_add(count, std::memory_order_relaxed);
    }
    p->st_rpcs.fetch_add(1, std::memory_order_relaxed);
    p->st_direct.fetch_add(1, std::memory_order_relaxed);
    *resp_len = used;
    return GUBER_OK;
}
}  // namespace

extern "C" int guber_wire_mesh_pool_set_direct(guber_wire_mesh_pool_t* p, uint32_t max_items, uint32_t max_calls) {
    if (!p) return fail(GUBER_E_INVALID_ARG, "null argument");
    if (max_items > 256u) return fail(GUBER_E_INVALID_ARG, "guber_wire_mesh_pool: the direct path takes RPCs of at most 256 items");
    p->direct_calls.store(max_calls ? max_calls : 8u, std::memory_order_relaxed);
    p->direct.store(mpl_direct, std::memory_order_release);
    p->direct_items.store(max_items, std::memory_order_release);
    return GUBER_OK;
}

extern "C" int guber_wire_mesh_pool_direct_stats(guber_wire_mesh_pool_t* p, guber_wire_mesh_pool_direct_stats_t* o) {
    if (!p || !o) return fail(GUBER_E_INVALID_ARG, "null argument");
    o->direct_rpcs = p->st_direct.load(); o->fallback_rpcs = p->st_direct_fallback.load();
    return GUBER_OK;
}
