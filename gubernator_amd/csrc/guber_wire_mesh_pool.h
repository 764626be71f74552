// guber_wire_mesh_pool.h — guber_wire_mesh_pool_*: the payload stage over a MESH.  Caller threads (the gRPC handlers of a daemon on a node with
// several GPUs) hand the SERIALIZED GetRateLimitsReq of their RPC to ANY rank of a guber_mesh_t and get the serialized GetRateLimitsResp back,
// with metadata{"owner": <address>} on every answer another rank owns.  Decode (k_wire_*), the ring's owner decision (gubernator.go:236-283:
// k_mx_count<true> / k_mx_scan / k_mx_pack<true>), the evaluation on the owners' fronts, the answers' order (k_mx_apack / k_mx_out) and the
// marshalling (k_wire_enc_owner) all stay on the devices; this file adds no kernel — it is the host protocol that lets many threads share them.
//
// Part of guber_engine.hip's translation unit, behind guber_wire_dev.h (wire_mesh_pool_*: the split of guber_wire_dev_eval_mesh_enc) and
// guber_wire_pool.h, whose helpers it shares (wpl_item_bound, wpl_mono_us).  It compiles on its own against stand-ins for those calls
// (tests/hostsim/mesh_pool_tsan.cpp), which is why it reaches into no struct of the mesh, the fronts or the engines.
//
//   stage set        one stage per rank: a decoder bound to the first engine of the rank's front, its pinned staging buffer, the RPCs' offsets
//                    and lengths.  `sets` of them in rotation: one fills while another is on the GPUs.
//   callers          under the pool's mutex: a place in rank r's stage of the open set (RPC index, item bound, payload bytes at a 16-byte
//                    aligned offset); outside it: the payload copied in, the wait for the set, the RPC's bytes copied out — or, for an RPC
//                    with an item error (WIRE_ENC_RAW), marshalled by the caller from its own req bytes through the host transcoder.
//   a set leaves     when a rank's stage cannot take the RPC that asks (sealed_full), batch_wait_us after its first payload (sealed_wait), or
//                    at once while no set is on the GPUs (sealed_idle: a lightly loaded pool does not wait).  The clock is read once, when the
//                    set is sealed: every rank's decode gets that now_ms.  The next set opens before the sealed one is enqueued.
//   dispatcher       ONE thread, sets strictly in the order they were sealed: waits for the set's copies, enqueues every non-empty rank's
//                    decode before it collects any, runs the mesh evaluation with serialized responses (wire_mesh_pool_eval), announces the
//                    set.  It may block on the GPU, and it does nothing per item or per RPC: one client's bad items hold up nobody's set.
//   host protocol    ONE mutex and condition variables (callers waiting for a set to open, the dispatcher, one per set for its callers), not
//                    guber_wire_pool's reservation word: a place here is three counters of one of W stages plus the set's own, which one
//                    compare-and-swap does not cover, and the mesh call behind it is host-bound at ~1 ms (profiles/mesh_first_numbers.txt) —
//                    a mutex held for a few dozen instructions per RPC is not what limits it.  Correctness first.
//   direct path      opt-in (guber_wire_mesh_pool_set_direct): a lone small RPC that arrives while few calls are inside joins no set — its caller
//                    evaluates it through the mesh's one-launch call.  guber_wire_mesh_pool_direct.h, reached through `direct` alone.
#pragma once
#include <condition_variable>
#include <deque>

#include "guber_wire_pool.h"          // wpl_item_bound (guber_wire_parse.h), wpl_mono_us

struct guber_wire_mesh_pool {
    enum State : int { FREE = 0, OPEN, SEALED, ANSWERED };
    static constexpr uint32_t NONE = 0xffffffffu;
    struct Stage {                                                       // one rank's part of a set
        guber_wire_dev* dec = nullptr; uint8_t* buf = nullptr;
        std::vector<uint32_t> offs, lens, first, count; std::vector<int32_t> status;   // per RPC: where its payload lies; the decode's verdicts
        uint32_t n_rpc = 0, items = 0, b16 = 0;                           // places taken: RPCs, items (upper bound), payload bytes / 16
    };
    struct Set {
        std::vector<Stage> st; std::vector<WireMeshEncDone> done;         // [W]
        int state = FREE; uint32_t rpcs = 0, copying = 0, readers = 0; int rc = 0;
        int64_t now_ms = 0, t_first_us = 0, t_seal_us = 0;
        uint64_t seq = 0, answered_seq = 0;                               // the opening the set is in; the last one that was announced
        std::condition_variable cv_done;
    };
    guber_mesh_t* mesh = nullptr;
    uint32_t W = 0, n_sets = 0, max_items = 0, max_b16 = 0, max_rpcs = 0, wait_us = 0, max_per_rpc = 0, item_cap = 0; int wrap_errors = 0;
    std::vector<std::string> addr; std::vector<const char*> addr_ptr; WireMeshSfx sfx;
    std::unique_ptr<Set[]> sets;
    std::mutex mu;
    std::condition_variable cv_open, cv_disp;
    std::deque<uint32_t> queue;                                          // sealed sets, oldest first
    uint32_t open = NONE, inflight = 0; uint64_t seq_counter = 0;         // inflight: sealed and not yet announced ("on the GPUs")
    bool stop = false, closed = false, failed = false;                  // closed: no caller is let in any more; failed: a set failed on the devices
    std::atomic<int64_t> clock_ms{0};
    std::thread dispatcher;
    // the direct path (guber_wire_mesh_pool_direct.h, included behind this file; guber_wire_mesh_pool_set_direct fills `direct`): a lone small RPC
    // evaluated by its caller.  direct_items: the largest item bound that takes it (0 = off, the default); direct_calls: the most calls
    // that may be inside the pool for an RPC to take it; inside: calls past the door, on either path
    typedef int (*DirectFn)(guber_wire_mesh_pool*, uint32_t rank, const uint8_t* req, size_t len, guber_wire_batch_t* wb, uint8_t* resp, size_t cap, size_t* resp_len);
    std::atomic<DirectFn> direct{nullptr};
    std::atomic<uint32_t> direct_items{0}, direct_calls{8}, inside{0};
    std::atomic<uint64_t> st_direct{0}, st_direct_fallback{0};
    std::atomic<uint64_t> st_rpcs{0}, st_items{0}, st_sets{0}, st_full{0}, st_wait{0}, st_idle{0}, st_forwarded{0}, st_host_rpcs{0}, st_open_waits{0}, st_fill_us{0}, st_gpu_us{0};
};

namespace {
enum { MPL_FULL = 1, MPL_WAIT = 2, MPL_IDLE = 3 };
// (all three under the pool's mutex)
void mpl_open_next(guber_wire_mesh_pool* p) {
    for (uint32_t k = 0; k < p->n_sets; ++k) {
        guber_wire_mesh_pool::Set& s = p->sets[k];
        if (s.state != guber_wire_mesh_pool::FREE) continue;
        s.state = guber_wire_mesh_pool::OPEN; s.seq = ++p->seq_counter;
        s.rpcs = s.copying = s.readers = 0; s.rc = 0; s.t_first_us = 0;
        for (auto& g : s.st) g.n_rpc = g.items = g.b16 = 0;
        p->open = k;
        p->cv_open.notify_all();
        return;
    }
}
void mpl_seal(guber_wire_mesh_pool* p, uint32_t k, int why) {
    guber_wire_mesh_pool::Set& s = p->sets[k];
    const int64_t c = p->clock_ms.load(std::memory_order_relaxed);
    s.now_ms = c ? c : std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::system_clock::now().time_since_epoch()).count();
    s.t_seal_us = wpl_mono_us();
    s.state = guber_wire_mesh_pool::SEALED;
    (why == MPL_FULL ? p->st_full : why == MPL_WAIT ? p->st_wait : p->st_idle).fetch_add(1, std::memory_order_relaxed);
    if (s.t_first_us) p->st_fill_us.fetch_add((uint64_t)(s.t_seal_us - s.t_first_us), std::memory_order_relaxed);
    p->open = guber_wire_mesh_pool::NONE;
    mpl_open_next(p);                                                    // (the next set opens before this one is enqueued)
    p->queue.push_back(k); ++p->inflight;
    p->cv_disp.notify_one();
}
// a set's way through the GPUs (no lock held: the set is the dispatcher's alone until it is announced)
int mpl_run_set(guber_wire_mesh_pool* p, guber_wire_mesh_pool::Set& s) {
    const uint32_t W = p->W;
    std::vector<guber_wire_dev_t*> decs(W, nullptr);
    int rc = GUBER_OK;
    for (uint32_t r = 0; r < W && !rc; ++r) {                            // every decode is enqueued before any is collected
        guber_wire_mesh_pool::Stage& g = s.st[r];
        if (!g.n_rpc) continue;
        rc = guber_wire_dev_decode_staged_async(g.dec, g.offs.data(), g.lens.data(), g.n_rpc, nullptr, p->max_per_rpc, s.now_ms);
        if (!rc) decs[r] = g.dec;
    }
    for (uint32_t r = 0; r < W; ++r) {
        if (!decs[r]) continue;
        guber_wire_mesh_pool::Stage& g = s.st[r];
        uint32_t n = 0; int rc2;
        while ((rc2 = guber_wire_dev_decode_collect(g.dec, 1, g.status.data(), g.first.data(), g.count.data(), &n)) == GUBER_PENDING) wpl_relax();
        if (rc2 && !rc) rc = rc2;
    }
    if (rc) return rc;
    uint64_t forwarded = 0;
    rc = wire_mesh_pool_eval(decs.data(), p->mesh, p->sfx, s.done.data(), &forwarded);
    p->st_forwarded.fetch_add(forwarded, std::memory_order_relaxed);
    return rc;
}
void mpl_dispatch(guber_wire_mesh_pool* p) {
    using MP = guber_wire_mesh_pool;
    std::unique_lock<std::mutex> lk(p->mu);
    for (;;) {
        // the open set: BatchWait after its first payload (or the pool is going away) — sealed here; full and idle are the callers' to see
        if (p->open != MP::NONE) {
            MP::Set& o = p->sets[p->open];
            if (o.rpcs && (p->stop || wpl_mono_us() - o.t_first_us >= (int64_t)p->wait_us)) mpl_seal(p, p->open, MPL_WAIT);
        }
        if (!p->queue.empty() && p->sets[p->queue.front()].copying == 0) {
            const uint32_t k = p->queue.front();
            p->queue.pop_front();
            MP::Set& s = p->sets[k];
            int rc;
            if (p->failed) rc = GUBER_E_WIRE_CLOSED;                     // (a set before this one failed on the devices: nothing more is enqueued)
            else { lk.unlock(); rc = mpl_run_set(p, s); lk.lock(); }
            s.rc = rc;
            if (rc) p->closed = p->failed = true;
            p->st_sets.fetch_add(1, std::memory_order_relaxed);
            p->st_gpu_us.fetch_add((uint64_t)(wpl_mono_us() - s.t_seal_us), std::memory_order_relaxed);
            s.readers = s.rpcs; s.state = MP::ANSWERED; s.answered_seq = s.seq;
            s.cv_done.notify_all();
            --p->inflight;
            if (p->closed) p->cv_open.notify_all();
            if (!p->inflight && p->open != MP::NONE && p->sets[p->open].rpcs) mpl_seal(p, p->open, MPL_IDLE);
            continue;
        }
        if (p->stop && p->queue.empty() && (p->open == MP::NONE || p->sets[p->open].rpcs == 0)) return;
        if (p->open != MP::NONE && p->sets[p->open].rpcs) {
            const int64_t left = p->sets[p->open].t_first_us + (int64_t)p->wait_us - wpl_mono_us();
            // (wait_until on the system clock is pthread_cond_timedwait, which ThreadSanitizer follows; wait_for is pthread_cond_clockwait, which
            //  GCC 11's does not.  A clock step only moves this wake-up: the loop decides by the monotonic clock, and every arrival and every
            //  announcement wakes it anyway)
            p->cv_disp.wait_until(lk, std::chrono::system_clock::now() + std::chrono::microseconds(std::max<int64_t>(left, 1)));
        } else p->cv_disp.wait(lk);
    }
}
// the host transcoder's batch of a caller thread, for an RPC the device leaves raw: made (or grown) at the door, before the RPC joins a set
struct MplThreadBatch {
    guber_wire_batch_t* wb = nullptr; uint32_t items = 0; size_t bytes = 0;
    int ensure(uint32_t n, size_t b) {
        if (wb && n <= items && b <= bytes) return GUBER_OK;
        if (wb) guber_wire_batch_destroy(wb);
        wb = nullptr; items = std::max(n, 64u); bytes = std::max<size_t>(b, 4096);
        const int rc = guber_wire_batch_create(items, (uint32_t)std::min<size_t>(bytes, 0xffffffffu), 0, &wb);
        if (rc) { wb = nullptr; items = 0; bytes = 0; }
        return rc;
    }
    ~MplThreadBatch() { if (wb) guber_wire_batch_destroy(wb); }
};
}  // namespace

extern "C" void guber_wire_mesh_pool_destroy(guber_wire_mesh_pool_t* p) {
    if (!p) return;
    if (p->dispatcher.joinable()) {
        { std::lock_guard<std::mutex> lk(p->mu); p->stop = true; p->closed = true; }
        p->cv_disp.notify_all(); p->cv_open.notify_all();
        p->dispatcher.join();
    }
    if (p->sets) for (uint32_t k = 0; k < p->n_sets; ++k) for (auto& g : p->sets[k].st) if (g.dec) guber_wire_dev_destroy(g.dec);
    delete p;
}

extern "C" int guber_wire_mesh_pool_create(guber_mesh_t* m, const char* const* owner_addr, const guber_wire_mesh_pool_config_t* cfg, guber_wire_mesh_pool_t** out) {
    if (!m || !owner_addr || !out) return fail(GUBER_E_INVALID_ARG, "null argument");
    *out = nullptr;
    guber_wire_mesh_pool_config_t c{};
    if (cfg) c = *cfg;
    uint32_t W = 0, max_n = 0;
    wire_mesh_pool_shape(m, &W, &max_n);
    std::unique_ptr<guber_wire_mesh_pool, void (*)(guber_wire_mesh_pool*)> p(new guber_wire_mesh_pool(), [](guber_wire_mesh_pool* q) { guber_wire_mesh_pool_destroy(q); });
    if (wire_mesh_sfx_build(owner_addr, W, p->sfx)) return fail(GUBER_E_INVALID_ARG, "guber_wire_mesh_pool: every rank has an address of 1 .. GUBER_WIRE_OWNER_ADDR_MAX bytes");
    std::vector<guber_engine_t*> eng(W, nullptr);
    uint32_t least = 0xffffffffu;
    for (uint32_t r = 0; r < W; ++r) { uint32_t mb = 0; eng[r] = wire_mesh_pool_engine(m, r, &mb); least = std::min(least, mb); }
    if (!c.sets) c.sets = 3;
    if (!c.max_items) c.max_items = std::min(std::min(49152u, max_n), least);
    if (!c.max_payload_bytes) c.max_payload_bytes = 8u << 20;
    if (!c.max_rpcs) c.max_rpcs = 1024;
    if (!c.batch_wait_us) c.batch_wait_us = 500;                       // config.go:131 BatchWait
    if (!c.max_per_rpc) c.max_per_rpc = 1000;                          // gubernator.go:40
    if (c.sets < 2 || c.sets > 8 || c.max_rpcs > WPL_MAX_RPCS || c.max_payload_bytes > (16u << 20) || c.max_payload_bytes < 64)
        return fail(GUBER_E_INVALID_ARG, "guber_wire_mesh_pool: 2 .. 8 sets of at most 4 095 RPCs and 16 MiB of payload bytes per rank");
    if (c.max_items > max_n || c.max_items > least)
        return fail(GUBER_E_INVALID_ARG, "guber_wire_mesh_pool: max_items above the mesh's max_n or a rank's decoder engine's max_batch");
    p->mesh = m; p->W = W; p->n_sets = c.sets; p->max_items = c.max_items; p->max_b16 = c.max_payload_bytes / 16; p->max_rpcs = c.max_rpcs;
    p->wait_us = c.batch_wait_us; p->max_per_rpc = c.max_per_rpc == 0xffffffffu ? 0 : c.max_per_rpc; p->wrap_errors = c.wrap_errors ? 1 : 0;
    p->item_cap = std::min<uint32_t>(std::min<uint32_t>(c.max_items, 4096u), p->max_per_rpc ? p->max_per_rpc : 4096u);
    for (uint32_t r = 0; r < W; ++r) p->addr.emplace_back(owner_addr[r]);
    for (uint32_t r = 0; r < W; ++r) p->addr_ptr.push_back(p->addr[r].c_str());
    p->sets.reset(new guber_wire_mesh_pool::Set[c.sets]);
    for (uint32_t k = 0; k < c.sets; ++k) {
        guber_wire_mesh_pool::Set& s = p->sets[k];
        s.st.resize(W); s.done.resize(W);
        for (uint32_t r = 0; r < W; ++r) {
            guber_wire_mesh_pool::Stage& g = s.st[r];
            int rc = guber_wire_dev_create(eng[r], c.max_items, c.max_payload_bytes, c.max_rpcs, &g.dec);
            if (rc) return rc;
            size_t cap = 0;
            rc = guber_wire_dev_buffer(g.dec, &g.buf, &cap);
            if (rc) return rc;
            rc = wire_mesh_pool_prepare(g.dec, p->sfx);                  // (the suffix table depends on the addresses alone: uploaded once)
            if (rc) return rc;
            g.offs.resize(c.max_rpcs); g.lens.resize(c.max_rpcs); g.first.resize(c.max_rpcs); g.count.resize(c.max_rpcs); g.status.resize(c.max_rpcs);
        }
    }
    mpl_open_next(p.get());
    p->dispatcher = std::thread(mpl_dispatch, p.get());
    *out = p.release();
    return GUBER_OK;
}

extern "C" int guber_wire_mesh_pool_set_clock(guber_wire_mesh_pool_t* p, int64_t now_ms) {
    if (!p) return fail(GUBER_E_INVALID_ARG, "null argument");
    p->clock_ms.store(now_ms, std::memory_order_relaxed);
    return GUBER_OK;
}

extern "C" int guber_wire_mesh_pool_stats(guber_wire_mesh_pool_t* p, guber_wire_mesh_pool_stats_t* o) {
    if (!p || !o) return fail(GUBER_E_INVALID_ARG, "null argument");
    o->rpcs = p->st_rpcs.load(); o->items = p->st_items.load(); o->sets = p->st_sets.load();
    o->sealed_full = p->st_full.load(); o->sealed_wait = p->st_wait.load(); o->sealed_idle = p->st_idle.load();
    o->forwarded = p->st_forwarded.load(); o->host_rpcs = p->st_host_rpcs.load(); o->open_waits = p->st_open_waits.load();
    o->fill_us_sum = p->st_fill_us.load(); o->gpu_us_sum = p->st_gpu_us.load();
    return GUBER_OK;
}

// everything guber_wire_dev_mesh_enc_bound counts, for one RPC: per item an answer with an error text and the longest owner suffix, plus the
// keys the texts may quote (no more than the payload's bytes)
extern "C" size_t guber_wire_mesh_pool_response_bound(const guber_wire_mesh_pool_t* p, const uint8_t* req, size_t len) {
    if (!p || (!req && len)) return 0;
    const size_t items = len ? wpl_item_bound(req, len, p->max_per_rpc ? p->max_per_rpc : 4096u) : 0;
    return items * (guber::wire::RESP_ERR_ITEM_BOUND + 1 + p->sfx.longest) + len;
}

// V1Instance.GetRateLimits on the serialized message that arrived at `rank` (gubernator.go:183-306)
extern "C" int guber_wire_mesh_pool_get_rate_limits(guber_wire_mesh_pool_t* p, uint32_t rank, const uint8_t* req, size_t len, uint8_t* resp, size_t cap, size_t* resp_len) {
    using MP = guber_wire_mesh_pool;
    if (!p || (!req && len) || !resp_len || (!resp && cap)) return fail(GUBER_E_INVALID_ARG, "null argument");
    *resp_len = 0;
    if (rank >= p->W) return fail(GUBER_E_INVALID_ARG, "guber_wire_mesh_pool: no such rank");
    if (len == 0) return GUBER_OK;                                     // no requests: an empty response, no set
    if (len > (size_t)p->max_b16 * 16) return fail(GUBER_E_WIRE_FULL, "payload larger than a stage");
    const size_t need = guber_wire_mesh_pool_response_bound(p, req, len);
    if (cap < need) { *resp_len = need; return fail(GUBER_E_NOMEM, "response buffer below guber_wire_mesh_pool_response_bound()"); }
    const uint32_t units = (uint32_t)((len + 15) / 16);
    const uint32_t bound = std::max(1u, wpl_item_bound(req, len, p->item_cap));
    thread_local MplThreadBatch tl;
    if (tl.ensure(bound, len + bound + 16)) return fail(GUBER_E_NOMEM, "guber_wire_mesh_pool: no memory for the host transcoder's batch");
    struct Inside { MP* p; uint32_t n; explicit Inside(MP* q) : p(q), n(q->inside.fetch_add(1, std::memory_order_acq_rel) + 1) {} ~Inside() { p->inside.fetch_sub(1, std::memory_order_acq_rel); } } in(p);
    // ---- a lone small RPC while few calls are inside: its caller evaluates it (off unless guber_wire_mesh_pool_set_direct switched it on)
    if (const uint32_t di = p->direct_items.load(std::memory_order_acquire)) {
        const MP::DirectFn fn = p->direct.load(std::memory_order_acquire);
        if (fn && bound <= di && in.n <= p->direct_calls.load(std::memory_order_relaxed)) return fn(p, rank, req, len, tl.wb, resp, cap, resp_len);
    }
    // ---- a place in rank's stage of the open set
    MP::Set* sp = nullptr;
    uint32_t idx = 0; size_t off = 0; uint64_t seq = 0;
    {
        std::unique_lock<std::mutex> lk(p->mu);
        bool waited = false;
        for (;;) {
            if (p->closed) return fail(GUBER_E_WIRE_CLOSED, "guber_wire_mesh_pool: closed");
            if (p->open == MP::NONE) mpl_open_next(p);
            if (p->open == MP::NONE) {                                   // every set is on its way through the GPUs or being read
                if (!waited) { waited = true; p->st_open_waits.fetch_add(1, std::memory_order_relaxed); }
                p->cv_open.wait(lk);
                continue;
            }
            const uint32_t k = p->open;
            MP::Set& s = p->sets[k];
            MP::Stage& g = s.st[rank];
            if (g.n_rpc + 1 > p->max_rpcs || g.items + bound > p->max_items || g.b16 + units > p->max_b16) {
                if (g.n_rpc == 0) return fail(GUBER_E_WIRE_FULL, "payload larger than a stage");
                mpl_seal(p, k, MPL_FULL);
                continue;
            }
            idx = g.n_rpc++; off = (size_t)g.b16 * 16; g.items += bound; g.b16 += units;
            g.offs[idx] = (uint32_t)off; g.lens[idx] = (uint32_t)len;
            if (!s.rpcs++) s.t_first_us = wpl_mono_us();
            ++s.copying;
            sp = &s; seq = s.seq;
            if (!p->inflight) mpl_seal(p, k, MPL_IDLE);                  // no set is on the GPUs: this one leaves at once
            else if (s.rpcs == 1) p->cv_disp.notify_one();               // (the dispatcher's BatchWait starts)
            break;
        }
    }
    MP::Set& s = *sp;
    memcpy(s.st[rank].buf + off, req, len);
    {
        std::unique_lock<std::mutex> lk(p->mu);
        if (--s.copying == 0 && s.state == MP::SEALED) p->cv_disp.notify_one();
        // ---- the set's way through the GPUs
        s.cv_done.wait(lk, [&] { return s.answered_seq == seq; });
    }
    // ---- my RPC's bytes
    int rc = s.rc;
    size_t used = 0;
    if (!rc) {
        const MP::Stage& g = s.st[rank];
        const int32_t st = g.status[idx];
        if (st != GUBER_OK) rc = fail(st, "guber_wire_mesh_pool: the message is turned away whole");   // GUBER_E_WIRE_MALFORMED / GUBER_E_WIRE_TOO_LARGE
        else if (const uint32_t count = g.count[idx]) {
            const uint32_t first = g.first[idx];
            const WireMeshEncDone& x = s.done[rank];
            const uint32_t el = x.enc_len[idx];
            if (el != guber::WIRE_ENC_RAW) {                             // k_wire_enc_owner has written it: one memcpy (cap >= the bound >= el)
                if (el > cap) rc = fail(GUBER_E_HIP, "guber_wire_mesh_pool: the device's responses exceed the bound");
                else { memcpy(resp, x.enc + guber::wire_enco_off(first, idx, x.item_max), el); used = el; }
            } else {                                                     // an item error: the texts need the keys — from my own req bytes
                rc = wire_mesh_enc_host_rpc(tl.wb, req, len, s.now_ms, first, count, x.raw, x.h_owner, rank, p->addr_ptr.data(), p->W, p->wrap_errors, resp, cap, &used);
                p->st_host_rpcs.fetch_add(1, std::memory_order_relaxed);
            }
            p->st_items.fetch_add(count, std::memory_order_relaxed);
        }
    } else fail(rc, rc == GUBER_E_WIRE_CLOSED ? "guber_wire_mesh_pool: closed" : "guber_wire_mesh_pool: the set failed on the devices");
    p->st_rpcs.fetch_add(1, std::memory_order_relaxed);
    {
        std::lock_guard<std::mutex> lk(p->mu);                           // (the set is not touched after this)
        if (--s.readers == 0) {
            s.state = MP::FREE;
            if (p->open == MP::NONE && !p->closed) mpl_open_next(p);
        }
    }
    *resp_len = used;
    return rc;
}
