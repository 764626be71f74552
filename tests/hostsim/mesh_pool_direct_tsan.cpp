// mesh_pool_direct_tsan.cpp — TEST INFRASTRUCTURE: the HOST protocol of the payload stage over a mesh WITH lone small RPCs evaluated by their
// callers (gubernator_amd/csrc/guber_wire_mesh_pool.h + guber_wire_mesh_pool_direct.h: the gate on the calls inside the pool, direct callers
// beside callers that take places in sets, guber_wire_mesh_pool_set_direct toggled meanwhile) under ThreadSanitizer.  The stand-ins for the
// device decoder are wire_pool_tsan.cpp's (that file is included whole, its main() under another name); those for the mesh are this file's own,
// as mesh_pool_tsan.cpp has them — ONE oracle behind its mutex, every key its arrival rank's — plus one for the mesh's one-launch call.  A stand-alone program
// with its own main(); never part of the product library.
//   make -C tests/hostsim -f mesh_pool_direct.mk mesh_pool_direct_tsan && /tmp/guber_mesh_pool_direct_tsan [callers] [rpcs per caller]
#define main wire_pool_tsan_main
#include "wire_pool_tsan.cpp"
#undef main

#include <unordered_map>

// ---- what guber_wire_mesh_pool.h expects from guber_wire_dev.h ---------------------------------------------------------------------------
struct guber_mesh { uint32_t W = 0, max_n = 0; std::vector<guber_engine> eng; std::atomic<int> inside{0}; int64_t last_now = 0; };
struct WireMeshSfx { size_t longest = 0; uint32_t item_max = 0; };
struct WireMeshEncDone { const uint8_t* enc = nullptr; const uint32_t* enc_len = nullptr; guber_result_t raw{}; const uint8_t* h_owner = nullptr; uint32_t item_max = 0; };
namespace guber { static size_t wire_enco_off(uint32_t first, uint32_t r, uint32_t item_max) { return ((size_t)first * item_max + (size_t)r * 32u) & ~(size_t)15; } }
struct MeshSide { std::vector<uint8_t> enc, owner; std::vector<uint32_t> enc_len; };
static std::unordered_map<guber_wire_dev*, MeshSide> g_side;            // (filled while the pool is created, read afterwards)
static int wire_mesh_sfx_build(const char* const* owner_addr, uint32_t W, WireMeshSfx& T) {
    T.longest = guber::wire::owner_suffix_longest(owner_addr, W, 16);
    if (!T.longest) return GUBER_E_INVALID_ARG;
    T.item_max = guber::WIRE_ENC_ITEM_MAX + (uint32_t)T.longest;
    return GUBER_OK;
}
static void wire_mesh_pool_shape(guber_mesh_t* m, uint32_t* W, uint32_t* max_n) { *W = m->W; *max_n = m->max_n; }
static guber_engine_t* wire_mesh_pool_engine(guber_mesh_t* m, uint32_t r, uint32_t* max_batch) { *max_batch = 1u << 20; return &m->eng[r]; }
static int wire_mesh_pool_prepare(guber_wire_dev* d, const WireMeshSfx& T) {
    MeshSide& s = g_side[d];
    s.enc.resize((size_t)d->max_items * T.item_max + (size_t)d->max_rpcs * 32 + 64); s.owner.resize(d->max_items); s.enc_len.resize(d->max_rpcs);
    return GUBER_OK;
}
static int wire_mesh_pool_eval(guber_wire_dev_t* const* decs, guber_mesh_t* m, const WireMeshSfx& T, WireMeshEncDone* done, uint64_t* forwarded) {
    *forwarded = 0;
    if (m->inside.fetch_add(1) != 0) { m->inside.fetch_sub(1); return fail(GUBER_E_INVALID_ARG, "stand-in mesh: two sets inside at once"); }
    int rc = GUBER_OK;
    int64_t now = 0;
    for (uint32_t r = 0; r < m->W && !rc; ++r) {
        guber_wire_dev* d = decs[r];
        done[r] = WireMeshEncDone{};
        if (!d) continue;
        if (d->dec_pending) { rc = fail(GUBER_E_INVALID_ARG, "stand-in mesh: a decode that was not collected"); break; }
        if (!d->n_items) continue;
        const int64_t t = guber_wire_batch_view(d->wb)->now_ms;
        if (now && t != now) { rc = fail(GUBER_E_INVALID_ARG, "stand-in mesh: the decodes of a set carry one now_ms"); break; }
        now = t;
        MeshSide& s = g_side.at(d);
        {
            std::lock_guard<std::mutex> lk(g_oracle_mu);
            oracle_eval_batch(g_oracle, guber_wire_batch_view(d->wb), guber_wire_batch_result(d->wb));
        }
        const guber_result_t* res = guber_wire_batch_result(d->wb);
        memset(s.owner.data(), (int)r, d->n_items);                      // (every key is its arrival rank's: no metadata, the parser stays wire_pool_tsan's)
        for (uint32_t q = 0; q < d->nrpc; ++q) {
            const uint32_t first = d->first[q], count = d->status[q] ? 0 : d->count[q];
            bool bad = false;
            const uint8_t* pre = guber_wire_batch_pre_errors(d->wb);         // (an item the transcoder rejected: never shown to a bucket, an error all the same)
            for (uint32_t i = 0; i < count; ++i) bad = bad || res->err[first + i] != 0 || pre[first + i] != 0;
            size_t used = 0;
            if (bad) s.enc_len[q] = guber::WIRE_ENC_RAW;
            else if (!count) s.enc_len[q] = 0;
            else if (guber_wire_encode_responses(d->wb, first, count, 1, s.enc.data() + guber::wire_enco_off(first, q, T.item_max), (size_t)count * T.item_max, &used)) { rc = GUBER_E_HIP; break; }
            else s.enc_len[q] = (uint32_t)used;
        }
        done[r].enc = s.enc.data(); done[r].enc_len = s.enc_len.data(); done[r].raw = *res; done[r].h_owner = s.owner.data(); done[r].item_max = T.item_max;
    }
    if (!rc && now) {
        if (now < m->last_now) rc = fail(GUBER_E_INVALID_ARG, "stand-in mesh: a set evaluated before one that was sealed earlier");
        m->last_now = now;
    }
    m->inside.fetch_sub(1);
    return rc;
}
static int wire_mesh_enc_host_rpc(guber_wire_batch_t* wb, const uint8_t* req, size_t len, int64_t now_ms, uint32_t first, uint32_t count, const guber_result_t& raw,
                                  const uint8_t* owner, uint32_t self, const char* const* owner_addr, uint32_t n_ranks, int wrap_errors, uint8_t* out, size_t cap, size_t* used) {
    guber_wire_batch_reset(wb, now_ms);
    uint32_t f0 = 0, c0 = 0;
    int rc = guber_wire_decode_requests(wb, req, len, 0, 1, &f0, &c0);
    if (rc || c0 != count) return fail(GUBER_E_HIP, "stand-in: the decoders disagree about a payload");
    guber_result_t* hr = guber_wire_batch_result(wb);
    memcpy(hr->status, raw.status + first, count); memcpy(hr->err, raw.err + first, count);
    memcpy(hr->limit, raw.limit + first, (size_t)count * 8); memcpy(hr->remaining, raw.remaining + first, (size_t)count * 8);
    memcpy(hr->reset_time, raw.reset_time + first, (size_t)count * 8);
    return guber_wire_encode_responses_owner(wb, 0, count, wrap_errors, owner + first, self, owner_addr, n_ranks, out, cap, used);
}

#include "../../gubernator_amd/csrc/guber_wire_mesh_pool.h"

static std::atomic<uint64_t> g_small_calls{0};
static int wire_mesh_pool_eval_small(guber_mesh_t* m, const guber_batch_t* gens, guber_result_t* results, uint8_t* const* owner_rank, uint64_t* forwarded, uint64_t* fallbacks) {
    *forwarded = 0; *fallbacks = 0;
    uint32_t with_items = 0;
    for (uint32_t r = 0; r < m->W; ++r) {
        if (!gens[r].n) continue;
        ++with_items;
        if (gens[r].is_owner || gens[r].n > 256u) return fail(GUBER_E_INVALID_ARG, "stand-in mesh: not a small call");
        std::lock_guard<std::mutex> lk(g_oracle_mu);
        oracle_eval_batch(g_oracle, &gens[r], &results[r]);
        if (owner_rank && owner_rank[r]) memset(owner_rank[r], (int)r, gens[r].n);
    }
    if (with_items != 1) return fail(GUBER_E_INVALID_ARG, "stand-in mesh: a direct call carries one rank's RPC");
    g_small_calls.fetch_add(1);
    return GUBER_OK;
}

#include "../../gubernator_amd/csrc/guber_wire_mesh_pool_direct.h"

int main(int argc, char** argv) {
    const int T = argc > 1 ? atoi(argv[1]) : 16, RPCS = argc > 2 ? atoi(argv[2]) : 400;
    const uint32_t W = 3;
    const int KEYS = 24, LIMIT = 40;
    const char* addrs[W] = {"gpu0:8080", "gpu1:8080", "gpu2:8080"};
    g_oracle = oracle_create(1 << 20, 1);
    guber_mesh mesh; mesh.W = W; mesh.max_n = 4096; mesh.eng.resize(W);
    guber_wire_mesh_pool_config_t cfg{};
    cfg.sets = 3; cfg.max_items = 2048; cfg.max_payload_bytes = 1 << 17; cfg.max_rpcs = 16; cfg.batch_wait_us = 200; cfg.wrap_errors = 1;
    guber_wire_mesh_pool_t* pool = nullptr;
    if (guber_wire_mesh_pool_create(&mesh, addrs, &cfg, &pool)) { fprintf(stderr, "create failed: %s\n", g_last_error.c_str()); return 1; }
    guber_wire_mesh_pool_set_clock(pool, 1700000000000ll);
    if (guber_wire_mesh_pool_set_direct(pool, 257, 0) != GUBER_E_INVALID_ARG || guber_wire_mesh_pool_set_direct(pool, 4, 2) != GUBER_OK) return 1;
    std::vector<uint64_t> admitted(KEYS, 0), refused(KEYS, 0), sum_rem(KEYS, 0);
    std::mutex acc_mu;
    std::atomic<int> bad{0};
    auto caller = [&](int t) {
        std::mt19937 rng(77 + t);
        std::vector<uint8_t> resp;
        std::vector<uint64_t> a(KEYS, 0), rf(KEYS, 0), sr(KEYS, 0);
        for (int q = 0; q < RPCS; ++q) {
            std::vector<std::string> keys; std::vector<int> ks;
            const int n = q % 11 == 7 ? 8 : 1 + (int)(rng() % 3);                // mostly lone small RPCs; every eleventh is above the direct path's bound
            const bool with_error = q % 16 == 5 && n > 1;                        // an empty unique_key
            for (int i = 0; i < n; ++i) {
                if (with_error && i == 1) { keys.push_back(""); ks.push_back(-2); }
                else { const int k = (int)(rng() % KEYS); keys.push_back("k" + std::to_string(k)); ks.push_back(k); }
            }
            std::vector<uint8_t> pl = payload_of(keys, LIMIT);
            resp.assign(guber_wire_mesh_pool_response_bound(pool, pl.data(), pl.size()), 0);
            size_t rl = 0;
            const int rc = guber_wire_mesh_pool_get_rate_limits(pool, (uint32_t)((t + q) % W), pl.data(), pl.size(), resp.data(), resp.size(), &rl);
            std::vector<Row> rows;
            if (rc || !parse_resp(resp.data(), rl, rows) || (int)rows.size() != n) { bad++; continue; }
            for (int i = 0; i < n; ++i) {
                const Row& r = rows[i];
                if (ks[i] == -2) { if (!r.err) bad++; continue; }
                if (r.err || r.limit != (uint64_t)LIMIT || r.status > 1) { bad++; continue; }
                if (r.status == 0) { a[ks[i]]++; sr[ks[i]] += r.remaining; } else { rf[ks[i]]++; if (r.remaining) bad++; }
            }
        }
        std::lock_guard<std::mutex> lk(acc_mu);
        for (int k = 0; k < KEYS; ++k) { admitted[k] += a[k]; refused[k] += rf[k]; sum_rem[k] += sr[k]; }
    };
    std::atomic<bool> done{false};
    std::thread toggler([&] {                                               // the path goes off, on for few calls, on for many, while callers are inside
        for (uint32_t i = 0; !done.load(); ++i) {
            guber_wire_mesh_pool_set_direct(pool, i % 3 == 0 ? 0u : 4u, i % 3 == 1 ? 2u : 0u);
            std::this_thread::sleep_for(std::chrono::microseconds(150));
        }
    });
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back(caller, t);
    for (auto& x : th) x.join();
    done.store(true);
    toggler.join();
    // a caller alone in the pool with the path on: direct whatever happened before
    guber_wire_mesh_pool_set_direct(pool, 4, 8);
    {
        std::vector<uint8_t> pl = payload_of({"alone"}, LIMIT), resp(guber_wire_mesh_pool_response_bound(pool, pl.data(), pl.size()), 0);
        size_t rl = 0;
        std::vector<Row> rows;
        if (guber_wire_mesh_pool_get_rate_limits(pool, 1, pl.data(), pl.size(), resp.data(), resp.size(), &rl) || !parse_resp(resp.data(), rl, rows) || rows.size() != 1 || rows[0].remaining != (uint64_t)LIMIT - 1) bad++;
    }
    guber_wire_mesh_pool_stats_t st{}; guber_wire_mesh_pool_direct_stats_t ds{};
    guber_wire_mesh_pool_stats(pool, &st);
    guber_wire_mesh_pool_direct_stats(pool, &ds);
    guber_wire_mesh_pool_destroy(pool);
    int viol = 0;
    for (int k = 0; k < KEYS; ++k) {
        const uint64_t a = admitted[k];
        if (a > (uint64_t)LIMIT || sum_rem[k] != a * LIMIT - a * (a + 1) / 2 || (refused[k] && a != (uint64_t)LIMIT)) viol++;
    }
    printf("%d callers x %d RPCs: %llu RPCs, %llu served by their callers (%llu small calls), %llu sets, bad %d, conservation violations %d\n", T, RPCS,
           (unsigned long long)st.rpcs, (unsigned long long)ds.direct_rpcs, (unsigned long long)g_small_calls.load(), (unsigned long long)st.sets, bad.load(), viol);
    const bool ok = !bad.load() && !viol && st.rpcs == (uint64_t)T * RPCS + 1 && ds.direct_rpcs >= 1 && ds.direct_rpcs == g_small_calls.load() && st.sets >= 1 && ds.fallback_rpcs == 0;
    g_side.clear();
    oracle_destroy(g_oracle);
    printf(ok ? "MESH POOL DIRECT TSAN OK\n" : "MESH POOL DIRECT TSAN FAILED\n");
    return ok ? 0 : 1;
}
