// mesh_rows_main.cpp — TEST-ONLY, stand-alone (tests/test_mesh_rows_asan_cpu.py compiles it under AddressSanitizer and runs it): the engine —
// gubernator_amd/csrc/guber_engine.hip, host code and kernels — compiled for the host against tests/hostsim/fakehip, the way enginesim.cpp
// includes it, with a main() that drives a mesh of three ranks (two engines each, max_key_bytes 16) through guber_mesh_eval_rows_dev:
// generations of 0, 1, 1 025 and 2 049 key ROWS per rank, 24 bytes apart (below the 32 a speculative read needs) or 48, the strides
// changing places from call to call, an empty and an over-long key among them, four calls.  Every "device" buffer is a host allocation of
// exactly its size — the rows n x stride bytes: the last row ends at the allocation's last byte, and every byte behind a key is 0xA5 — so
// a kernel (k_mx_count<true>, k_mx_pack<true>) that reads behind a row, or a copy that leaves a buffer, is a report.  Checked against a
// model: token buckets of hits 1 — a key's UNDER_LIMIT answers over all ranks and calls are min(limit, occurrences) — and the forwarded
// count against guber_ring_route; parity with the reference is the Python tests' job.
#define FAKEHIP_RUNTIME
#include <hip/hip_runtime.h>
#include "fakehip/fiber_runtime.h"
#include "../../gubernator_amd/csrc/guber_engine.hip"

#include <map>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "mesh_rows_main: line %d: %s (%s)\n", __LINE__, #x, guber_last_error()); return 1; } } while (0)

template <typename T> static T* exact(const std::vector<T>& v, size_t extra = 0) {      // an allocation of exactly the column's size
    T* p = (T*)malloc((v.size() + extra) * sizeof(T) + (v.empty() && !extra ? 1 : 0));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    if (extra) memset(p + v.size(), 0xA5, extra * sizeof(T));
    return p;
}

int main() {
    const uint32_t W = 3, NE = 2, MAXKEY = 16, LIMIT = 7;
    guber_engine_t* eng[W][NE]; guber_placement_t* place[W]; guber_front_t* fronts[W];
    for (uint32_t r = 0; r < W; ++r) {
        for (uint32_t j = 0; j < NE; ++j) {
            guber_config_t cfg{};
            cfg.struct_size = sizeof(cfg); cfg.cache_size = 1 << 14; cfg.max_batch = 1024; cfg.max_key_bytes = MAXKEY;   // (an inflow's shares go in pieces)
            cfg.stream = j ? guber_engine_stream(eng[r][0]) : nullptr;
            CHECK(guber_engine_create(&cfg, &eng[r][j]) == GUBER_OK);
        }
        CHECK(guber_placement_create(NE, 0, &place[r]) == GUBER_OK);
        guber_route_rule rule{};
        CHECK(guber_placement_export(place[r], &rule) == GUBER_OK);
        rule.global_engine = -1;
        CHECK(guber_front_create(eng[r], NE, &rule, 2049, 3, &fronts[r]) == GUBER_OK);   // (an inflow above 2 049 goes to the front as several generations)
    }
    const char* names[W] = {"gpu0", "gpu1", "gpu2"};
    guber_ring_t* ring = nullptr;
    CHECK(guber_ring_create(names, W, 512, 0, &ring) == GUBER_OK);
    guber_mesh_t* mesh = nullptr;
    CHECK(guber_mesh_create_local(fronts, W, ring, 2049, &mesh) == GUBER_OK);
    const int64_t now = 1700000000000ll;
    std::map<std::string, uint32_t> seen, under;
    uint64_t forwarded = 0, requests = 0;
    const uint32_t CALLS = 4, sizes[CALLS][W] = {{0, 1025, 2049}, {2049, 1, 1025}, {2049, 2049, 2049}, {1, 0, 1}};
    for (uint32_t c = 0; c < CALLS; ++c) {
        guber_batch_t B[W]; guber_result_t R[W]; guber_mesh_rows_t RW[W];
        std::vector<std::string> keys[W];
        std::vector<void*> owned;
        for (uint32_t r = 0; r < W; ++r) {
            const uint32_t n = sizes[c][r];
            keys[r].resize(n);
            std::vector<uint32_t> off(n + 1, 0), beh(n, 0); std::vector<uint8_t> kb, algo(n, 0);
            std::vector<int64_t> hits(n, 1), limit(n, LIMIT), duration(n, 600000);
            for (uint32_t i = 0; i < n; ++i) {
                char buf[64];
                const uint32_t id = (i * 7u + r * 131u + c * 17u) % 900u;
                snprintf(buf, sizeof buf, "k_%0*u", 1 + (int)(id % 14u), id);      // 3 .. 16 bytes, one width per id
                keys[r][i] = buf;
            }
            if (n > 600) { keys[r][n / 3] = ""; keys[r][n / 2] = std::string(MAXKEY + 1, 'x'); }
            for (uint32_t i = 0; i < n; ++i) { kb.insert(kb.end(), keys[r][i].begin(), keys[r][i].end()); off[i + 1] = (uint32_t)kb.size(); }
            std::vector<uint8_t> z8(n, 99); std::vector<int64_t> z64(n, -7);
            // the rows: exactly n x stride bytes, 0xA5 wherever no key byte lies (an over-long key: the 17 bytes a row of 24 holds)
            const uint32_t stride = ((r + c) & 1u) ? 24u : 48u;
            std::vector<uint8_t> rows((size_t)n * stride, 0xA5); std::vector<uint32_t> klen(n);
            for (uint32_t i = 0; i < n; ++i) { klen[i] = (uint32_t)keys[r][i].size(); memcpy(rows.data() + (size_t)i * stride, keys[r][i].data(), keys[r][i].size()); }
            uint8_t* d_rows = exact(rows); uint32_t* d_klen = exact(klen);
            owned.push_back(d_rows); owned.push_back(d_klen);
            uint8_t* d_kb = exact(kb, 8); uint32_t* d_off = exact(off);                       // (packed: for the host ring only)
            uint32_t* d_beh = exact(beh); uint8_t* d_algo = exact(algo);
            int64_t *d_hits = exact(hits), *d_limit = exact(limit), *d_dur = exact(duration);
            uint8_t *r_status = exact(z8), *r_err = exact(z8); int64_t *r_limit = exact(z64), *r_rem = exact(z64), *r_reset = exact(z64);
            for (void* p : {(void*)d_kb, (void*)d_off, (void*)d_beh, (void*)d_algo, (void*)d_hits, (void*)d_limit, (void*)d_dur, (void*)r_status, (void*)r_err,
                            (void*)r_limit, (void*)r_rem, (void*)r_reset}) owned.push_back(p);
            B[r] = guber_batch_t{}; R[r] = guber_result_t{};
            RW[r] = guber_mesh_rows_t{n ? stride : 0u, n ? d_klen : nullptr};
            B[r].n = n; B[r].key_bytes = d_rows; B[r].key_off = nullptr; B[r].hits = d_hits; B[r].limit = d_limit; B[r].duration = d_dur;
            B[r].algorithm = d_algo; B[r].behavior = d_beh; B[r].now_ms = now;
            R[r].status = r_status; R[r].err = r_err; R[r].limit = r_limit; R[r].remaining = r_rem; R[r].reset_time = r_reset;
            if (n) {
                std::vector<uint32_t> owner(n);
                CHECK(guber_ring_route(ring, d_kb, d_off, n, owner.data()) == GUBER_OK);
                for (uint32_t i = 0; i < n; ++i) if (!keys[r][i].empty() && keys[r][i].size() <= MAXKEY && owner[i] != r) ++forwarded;
            }
            requests += n;
        }
        B[2].is_owner = (const uint8_t*)B[2].behavior;
        CHECK(guber_mesh_eval_rows_dev(mesh, B, RW, R) == GUBER_E_INVALID_ARG);  // the ring decides ownership
        B[2].is_owner = nullptr;
        CHECK(guber_mesh_eval_rows_dev(mesh, B, RW, R) == GUBER_OK);
        CHECK(guber_mesh_synchronize(mesh) == GUBER_OK);
        for (uint32_t r = 0; r < W; ++r)
            for (uint32_t i = 0; i < B[r].n; ++i) {
                const std::string& k = keys[r][i];
                if (k.empty()) { CHECK(R[r].err[i] == 4); continue; }            // GUBER_ITEM_E_EMPTY_KEY
                if (k.size() > MAXKEY) { CHECK(R[r].err[i] == 7); continue; }    // GUBER_ITEM_E_KEY_TOO_LONG
                CHECK(R[r].err[i] == 0 && R[r].limit[i] == LIMIT && R[r].status[i] <= 1);
                ++seen[k];
                if (R[r].status[i] == 0) ++under[k];
            }
        for (void* p : owned) free(p);
    }
    for (auto& kv : seen) CHECK(under[kv.first] == std::min<uint32_t>(LIMIT, kv.second));
    guber_mesh_stats_t st{};
    CHECK(guber_mesh_stats(mesh, &st) == GUBER_OK);
    CHECK(st.calls == CALLS && st.requests == requests && st.forwarded == forwarded && forwarded > 0 && st.inflow_pieces > 9);
    int64_t resident = 0;
    for (uint32_t r = 0; r < W; ++r) for (uint32_t j = 0; j < NE; ++j) resident += guber_size(eng[r][j]);
    CHECK(resident == (int64_t)seen.size());
    guber_mesh_destroy(mesh);
    guber_ring_destroy(ring);
    for (uint32_t r = 0; r < W; ++r) {
        guber_front_destroy(fronts[r]);
        guber_placement_destroy(place[r]);
        for (uint32_t j = 0; j < NE; ++j) guber_engine_destroy(eng[r][j]);
    }
    printf("MESH ROWS MAIN OK: %llu requests, %llu forwarded, %llu pieces\n", (unsigned long long)requests, (unsigned long long)forwarded, (unsigned long long)st.inflow_pieces);
    return 0;
}
