// mesh_small_main.cpp — TEST-ONLY, stand-alone (tests/test_mesh_small_asan_cpu.py compiles it under AddressSanitizer and runs it): the
// engine — gubernator_amd/csrc/guber_engine.hip, host code and kernels — compiled for the host against tests/hostsim/fakehip, the way
// enginesim.cpp includes it, with a main() that drives the one-launch path of a mesh of three ranks (two engines each):
// guber_mesh_eval_small over totals of 1, 64, 256, 255 and 129 ragged keys spread unevenly over the ranks, among them an empty and an
// over-long key, a call of 257 that is refused, and a call in which one key's requests differ (a share that falls back).  Every buffer
// the call is handed — keys (8 readable bytes behind the last, as include/guber_gpu.h promises), columns, answers, the owner column — is
// a host allocation of exactly its size, so a kernel (k_mx_small) or a copy that reads or writes outside one is a report.  Checked against
// a model: token buckets of hits 1 — a key's UNDER_LIMIT answers over all ranks and calls are min(limit, occurrences) — and the forwarded
// count and the owner column against guber_ring_route; parity with the reference is the Python tests' job.
#define FAKEHIP_RUNTIME
#include <hip/hip_runtime.h>
#include "fakehip/fiber_runtime.h"
#include "../../gubernator_amd/csrc/guber_engine.hip"

#include <map>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "mesh_small_main: line %d: %s (%s)\n", __LINE__, #x, guber_last_error()); return 1; } } while (0)

template <typename T> static T* exact(const std::vector<T>& v, size_t extra = 0) {      // an allocation of exactly the column's size
    T* p = (T*)malloc((v.size() + extra) * sizeof(T) + (v.empty() && !extra ? 1 : 0));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    if (extra) memset(p + v.size(), 0xA5, extra * sizeof(T));
    return p;
}

int main() {
    const uint32_t W = 3, NE = 2, MAXKEY = 24, LIMIT = 7;
    guber_engine_t* eng[W][NE]; guber_placement_t* place[W]; guber_front_t* fronts[W];
    for (uint32_t r = 0; r < W; ++r) {
        for (uint32_t j = 0; j < NE; ++j) {
            guber_config_t cfg{};
            cfg.struct_size = sizeof(cfg); cfg.cache_size = 1 << 14; cfg.max_batch = 1024; cfg.max_key_bytes = MAXKEY;
            cfg.stream = j ? guber_engine_stream(eng[r][0]) : nullptr;
            CHECK(guber_engine_create(&cfg, &eng[r][j]) == GUBER_OK);
        }
        CHECK(guber_placement_create(NE, 0, &place[r]) == GUBER_OK);
        guber_route_rule rule{};
        CHECK(guber_placement_export(place[r], &rule) == GUBER_OK);
        rule.global_engine = -1;
        CHECK(guber_front_create(eng[r], NE, &rule, 256, 3, &fronts[r]) == GUBER_OK);
    }
    const char* names[W] = {"gpu0", "gpu1", "gpu2"};
    guber_ring_t* ring = nullptr;
    CHECK(guber_ring_create(names, W, 512, 0, &ring) == GUBER_OK);
    guber_mesh_t* mesh = nullptr;
    CHECK(guber_mesh_create_local(fronts, W, ring, 256, &mesh) == GUBER_OK);
    const int64_t now = 1700000000000ll;
    std::map<std::string, uint32_t> seen, under;
    uint64_t forwarded = 0, requests = 0, calls = 0;
    const uint32_t NC = 7;
    const uint32_t sizes[NC][W] = {{0, 1, 0}, {0, 0, 64}, {100, 0, 156}, {85, 85, 85}, {100, 100, 57}, {43, 43, 43}, {0, 0, 0}};
    for (uint32_t c = 0; c < NC; ++c) {
        guber_batch_t B[W]; guber_result_t R[W]; uint8_t* OW[W];
        std::vector<std::string> keys[W];
        std::vector<uint32_t> owners[W];
        std::vector<void*> owned;
        uint32_t total = 0;
        for (uint32_t r = 0; r < W; ++r) {
            const uint32_t n = sizes[c][r];
            total += n;
            keys[r].resize(n);
            std::vector<uint32_t> off(n + 1, 0), beh(n, 0); std::vector<uint8_t> kb, algo(n, 0);
            std::vector<int64_t> hits(n, 1), limit(n, LIMIT), duration(n, 600000);
            for (uint32_t i = 0; i < n; ++i) {
                char buf[64];
                const uint32_t id = (i * 7u + r * 131u + c * 17u) % 300u;
                snprintf(buf, sizeof buf, "k_%0*u", 1 + (int)(id % 21u), id);      // 3 .. 23 bytes, one width per id
                keys[r][i] = buf;
            }
            if (n > 40) { keys[r][n / 3] = ""; keys[r][n / 2] = std::string(MAXKEY + 1, 'x'); }
            if (c == 5) for (uint32_t i = 0; i < n; i += 9) { keys[r][i] = "k_differs"; duration[i] = 600000 + i; }   // (one key, requests that differ: its share falls back)
            for (uint32_t i = 0; i < n; ++i) { kb.insert(kb.end(), keys[r][i].begin(), keys[r][i].end()); off[i + 1] = (uint32_t)kb.size(); }
            std::vector<uint8_t> z8(n, 99); std::vector<int64_t> z64(n, -7);
            uint8_t* d_kb = exact(kb, 8); uint32_t* d_off = exact(off); uint32_t* d_beh = exact(beh); uint8_t* d_algo = exact(algo);
            int64_t *d_hits = exact(hits), *d_limit = exact(limit), *d_dur = exact(duration);
            uint8_t *r_status = exact(z8), *r_err = exact(z8), *r_owner = exact(z8); int64_t *r_limit = exact(z64), *r_rem = exact(z64), *r_reset = exact(z64);
            for (void* p : {(void*)d_kb, (void*)d_off, (void*)d_beh, (void*)d_algo, (void*)d_hits, (void*)d_limit, (void*)d_dur, (void*)r_status, (void*)r_err,
                            (void*)r_owner, (void*)r_limit, (void*)r_rem, (void*)r_reset}) owned.push_back(p);
            B[r] = guber_batch_t{}; R[r] = guber_result_t{};
            B[r].n = n; B[r].key_bytes = d_kb; B[r].key_off = d_off; B[r].hits = d_hits; B[r].limit = d_limit; B[r].duration = d_dur;
            B[r].algorithm = c % 2 ? d_algo : nullptr; B[r].behavior = c % 2 ? nullptr : d_beh; B[r].now_ms = now;      // (optional columns given and NULL)
            R[r].status = r_status; R[r].err = r_err; R[r].limit = r_limit; R[r].remaining = r_rem; R[r].reset_time = r_reset;
            OW[r] = r_owner;
            owners[r].resize(n);
            if (n) CHECK(guber_ring_route(ring, d_kb, d_off, n, owners[r].data()) == GUBER_OK);
        }
        if (total > 256) {
            CHECK(guber_mesh_eval_small(mesh, B, R, OW) == GUBER_E_BATCH_TOO_LARGE);
            for (void* p : owned) free(p);
            continue;
        }
        B[1].is_owner = (const uint8_t*)B[1].hits;
        CHECK(guber_mesh_eval_small(mesh, B, R, OW) == GUBER_E_INVALID_ARG);     // the ring decides ownership
        B[1].is_owner = nullptr;
        CHECK(guber_mesh_eval_small(mesh, B, R, OW) == GUBER_OK);
        ++calls; requests += total;
        for (uint32_t r = 0; r < W; ++r)
            for (uint32_t i = 0; i < B[r].n; ++i) {
                const std::string& k = keys[r][i];
                if (k.empty()) { CHECK(R[r].err[i] == 4 && OW[r][i] == 0xff); continue; }            // GUBER_ITEM_E_EMPTY_KEY
                if (k.size() > MAXKEY) { CHECK(R[r].err[i] == 7 && OW[r][i] == 0xff); continue; }    // GUBER_ITEM_E_KEY_TOO_LONG
                CHECK(R[r].err[i] == 0 && R[r].limit[i] == LIMIT && R[r].status[i] <= 1 && OW[r][i] == owners[r][i]);
                if (owners[r][i] != r) ++forwarded;
                ++seen[k];
                if (R[r].status[i] == 0) ++under[k];
            }
        for (void* p : owned) free(p);
    }
    for (auto& kv : seen) CHECK(under[kv.first] == std::min<uint32_t>(LIMIT, kv.second));
    guber_mesh_stats_t st{}; guber_mesh_small_stats_t ss{};
    CHECK(guber_mesh_stats(mesh, &st) == GUBER_OK && guber_mesh_small_stats(mesh, &ss) == GUBER_OK);
    CHECK(st.calls == calls && st.requests == requests && st.forwarded == forwarded && forwarded > 0);
    CHECK(ss.calls == calls - 1 && ss.launches == 3 * (calls - 1) && ss.wholesale_fallbacks == 0 && ss.share_fallbacks == 1);
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
    printf("MESH SMALL MAIN OK: %llu requests, %llu forwarded, %llu launches, %llu shares re-run\n", (unsigned long long)requests, (unsigned long long)forwarded,
           (unsigned long long)ss.launches, (unsigned long long)ss.share_fallbacks);
    return 0;
}
