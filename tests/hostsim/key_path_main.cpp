// key_path_main.cpp — TEST-ONLY, stand-alone (tests/test_key_path_asan_cpu.py compiles it under AddressSanitizer and runs it): the engine —
// gubernator_amd/csrc/guber_engine.hip, host code and kernels — compiled for the host against tests/hostsim/fakehip, the way
// front_store_main.cpp includes it, with a main() that sends generations of fixed-width keys through guber_front_eval_dev on three engines:
// widths 1 .. 32 around the steps of the speculative key fetch (key_fetch_spec: 8, 16, 16 + 8, 32 bytes) and of the uniform-length hash,
// generations of 1, 1 024 and 1 025 requests.  The key buffer is an allocation of exactly n x width + 8 bytes (what include/guber_gpu.h
// promises behind the last key) filled with 0xFF behind the keys, every column one of exactly its size: a kernel (k_fr_count, k_fr_scatter)
// that reads a byte further is a report.  The engines take 256 requests at a time, so a share goes in two pieces and the second one's
// keys start at d0 x width — an odd address for odd widths — in the front's mirror (BatchView::key_width: no offsets).
// Every answer is compared with a std::map model (one token bucket per key, hits = 1 under a limit that is never reached: remaining
// counts the key's requests so far, so a key hashed, routed or compared wrongly shows); parity with the reference is the Python tests' job.
#define FAKEHIP_RUNTIME
#include <hip/hip_runtime.h>
#include "fakehip/fiber_runtime.h"
#include "../../gubernator_amd/csrc/guber_engine.hip"

#include <map>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "key_path_main: line %d: %s (%s)\n", __LINE__, #x, guber_last_error()); return 1; } } while (0)

template <typename T> static T* exact(const std::vector<T>& v) {          // an allocation of exactly the column's size
    T* p = (T*)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

int main() {
    const int NE = 3;
    const int64_t LIMIT = 1000000, now = 1700000000000ll;
    guber_engine_t* eng[NE] = {nullptr, nullptr, nullptr};
    for (int j = 0; j < NE; ++j) {
        guber_config_t cfg{};
        cfg.struct_size = sizeof(cfg); cfg.cache_size = 1 << 14; cfg.max_batch = 256;       // (shares above 256 requests go in pieces)
        cfg.stream = j ? guber_engine_stream(eng[0]) : nullptr;
        CHECK(guber_engine_create(&cfg, &eng[j]) == GUBER_OK);
    }
    guber_placement_t* place = nullptr;
    CHECK(guber_placement_create(NE, 0, &place) == GUBER_OK);
    guber_route_rule rule{};
    CHECK(guber_placement_export(place, &rule) == GUBER_OK);
    rule.global_engine = -1;
    guber_front_t* front = nullptr;
    CHECK(guber_front_create(eng, NE, &rule, 1025, 3, &front) == GUBER_OK);
    std::map<std::string, int64_t> seen;                                   // key -> requests so far
    unsigned long long total = 0, gens = 0;
    for (uint32_t W : {1u, 7u, 8u, 9u, 15u, 16u, 17u, 24u, 25u, 31u, 32u}) {
        for (uint32_t n : {1u, 1024u, 1025u}) {
            // n requests over min(n / 2 + 1, 200) keys of W bytes, none of them zero: the key's number in base 255, then a pattern
            const uint32_t K = std::min<uint32_t>(n / 2 + 1, 200u);
            std::vector<std::string> keys(n);
            for (uint32_t i = 0; i < n; ++i) {
                uint32_t k = (i * 7u + W) % K;
                std::string s(W, '\0');
                s[0] = (char)(k + 1);
                for (uint32_t b = 1; b < W; ++b) s[b] = (char)(((k * 31u + b * 17u + W) % 255u) + 1u);
                keys[i] = s;
            }
            std::vector<uint8_t> kb((size_t)n * W + 8, 0xFF), algo(n, 0);
            std::vector<uint32_t> off(n + 1), beh(n, 0);
            for (uint32_t i = 0; i < n; ++i) { memcpy(kb.data() + (size_t)i * W, keys[i].data(), W); off[i] = i * W; }
            off[n] = n * W;
            std::vector<int64_t> hits(n, 1), limit(n, LIMIT), duration(n, 600000);
            uint8_t* d_kb = exact(kb); uint32_t* d_off = exact(off); uint32_t* d_beh = exact(beh); uint8_t* d_algo = exact(algo);
            int64_t *d_hits = exact(hits), *d_limit = exact(limit), *d_dur = exact(duration);
            std::vector<uint8_t> z8(n, 99); std::vector<int64_t> z64(n, -7);
            uint8_t *r_status = exact(z8), *r_err = exact(z8); int64_t *r_limit = exact(z64), *r_rem = exact(z64), *r_reset = exact(z64);
            guber_batch_t b{}; guber_result_t r{};
            b.n = n; b.key_bytes = d_kb; b.key_off = d_off; b.hits = d_hits; b.limit = d_limit; b.duration = d_dur;
            b.algorithm = d_algo; b.behavior = d_beh; b.now_ms = now;
            r.status = r_status; r.err = r_err; r.limit = r_limit; r.remaining = r_rem; r.reset_time = r_reset;
            uint32_t done = 0;
            CHECK(guber_front_eval_dev(front, &b, &r, 1, &done) == GUBER_OK && done == 1);
            CHECK(guber_front_synchronize(front) == GUBER_OK);
            for (uint32_t i = 0; i < n; ++i) {
                const int64_t c = ++seen[keys[i]];
                if (!(r.err[i] == 0 && r.status[i] == 0 && r.limit[i] == LIMIT && r.remaining[i] == LIMIT - c)) {
                    fprintf(stderr, "key_path_main: width %u n %u request %u: err %u status %u limit %lld remaining %lld, expected %lld\n", W, n, i, r.err[i], r.status[i],
                            (long long)r.limit[i], (long long)r.remaining[i], (long long)(LIMIT - c));
                    return 1;
                }
            }
            total += n; ++gens;
            free(d_kb); free(d_off); free(d_beh); free(d_algo); free(d_hits); free(d_limit); free(d_dur);
            free(r_status); free(r_err); free(r_limit); free(r_rem); free(r_reset);
        }
    }
    guber_front_stats_t st{};
    CHECK(guber_front_stats(front, &st) == GUBER_OK && st.generations == gens && st.forced_flushes == 0);
    uint64_t resident = 0;
    for (int j = 0; j < NE; ++j) { const int64_t sz = guber_size(eng[j]); CHECK(sz >= 0); resident += (uint64_t)sz; }
    CHECK(resident == seen.size());
    guber_front_destroy(front);
    guber_placement_destroy(place);
    for (int j = 0; j < NE; ++j) guber_engine_destroy(eng[j]);
    printf("KEY PATH MAIN OK: %llu requests in %llu generations, %zu keys\n", total, gens, seen.size());
    return 0;
}
