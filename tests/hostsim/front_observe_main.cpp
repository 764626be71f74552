// front_observe_main.cpp — TEST-ONLY, stand-alone (tests/test_front_observe_asan_cpu.py compiles it under AddressSanitizer and runs it): the
// engine — gubernator_amd/csrc/guber_engine.hip, host code and kernels — compiled for the host against tests/hostsim/fakehip, the way
// enginesim.cpp includes it, with a main() that runs a front's observation kernels (k_fr_observe, k_fr_observe_top) on buffers that end
// exactly where they may be read: packed keys in an allocation that ends 8 bytes behind the last key, key ROWS (what the device wire
// decoder leaves: key i at i x key_stride, padding that is not zero) in an allocation that ends with the last row.  A kernel that reads
// outside one is a report.  What the window counted is compared with a std::map model over the host's XXH64 and the placement's own
// slot_of; once more with the per-tile aggregation switched off (the laboratory knob).  Parity of the answers is the Python tests' job.
#define FAKEHIP_RUNTIME
#include <hip/hip_runtime.h>
#include "fakehip/fiber_runtime.h"
#include "../../gubernator_amd/csrc/guber_engine.hip"
#include "../../gubernator_amd/csrc/guber_placement_impl.h"

#include <map>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "front_observe_main: line %d: %s (%s)\n", __LINE__, #x, guber_last_error()); return 1; } } while (0)

template <typename T> static T* exact(const std::vector<T>& v, size_t extra = 0) {      // an allocation of exactly the column's size
    T* p = (T*)malloc((v.size() + extra) * sizeof(T) + (v.empty() && !extra ? 1 : 0));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    if (extra) memset(p + v.size(), 0xA5, extra * sizeof(T));
    return p;
}

static const int NE = 4;
static guber_front_t* front;
static guber_placement_t* place;

// one generation of `keys` through the front — packed (stride 0: the buffer ends 8 bytes behind the last key) or as rows of `stride` bytes
// (the buffer ends with the last row) — and its window against the model
static int generation(const std::vector<std::string>& keys, uint32_t stride, int64_t now) {
    const uint32_t n = (uint32_t)keys.size();
    std::vector<uint8_t> kb, algo(n, 0);
    std::vector<uint32_t> off(n + 1, 0), len(n), beh(n, 0);
    std::vector<int64_t> hits(n, 1), limit(n, 1000000), duration(n, 600000);
    for (uint32_t i = 0; i < n; ++i) {
        len[i] = (uint32_t)keys[i].size();
        if (stride) { kb.resize((size_t)i * stride, 0); kb.insert(kb.end(), keys[i].begin(), keys[i].end()); kb.resize((size_t)(i + 1) * stride, 0xA5); }
        else kb.insert(kb.end(), keys[i].begin(), keys[i].end());
        off[i + 1] = (uint32_t)kb.size();
    }
    uint8_t* d_kb = exact(kb, stride ? 0 : 8); uint32_t* d_off = exact(off); uint32_t* d_len = exact(len); uint32_t* d_beh = exact(beh); uint8_t* d_algo = exact(algo);
    int64_t *d_hits = exact(hits), *d_limit = exact(limit), *d_dur = exact(duration);
    std::vector<uint8_t> z8(n, 99); std::vector<int64_t> z64(n, -7);
    uint8_t *r_status = exact(z8), *r_err = exact(z8); int64_t *r_limit = exact(z64), *r_rem = exact(z64), *r_reset = exact(z64);
    FrontGen g;
    g.b = guber_batch_t{};
    g.b.n = n; g.b.key_bytes = d_kb; g.b.key_off = stride ? nullptr : d_off; g.b.hits = d_hits; g.b.limit = d_limit; g.b.duration = d_dur;
    g.b.algorithm = d_algo; g.b.behavior = d_beh; g.b.now_ms = now;
    g.key_stride = stride; g.key_len = stride ? d_len : nullptr;
    guber_result_t r{};
    r.status = r_status; r.err = r_err; r.limit = r_limit; r.remaining = r_rem; r.reset_time = r_reset;
    uint32_t done = 0;
    CHECK(front_eval(front, &g, &r, 1, &done) == GUBER_OK && done == 1);
    CHECK(guber_front_synchronize(front) == GUBER_OK);
    for (uint32_t i = 0; i < n; ++i) CHECK(r_err[i] == 0 && r_limit[i] == 1000000);
    // the model
    std::map<uint64_t, uint32_t> count;
    std::vector<uint32_t> want_slots(place->n_slots, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t h = guber_xxhash64((const uint8_t*)keys[i].data(), keys[i].size(), 0);
        count[h]++; want_slots[place->slot_of(h)]++;
    }
    std::vector<uint32_t> sw(place->n_slots, 0xA5A5A5A5u), cc(FO_TOP_MAX, 0); std::vector<uint64_t> hh(FO_TOP_MAX, 0);
    uint32_t* o_sw = exact(sw); uint32_t* o_cc = exact(cc); uint64_t* o_hh = exact(hh);
    guber_front_observation_t o{};
    o.slot_w = o_sw; o.slot_cap = place->n_slots; o.hash = o_hh; o.count = o_cc; o.cap = FO_TOP_MAX;
    CHECK(guber_front_observation(front, &o) == GUBER_OK);
    CHECK(o.observed == n && o.skipped == 0 && o.dropped == 0 && o.generations == 1 && o.n_slots == place->n_slots);
    CHECK(o.threshold == std::max<uint32_t>(1, n / (NE * 64)));
    for (uint32_t s = 0; s < place->n_slots; ++s) CHECK(o_sw[s] == want_slots[s]);
    uint32_t want_top = 0;
    for (auto& kv : count) want_top += kv.second >= o.threshold;
    CHECK(o.n == want_top);
    std::map<uint64_t, uint32_t> got;
    for (uint32_t k = 0; k < o.n; ++k) { CHECK(got.emplace(o_hh[k], o_cc[k]).second); CHECK(count.count(o_hh[k]) && count[o_hh[k]] == o_cc[k] && o_cc[k] >= o.threshold); }
    free(d_kb); free(d_off); free(d_len); free(d_beh); free(d_algo); free(d_hits); free(d_limit); free(d_dur);
    free(r_status); free(r_err); free(r_limit); free(r_rem); free(r_reset); free(o_sw); free(o_cc); free(o_hh);
    return 0;
}

// n keys drawn from `distinct` of them (key k: `width` bytes, or — width 0 — between lo and hi), a few of them often
static std::vector<std::string> draw(uint32_t n, uint32_t distinct, uint32_t width, uint32_t lo, uint32_t hi, uint32_t salt) {
    std::vector<std::string> keys(n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t k = (i % 3 == 0) ? i % 5 : (i * 2654435761u + salt) % distinct;
        char buf[96];
        snprintf(buf, sizeof buf, "%u_%u_", salt, k);
        std::string s(buf);
        const uint32_t w = width ? width : lo + k % (hi - lo + 1);
        while (s.size() < w) s += (char)('a' + (k + s.size()) % 26);
        s.resize(w);
        if (w >= 4) { s[w - 1] = (char)('0' + k % 10); s[w - 2] = (char)('0' + k / 10 % 10); s[w - 3] = (char)('0' + k / 100 % 10); s[w - 4] = (char)('0' + k / 1000 % 10); }
        keys[i] = s;
    }
    return keys;
}

int main() {
    guber_engine_t* eng[NE] = {nullptr, nullptr, nullptr, nullptr};
    for (int j = 0; j < NE; ++j) {
        guber_config_t cfg{};
        cfg.struct_size = sizeof(cfg); cfg.cache_size = 1 << 14; cfg.max_batch = 4096;
        cfg.stream = j ? guber_engine_stream(eng[0]) : nullptr;
        CHECK(guber_engine_create(&cfg, &eng[j]) == GUBER_OK);
    }
    CHECK(guber_placement_create(NE, 0, &place) == GUBER_OK);
    guber_route_rule rule{};
    CHECK(guber_placement_export(place, &rule) == GUBER_OK);
    rule.global_engine = -1;
    CHECK(guber_front_create(eng, NE, &rule, 4097, 3, &front) == GUBER_OK);
    int64_t now = 1700000000000ll;
    uint32_t runs = 0;
    for (int no_agg = 0; no_agg < 2; ++no_agg) {
        if (no_agg) setenv("GUBER_FRONT_OBSERVE_NO_AGG", "1", 1);        // (read by guber_front_observe in this -DGUBER_LAB build)
        CHECK(guber_front_observe(front, 1) == GUBER_OK);
        for (uint32_t n : {1u, 64u, 1025u, 4097u}) {
            // packed: one width of 16 bytes (the speculative fetch, also for the buffer's last key), of 31, ragged 5 .. 40
            if (generation(draw(n, 300, 16, 0, 0, 1 + runs), 0, now += 500)) return 1;
            if (generation(draw(n, 300, 31, 0, 0, 2 + runs), 0, now += 500)) return 1;
            if (generation(draw(n, 300, 0, 5, 40, 3 + runs), 0, now += 500)) return 1;
            // rows: every key fills its row (the last row's key ends at the allocation's last byte: stride 16 fetched ahead, stride 40 hashed from
            // memory), and ragged keys in rows of 24 with the last one full
            if (generation(draw(n, 300, 16, 0, 0, 4 + runs), 16, now += 500)) return 1;
            if (generation(draw(n, 300, 40, 0, 0, 5 + runs), 40, now += 500)) return 1;
            std::vector<std::string> rag = draw(n, 300, 0, 4, 24, 6 + runs);
            rag.back().resize(24, 'z');
            if (generation(rag, 24, now += 500)) return 1;
            runs += 6;
        }
    }
    guber_front_destroy(front);
    guber_placement_destroy(place);
    for (int j = NE - 1; j >= 0; --j) guber_engine_destroy(eng[j]);
    printf("FRONT OBSERVE MAIN OK: %u generations\n", runs);
    return 0;
}
