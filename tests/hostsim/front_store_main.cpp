// front_store_main.cpp — TEST-ONLY, stand-alone (tests/test_front_store_asan_cpu.py compiles it under AddressSanitizer and runs it): the
// engine — gubernator_amd/csrc/guber_engine.hip, host code and kernels — compiled for the host against tests/hostsim/fakehip, the way
// enginesim.cpp includes it, with a main() that drives a front's Store side channel: guber_front_probe_missing_dev -> guber_add_items ->
// guber_front_eval_store_dev for generations of 1, 1 025 and 2 049 requests on three engines.  Every "device" buffer is a host allocation
// of exactly its size, so a kernel (k_fr_elect, k_fr_missing, k_fr_ask, k_fr_out_store) or a copy that reads or writes outside one is a
// report.  index / engine / cut_at are compared with a std::map model; parity with the reference is the Python tests' job.
#define FAKEHIP_RUNTIME
#include <hip/hip_runtime.h>
#include "fakehip/fiber_runtime.h"
#include "../../gubernator_amd/csrc/guber_engine.hip"

#include <map>
#include <set>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "front_store_main: line %d: %s (%s)\n", __LINE__, #x, guber_last_error()); return 1; } } while (0)

template <typename T> static T* exact(const std::vector<T>& v, size_t extra = 0) {      // an allocation of exactly the column's size
    T* p = (T*)malloc((v.size() + extra) * sizeof(T) + (v.empty() && !extra ? 1 : 0));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    if (extra) memset(p + v.size(), 0xA5, extra * sizeof(T));
    return p;
}

int main() {
    const int NE = 3;
    guber_engine_t* eng[NE] = {nullptr, nullptr, nullptr};
    for (int j = 0; j < NE; ++j) {
        guber_config_t cfg{};
        cfg.struct_size = sizeof(cfg); cfg.cache_size = 1 << 14; cfg.max_batch = 512;       // (shares above 512 requests go in pieces)
        cfg.stream = j ? guber_engine_stream(eng[0]) : nullptr;
        CHECK(guber_engine_create(&cfg, &eng[j]) == GUBER_OK);
    }
    guber_placement_t* place = nullptr;
    CHECK(guber_placement_create(NE, 0, &place) == GUBER_OK);
    guber_route_rule rule{};
    CHECK(guber_placement_export(place, &rule) == GUBER_OK);
    rule.global_engine = -1;
    guber_front_t* front = nullptr;
    CHECK(guber_front_create(eng, NE, &rule, 2049, 3, &front) == GUBER_OK);
    const int64_t now = 1700000000000ll;
    std::set<std::string> resident;
    uint64_t asked_total = 0, cuts = 0;
    for (uint32_t n : {1u, 1025u, 2049u}) {
        // n requests over n / 2 + 1 fresh keys of 4 .. 12 bytes; a RESET_REMAINING request at n / 3 whose key comes again at 2 n / 3
        std::vector<std::string> keys(n);
        std::vector<uint32_t> off(n + 1, 0), beh(n, 0);
        std::vector<uint8_t> kb, algo(n, 0);
        std::vector<int64_t> hits(n, 1), limit(n, 50), duration(n, 600000);
        for (uint32_t i = 0; i < n; ++i) {
            char buf[32];
            snprintf(buf, sizeof buf, "a%u_%u", n, (i * 7u) % (n / 2 + 1));
            keys[i] = buf;
        }
        if (n >= 3) { beh[n / 3] = GUBER_BEHAVIOR_RESET_REMAINING; keys[2 * n / 3] = keys[n / 3]; }
        for (uint32_t i = 0; i < n; ++i) { kb.insert(kb.end(), keys[i].begin(), keys[i].end()); off[i + 1] = (uint32_t)kb.size(); }
        uint8_t* d_kb = exact(kb, 8); uint32_t* d_off = exact(off); uint32_t* d_beh = exact(beh); uint8_t* d_algo = exact(algo);
        int64_t *d_hits = exact(hits), *d_limit = exact(limit), *d_dur = exact(duration);
        std::vector<uint8_t> z8(n, 99); std::vector<int64_t> z64(n, -7);
        uint8_t *r_status = exact(z8), *r_err = exact(z8); int64_t *r_limit = exact(z64), *r_rem = exact(z64), *r_reset = exact(z64);
        std::vector<std::pair<uint32_t, uint32_t>> todo{{0u, n}};
        while (!todo.empty()) {
            const uint32_t lo = todo.back().first, hi = todo.back().second, m = hi - lo;
            todo.pop_back();
            guber_batch_t b{}; guber_result_t r{};
            b.n = m; b.key_bytes = d_kb; b.key_off = d_off + lo; b.hits = d_hits + lo; b.limit = d_limit + lo; b.duration = d_dur + lo;
            b.algorithm = d_algo + lo; b.behavior = d_beh + lo; b.now_ms = now;
            r.status = r_status + lo; r.err = r_err + lo; r.limit = r_limit + lo; r.remaining = r_rem + lo; r.reset_time = r_reset + lo;
            // the model: cut_at and the first requests of the keys that are not resident
            std::map<std::string, bool> seen;                       // key -> an earlier request carried the bit
            uint32_t want_cut = m;
            for (uint32_t i = 0; i < m; ++i) {
                auto it = seen.find(keys[lo + i]);
                if (it != seen.end() && it->second) { want_cut = i; break; }
                if (it == seen.end()) it = seen.emplace(keys[lo + i], false).first;
                if (beh[lo + i] & GUBER_BEHAVIOR_RESET_REMAINING) it->second = true;
            }
            std::vector<uint32_t> want;
            std::set<std::string> first;
            for (uint32_t i = 0; i < want_cut; ++i) if (first.insert(keys[lo + i]).second && !resident.count(keys[lo + i])) want.push_back(i);
            std::vector<uint32_t> index(want.size()); std::vector<uint8_t> engine(want.size());
            uint32_t* h_index = exact(index); uint8_t* h_engine = exact(engine);
            guber_front_ask_t ask{h_index, h_engine, (uint32_t)want.size(), 0, 0};
            if (!want.empty()) {                                    // one entry too few first
                ask.cap = (uint32_t)want.size() - 1;
                CHECK(guber_front_probe_missing_dev(front, &b, &ask) == GUBER_E_NOMEM && ask.n == want.size());
                ask.cap = (uint32_t)want.size();
            }
            CHECK(guber_front_probe_missing_dev(front, &b, &ask) == GUBER_OK);
            CHECK(ask.cut_at == want_cut && ask.n == want.size());
            for (uint32_t k = 0; k < ask.n; ++k) {
                uint32_t sh = 0;
                const uint32_t o2[2] = {0, (uint32_t)keys[lo + want[k]].size()};
                std::vector<uint8_t> kk(keys[lo + want[k]].begin(), keys[lo + want[k]].end()); kk.resize(kk.size() + 8, 0);
                CHECK(guber_placement_route_keys(place, kk.data(), o2, 1, &sh, nullptr) == GUBER_OK);
                CHECK(h_index[k] == want[k] && h_engine[k] == sh);
            }
            if (want_cut < m) {
                guber_store_events_t none{nullptr, nullptr};
                uint8_t f1[1]; guber_item_t i1[1]; none.flags = f1; none.items = i1;
                CHECK(guber_front_eval_store_dev(front, &b, &r, &none) == GUBER_E_INVALID_ARG);
                todo.push_back({lo + want_cut, hi});
                todo.push_back({lo, lo + want_cut});
                ++cuts;
                free(h_index); free(h_engine);
                continue;
            }
            // what a Store holds: an item for every second asked key
            std::vector<guber_item_t> items[NE];
            for (uint32_t k = 0; k < ask.n; k += 2) {
                const std::string& key = keys[lo + h_index[k]];
                if (beh[lo + h_index[k]] & GUBER_BEHAVIOR_RESET_REMAINING) continue;      // (a reset of a stored item is a Remove without an OnChange: kept out of the checks below)
                guber_item_t it{};
                it.algorithm = 0; it.key = (const uint8_t*)key.data(); it.key_len = (uint32_t)key.size();
                it.limit = 50; it.duration = 600000; it.remaining = 20; it.stamp = now; it.expire_at = now + 600000;
                items[h_engine[k]].push_back(it);
            }
            for (int j = 0; j < NE; ++j) if (!items[j].empty()) CHECK(guber_add_items(eng[j], items[j].data(), (uint32_t)items[j].size(), nullptr) == GUBER_OK);
            asked_total += ask.n;
            std::vector<uint8_t> fl(m, 0x55); std::vector<guber_item_t> its(m);
            uint8_t* e_flags = exact(fl); guber_item_t* e_items = exact(its);
            guber_store_events_t ev{e_flags, e_items};
            CHECK(guber_front_eval_store_dev(front, &b, &r, &ev) == GUBER_OK);
            for (uint32_t i = 0; i < m; ++i) {
                CHECK(r.err[i] == 0 && r.limit[i] == 50);
                CHECK((e_flags[i] & ~3u) == 0 && (e_flags[i] & GUBER_STORE_ONCHANGE));
                CHECK(e_items[i].key == nullptr && e_items[i].key_len == keys[lo + i].size() && e_items[i].limit == 50);
                resident.insert(keys[lo + i]);
            }
            free(h_index); free(h_engine); free(e_flags); free(e_items);
        }
        free(d_kb); free(d_off); free(d_beh); free(d_algo); free(d_hits); free(d_limit); free(d_dur);
        free(r_status); free(r_err); free(r_limit); free(r_rem); free(r_reset);
    }
    guber_front_store_stats_t st{};
    CHECK(guber_front_store_stats(front, &st) == GUBER_OK);
    CHECK(st.cuts >= cuts && cuts == 2 && st.asked >= asked_total && st.collisions == 0 && st.evaluations >= 3);
    guber_front_destroy(front);
    guber_placement_destroy(place);
    for (int j = 0; j < NE; ++j) guber_engine_destroy(eng[j]);
    printf("FRONT STORE MAIN OK: %llu asked, %llu cuts\n", (unsigned long long)asked_total, (unsigned long long)cuts);
    return 0;
}
