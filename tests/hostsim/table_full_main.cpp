// table_full_main.cpp — TEST-ONLY, stand-alone (tests/test_table_full_asan_cpu.py compiles it under AddressSanitizer and runs it): the engine —
// gubernator_amd/csrc/guber_engine.hip, host code and kernels — compiled for the host against tests/hostsim/fakehip, the way
// key_path_main.cpp includes it, with a main() that drives the long-key arena through the C ABI, once on the two-launch and once on the
// owner-partitioned pipeline (tests/table_full_cases.py has the cases' geometry: 4 096 slots, keys of up to 512 bytes, an arena of 1 MiB):
//   1  churn of 408-byte keys over a cache of 1 000: the arena's bound asks for rebuilds, each of which copies the live keys into a new arena;
//   2  3 000 keys of 63 .. 512 bytes, twins that differ in the last byte or are one byte longer: the rebuilds GROW the arena — the copy from
//      the old arena into one of another size is where an off-by-8 shows here —, then new keys, so that the cache evicts;
//   3  GUBER_FLAG_TEST_FIXED_ARENA: 2 570 keys fill the arena, further long keys are refused (error 6, nothing else in the answer), twice,
//      and served after 100 keys have left and the table has been rebuilt.
// Every "device" buffer is a host allocation here, so a kernel that reads or writes past the arena is a report.  Answers are compared with
// a std::map model: one token bucket per key, hits = 1 under a limit that is never reached — remaining counts the key's requests since it
// entered the cache — and the reference's LRU list (the least recently used key leaves when the cache is over its size).
#define FAKEHIP_RUNTIME
#include <hip/hip_runtime.h>
#include "fakehip/fiber_runtime.h"
#include "../../gubernator_amd/csrc/guber_engine.hip"

#include <map>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "table_full_main: line %d: %s (%s)\n", __LINE__, #x, guber_last_error()); return 1; } } while (0)

static const int64_t LIMIT = 1000000, HOUR = 3600000, NOW0 = 1700000000000ll;

struct Model {                                                             // key -> (requests since it entered, last touch), LRU of `cap` keys
    size_t cap; uint64_t clock = 0;
    std::map<std::string, std::pair<int64_t, uint64_t>> m;
    int64_t touch(const std::string& k) {
        auto it = m.find(k);
        if (it == m.end()) {
            it = m.emplace(k, std::make_pair(0, 0)).first;
            if (m.size() > cap) {
                auto old = m.end();
                for (auto j = m.begin(); j != m.end(); ++j) if (j != it && (old == m.end() || j->second.second < old->second.second)) old = j;
                m.erase(old);
            }
        }
        it->second.second = ++clock;
        return ++it->second.first;
    }
};

static std::string key_of(const char* tag, unsigned i, size_t len) {
    char head[32];
    const int h = snprintf(head, sizeof head, "%s_%05u_", tag, i);
    std::string s(head, (size_t)h);
    for (size_t b = s.size(); b < len; ++b) s.push_back((char)('a' + (i * 7u + b * 13u) % 26u));
    return s;
}

// one batch through guber_eval_batch (the key buffer an allocation of exactly the keys' bytes + the 8 the API promises); keys of `refused`
// must come back with error 6 and zeros, the others as the model says
static int run_batch(guber_engine_t* e, Model& M, const std::vector<std::string>& keys, const std::map<std::string, int>* refused, int64_t now, const char* what) {
    const uint32_t n = (uint32_t)keys.size();
    size_t total = 0;
    for (auto& k : keys) total += k.size();
    uint8_t* kb = (uint8_t*)malloc(total + 8);
    memset(kb + total, 0xFF, 8);
    std::vector<uint32_t> off(n + 1), beh(n, 0);
    std::vector<uint8_t> algo(n, 0), status(n, 99), err(n, 99);
    std::vector<int64_t> hits(n, 1), limit(n, LIMIT), duration(n, HOUR), r_limit(n, -7), r_rem(n, -7), r_reset(n, -7);
    size_t at = 0;
    for (uint32_t i = 0; i < n; ++i) { off[i] = (uint32_t)at; memcpy(kb + at, keys[i].data(), keys[i].size()); at += keys[i].size(); }
    off[n] = (uint32_t)at;
    guber_batch_t b{}; guber_result_t r{};
    b.n = n; b.key_bytes = kb; b.key_off = off.data(); b.hits = hits.data(); b.limit = limit.data(); b.duration = duration.data();
    b.algorithm = algo.data(); b.behavior = beh.data(); b.now_ms = now;
    r.status = status.data(); r.err = err.data(); r.limit = r_limit.data(); r.remaining = r_rem.data(); r.reset_time = r_reset.data();
    const int rc = guber_eval_batch(e, &b, &r);
    free(kb);
    if (rc != GUBER_OK) { fprintf(stderr, "table_full_main: %s: guber_eval_batch %d (%s)\n", what, rc, guber_last_error()); return 1; }
    for (uint32_t i = 0; i < n; ++i) {
        if (refused && refused->count(keys[i])) {
            if (!(err[i] == 6 && status[i] == 0 && r_limit[i] == 0 && r_rem[i] == 0 && r_reset[i] == 0)) {
                fprintf(stderr, "table_full_main: %s: request %u of a key without room: err %u status %u limit %lld remaining %lld\n", what, i, err[i], status[i],
                        (long long)r_limit[i], (long long)r_rem[i]);
                return 1;
            }
            continue;
        }
        const int64_t c = M.touch(keys[i]);
        if (!(err[i] == 0 && status[i] == 0 && r_limit[i] == LIMIT && r_rem[i] == LIMIT - c)) {
            fprintf(stderr, "table_full_main: %s: request %u (key of %zu bytes): err %u status %u limit %lld remaining %lld, expected %lld\n", what, i, keys[i].size(),
                    err[i], status[i], (long long)r_limit[i], (long long)r_rem[i], (long long)(LIMIT - c));
            return 1;
        }
    }
    if (guber_size(e) != (int64_t)M.m.size()) { fprintf(stderr, "table_full_main: %s: size %lld, the model has %zu\n", what, (long long)guber_size(e), M.m.size()); return 1; }
    return 0;
}

static guber_engine_t* engine(uint64_t cache, uint32_t flags) {
    guber_config_t cfg{};
    cfg.struct_size = sizeof(cfg); cfg.cache_size = cache; cfg.table_slots = 4096; cfg.max_key_bytes = 512; cfg.max_batch = 1024; cfg.flags = flags;
    guber_engine_t* e = nullptr;
    return guber_engine_create(&cfg, &e) == GUBER_OK ? e : nullptr;
}

static int cases(uint32_t flags, unsigned long long* requests) {
    char what[96];
    int64_t now = NOW0;
    {   // 1: churn over a small cache
        guber_engine_t* e = engine(1000, flags); CHECK(e);
        Model M{1000};
        for (unsigned step = 0; step < 12; ++step, now += 1000) {
            std::vector<std::string> keys;
            for (unsigned i = 0; i < 400; ++i) keys.push_back(key_of("churn", step * 400 + i, 408));
            for (unsigned i = 0; i < 50; ++i) keys.push_back(key_of("resident", i, 408));
            snprintf(what, sizeof what, "flags %u churn step %u", flags, step);
            if (run_batch(e, M, keys, nullptr, now, what)) return 1;
            *requests += keys.size();
        }
        guber_stats_t st{};
        CHECK(guber_stats(e, &st) == GUBER_OK && st.compactions >= 1);
        guber_engine_destroy(e);
    }
    {   // 2: a cache's worth of long keys; the arena grows
        guber_engine_t* e = engine(3000, flags); CHECK(e);
        Model M{3000};
        // (mostly the long ones: the 3 000 keys take about 1.1 MiB, more than the arena's first size)
        static const size_t L[24] = {63, 512, 64, 512, 65, 512, 408, 512, 71, 512, 72, 512, 408, 512, 73, 512, 200, 512, 408, 512, 512, 512, 512, 512};
        std::vector<std::string> all;
        for (unsigned i = 0; all.size() < 3000; ++i) {
            const size_t len = L[(i * 5u + i / 24u) % 24u];
            const std::string k = key_of("long", i, len);
            all.push_back(k);
            if (i % 4 == 0) {
                std::string twin = k; twin.back() = (char)(twin.back() ^ 1);
                all.push_back(twin);
                all.push_back(len < 512 ? k + "q" : k.substr(0, len - 1));
            }
        }
        all.resize(3000);
        for (int round = 0; round < 4; ++round) {
            std::vector<std::string> seq;
            if (round == 2) for (unsigned i = 0; i < 400; ++i) seq.push_back(key_of("late", i, L[i % 24u]));
            else for (size_t i = 0; i < all.size(); ++i) seq.push_back(all[(i * (round == 0 ? 1 : round == 1 ? 1013 : 2003)) % all.size()]);   // (1 013, 2 003: coprime to 3 000)
            for (size_t p = 0; p < seq.size(); p += 400, now += 1000) {
                std::vector<std::string> keys(seq.begin() + p, seq.begin() + std::min(seq.size(), p + 400));
                snprintf(what, sizeof what, "flags %u long keys round %d batch %zu", flags, round, p / 400);
                if (run_batch(e, M, keys, nullptr, now, what)) return 1;
                *requests += keys.size();
            }
        }
        guber_stats_t st{};
        CHECK(guber_stats(e, &st) == GUBER_OK && st.compactions >= 1);
        guber_engine_destroy(e);
    }
    {   // 3: the refusal
        guber_engine_t* e = engine(3000, flags | GUBER_FLAG_TEST_FIXED_ARENA); CHECK(e);
        Model M{3000};
        for (unsigned p = 0; p < 2570; p += 400, now += 1000) {
            std::vector<std::string> keys;
            for (unsigned i = p; i < std::min(2570u, p + 400u); ++i) keys.push_back(key_of("fill", i, 408));
            snprintf(what, sizeof what, "flags %u fill batch %u", flags, p / 400);
            if (run_batch(e, M, keys, nullptr, now, what)) return 1;
            *requests += keys.size();
        }
        std::map<std::string, int> refused;
        std::vector<std::string> X, again;
        for (unsigned i = 0; i < 100; ++i) {
            X.push_back(key_of("fill", i * 25, 408));
            if (i < 40) { X.push_back(key_of("new", i, 408)); refused[X.back()] = 1; again.push_back(X.back()); }
            if (i < 50) X.push_back(key_of("s", i, 12 + i));
            if (i >= 60) X.push_back(key_of("new", (i - 60 + 20) % 40, 408));
        }
        for (int t = 0; t < 2; ++t, ++now) {
            snprintf(what, sizeof what, "flags %u batch X, time %d", flags, t);
            if (run_batch(e, M, X, &refused, now, what)) return 1;
            *requests += X.size();
        }
        for (unsigned i = 0; i < 100; ++i) {
            const std::string k = key_of("fill", i * 25, 408);
            CHECK(guber_remove_item(e, (const uint8_t*)k.data(), (uint32_t)k.size()) == GUBER_OK);
            M.m.erase(k);
        }
        CHECK(guber_compact(e, now) == GUBER_OK);
        { const std::vector<std::string> once = again; again.insert(again.end(), once.rbegin(), once.rend()); }   // (each key twice)
        for (int t = 0; t < 2; ++t, ++now) {
            snprintf(what, sizeof what, "flags %u the refused keys after the rebuild, time %d", flags, t);
            if (run_batch(e, M, again, nullptr, now, what)) return 1;
            *requests += again.size();
        }
        guber_engine_destroy(e);
    }
    return 0;
}

int main() {
    unsigned long long requests = 0;
    if (cases(0u, &requests)) return 1;                                    // the two-launch pipeline
    if (cases(GUBER_FLAG_TEST_FORCE_PART, &requests)) return 1;            // the owner-partitioned pipeline
    printf("TABLE FULL MAIN OK: %llu requests\n", requests);
    return 0;
}
