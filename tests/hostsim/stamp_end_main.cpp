// stamp_end_main.cpp — TEST-ONLY, stand-alone (tests/test_stamp_end_asan_cpu.py compiles it under AddressSanitizer and runs it): the engine —
// gubernator_amd/csrc/guber_engine.hip, host code and kernels — compiled for the host against tests/hostsim/fakehip, the way
// cache_ops_main.cpp includes it, with a main() that drives engines created with GUBER_FLAG_TEST_LAST_STAMPS over the end of the 53-bit
// recency stamp through the C ABI (tests/stamp_end_cases.py has the cases):
//   cache operations  Add of 11 items into a cache of 10 with 6 stamps left, as one call and item by item; GetItem on the oldest survivor; one
//                     more Add: the renumbering comes before the call of eleven / before the seventh Add, the victims are items 0 and 2;
//   one pipeline run  the cyclic scan of the pipelines' case — a cache of 300 under 400 keys, batches of 230 + 10 pinned keys, 24 steps, the call
//                     of step 15 the first whose 240 stamps do not fit — against a std::list model of LRUCache (token bucket, one hit per
//                     request: remaining, reset_time, the size and the unexpired evictions of every batch).
// Every "device" buffer is a host allocation here, so k_lru_gather, the sort's buffers and k_lru_renumber writing past the live count, or a
// tail list read past what the renumbering left, is a report.  Nothing is preloaded.
#define FAKEHIP_RUNTIME
#include <hip/hip_runtime.h>
#include "fakehip/fiber_runtime.h"
#include "../../gubernator_amd/csrc/guber_engine.hip"

#include <list>
#include <map>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "stamp_end_main: line %d: %s (%s)\n", __LINE__, #x, guber_last_error()); return 1; } } while (0)

static const int64_t HOUR = 3600000, NOW0 = 1700000000000ll;
static const uint64_t END = 1ull << 53;

static guber_engine_t* engine(uint64_t cache) {
    guber_config_t cfg{};
    cfg.struct_size = sizeof(cfg); cfg.cache_size = cache; cfg.max_batch = 1024; cfg.flags = GUBER_FLAG_TEST_LAST_STAMPS;
    guber_engine_t* e = nullptr;
    return guber_engine_create(&cfg, &e) == GUBER_OK ? e : nullptr;
}
static guber_recency_info_t recency(guber_engine_t* e) {
    guber_recency_info_t r{};
    if (guber_recency_info(e, &r) != GUBER_OK) r.renumbers = ~0ull;
    return r;
}

// one batch in allocations of exactly its sizes (keys + the 8 bytes the kernels may load behind the last one)
struct Batch {
    std::vector<std::string> keys; uint8_t algorithm; int64_t now;
    uint8_t *kb = nullptr, *algo = nullptr, *status = nullptr, *err = nullptr; uint32_t* off = nullptr;
    int64_t *hits = nullptr, *limit = nullptr, *duration = nullptr, *rlimit = nullptr, *remaining = nullptr, *reset = nullptr;
    guber_result_t r{};
    Batch(std::vector<std::string> k, uint8_t a, int64_t now_ms) : keys(std::move(k)), algorithm(a), now(now_ms) {}
    int eval(guber_engine_t* e) {
        const size_t n = keys.size();
        size_t bytes = 0;
        for (auto& s : keys) bytes += s.size();
        kb = (uint8_t*)calloc(bytes + 8, 1); off = (uint32_t*)malloc((n + 1) * 4); algo = (uint8_t*)malloc(n); status = (uint8_t*)malloc(n); err = (uint8_t*)malloc(n);
        hits = (int64_t*)malloc(n * 8); limit = (int64_t*)malloc(n * 8); duration = (int64_t*)malloc(n * 8);
        rlimit = (int64_t*)malloc(n * 8); remaining = (int64_t*)malloc(n * 8); reset = (int64_t*)malloc(n * 8);
        uint32_t o = 0;
        for (size_t i = 0; i < n; ++i) {
            off[i] = o; memcpy(kb + o, keys[i].data(), keys[i].size()); o += (uint32_t)keys[i].size();
            algo[i] = algorithm; hits[i] = 1; limit[i] = 1000; duration[i] = HOUR;
        }
        off[n] = o;
        guber_batch_t b{};
        b.n = (uint32_t)n; b.key_bytes = kb; b.key_off = off; b.hits = hits; b.limit = limit; b.duration = duration; b.algorithm = algo; b.now_ms = now;
        r.status = status; r.limit = rlimit; r.remaining = remaining; r.reset_time = reset; r.err = err;
        return guber_eval_batch(e, &b, &r);
    }
    ~Batch() { free(kb); free(off); free(algo); free(status); free(err); free(hits); free(limit); free(duration); free(rlimit); free(remaining); free(reset); }
};

// stamps and nothing else: requests with an algorithm the reference rejects before it looks at the cache
static int advance_to(guber_engine_t* e, uint64_t seq) {
    for (;;) {
        const guber_recency_info_t r = recency(e);
        CHECK(r.renumbers == 0 && r.next_stamp <= seq);
        if (r.next_stamp == seq) return 0;
        const size_t n = (size_t)std::min<uint64_t>(seq - r.next_stamp, 200);
        std::vector<std::string> keys;
        for (size_t i = 0; i < n; ++i) keys.push_back("late_advance_" + std::to_string(i & 3));
        Batch b(keys, 7, NOW0);
        CHECK(b.eval(e) == GUBER_OK);
        for (size_t i = 0; i < n; ++i) CHECK(b.err[i] != 0);
    }
}

struct Items {                                                             // guber_item_t array whose keys are allocations of exactly their length
    std::vector<guber_item_t> v; std::vector<uint8_t*> keys;
    void add(const std::string& k, int64_t remaining) {
        uint8_t* p = (uint8_t*)malloc(k.size());
        memcpy(p, k.data(), k.size());
        keys.push_back(p);
        guber_item_t it{};
        it.algorithm = 0; it.key = p; it.key_len = (uint32_t)k.size(); it.limit = 10; it.duration = HOUR; it.remaining = remaining;
        it.stamp = NOW0; it.expire_at = NOW0 + HOUR;
        v.push_back(it);
    }
    ~Items() { for (uint8_t* p : keys) free(p); }
};

static int cache_sequence(bool one_call) {
    guber_engine_t* e = engine(10); CHECK(e);
    CHECK(guber_set_clock(e, NOW0) == GUBER_OK);
    CHECK(advance_to(e, END - 6) == 0);
    Items in;
    for (unsigned i = 0; i < 12; ++i) in.add("seq_" + std::to_string(i), 9 - i % 7);
    std::vector<uint8_t> existed(11, 9);
    if (one_call) {
        CHECK(guber_add_items(e, in.v.data(), 11, existed.data()) == GUBER_OK);
        const guber_recency_info_t r = recency(e);
        CHECK(r.renumbers == 1 && r.last_live == 0 && r.next_stamp == 12);              // an empty table: the eleven are 1 .. 11
    } else {
        for (unsigned i = 0; i < 11; ++i) {
            const guber_recency_info_t r0 = recency(e);
            CHECK(r0.renumbers == (i > 6 ? 1u : 0u) && (i > 6 || r0.next_stamp == END - 6 + i));
            CHECK(guber_add_items(e, &in.v[i], 1, &existed[i]) == GUBER_OK);
            if (i == 6) { const guber_recency_info_t r = recency(e); CHECK(r.renumbers == 1 && r.last_live == 6 && r.next_stamp == 8); }
        }
    }
    for (unsigned i = 0; i < 11; ++i) CHECK(existed[i] == 0);
    guber_stats_t st{};
    CHECK(guber_stats(e, &st) == GUBER_OK && st.cache_size == 10 && st.unexpired_evictions == 1);
    guber_item_t it{}; int found = 0;
    CHECK(guber_get_item(e, in.keys[1], in.v[1].key_len, NOW0, &it, &found) == GUBER_OK && found && it.remaining == 8);   // the oldest left: to the front
    CHECK(guber_add_items(e, &in.v[11], 1, nullptr) == GUBER_OK);
    CHECK(guber_stats(e, &st) == GUBER_OK && st.cache_size == 10 && st.unexpired_evictions == 2);
    for (unsigned i = 0; i < 12; ++i) {
        CHECK(guber_get_item(e, in.keys[i], in.v[i].key_len, NOW0, &it, &found) == GUBER_OK);
        CHECK((found != 0) == (i != 0 && i != 2));                                       // the victims: item 0, then item 2
        if (found) CHECK(it.remaining == (int64_t)(9 - i % 7));
    }
    CHECK(recency(e).renumbers == 1);
    guber_engine_destroy(e);
    return 0;
}

// LRUCache (lrucache.go:88-149) for token-bucket requests of one hit that never reach their limit
struct Lru {
    struct Item { std::string key; int64_t remaining, reset; };
    size_t cap; std::list<Item> order; std::map<std::string, std::list<Item>::iterator> at; uint64_t evictions = 0;
    Item& touch(const std::string& k, int64_t now) {
        auto f = at.find(k);
        if (f != at.end()) {
            order.splice(order.begin(), order, f->second);
            f->second->remaining -= 1;
            return *f->second;
        }
        order.push_front(Item{k, 999, now + HOUR});
        at[k] = order.begin();
        if (order.size() > cap) { at.erase(order.back().key); order.pop_back(); ++evictions; }
        return order.front();
    }
};

static int cyclic_scan() {
    const size_t cs = 300, nkeys = 400, bsz = 230, pins = 10, steps = 24, k = 15, n = bsz + pins;
    guber_engine_t* e = engine(cs); CHECK(e);
    CHECK(advance_to(e, END - 100 - k * n) == 0);
    Lru M; M.cap = cs;
    size_t pos = 0;
    uint64_t rebuilds_before = 0;
    for (size_t step = 0; step < steps; ++step) {
        std::vector<std::string> keys;
        for (size_t i = 0; i < bsz; ++i) keys.push_back("ret_" + std::to_string((pos + i) % nkeys));
        for (size_t i = 0; i < pins; ++i) keys.push_back("pin_" + std::to_string(i));
        pos += bsz;
        const int64_t now = NOW0 + (int64_t)step * 1000;
        const guber_recency_info_t r0 = recency(e);
        guber_stats_t st{};
        CHECK(guber_stats(e, &st) == GUBER_OK);
        if (step < k) CHECK(r0.renumbers == 0 && r0.next_stamp + n <= END);
        if (step == k) { CHECK(r0.renumbers == 0 && r0.next_stamp == END - 100 && st.cache_size == (int64_t)cs); rebuilds_before = st.tail_rebuilds; }
        Batch b(keys, 0, now);
        const uint64_t ev0 = M.evictions;
        CHECK(b.eval(e) == GUBER_OK);
        for (size_t i = 0; i < n; ++i) {
            const Lru::Item& m = M.touch(keys[i], now);
            if (b.err[i] != 0 || b.status[i] != 0 || b.rlimit[i] != 1000 || b.remaining[i] != m.remaining || b.reset[i] != m.reset) {
                fprintf(stderr, "stamp_end_main: step %zu request %zu (%s): got err %u status %u remaining %lld reset %lld, the list has remaining %lld reset %lld\n", step, i,
                        keys[i].c_str(), b.err[i], b.status[i], (long long)b.remaining[i], (long long)b.reset[i], (long long)m.remaining, (long long)m.reset);
                return 1;
            }
        }
        CHECK(b.r.cache_size == (int64_t)M.order.size() && b.r.unexpired_evictions == M.evictions - ev0);
        if (step == k) {
            const guber_recency_info_t r = recency(e);
            CHECK(r.renumbers == 1 && r.last_live == cs && r.next_stamp == cs + 1 + n);
            CHECK(guber_stats(e, &st) == GUBER_OK && st.tail_rebuilds == rebuilds_before + 1);
            CHECK(M.evictions - ev0 > 0);                                               // (the cache binds in the call that renumbers)
        }
    }
    CHECK(recency(e).renumbers == 1 && M.evictions > 1000);
    guber_engine_destroy(e);
    return 0;
}

int main() {
    CHECK(cache_sequence(true) == 0);
    CHECK(cache_sequence(false) == 0);
    CHECK(cyclic_scan() == 0);
    printf("STAMP END MAIN OK\n");
    return 0;
}
