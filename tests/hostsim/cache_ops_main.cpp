// cache_ops_main.cpp — TEST-ONLY, stand-alone (tests/test_cache_ops_asan_cpu.py compiles it under AddressSanitizer and runs it): the engine —
// gubernator_amd/csrc/guber_engine.hip, host code and kernels — compiled for the host against tests/hostsim/fakehip, the way
// table_full_main.cpp includes it, with a main() that drives the cache operations through the C ABI (tests/cache_ops_cases.py has the cases):
//   b  guber_add_items of 1 200 keys of 4 .. 200 bytes + 300 duplicates under GUBER_FLAG_TEST_WEAK_HASH: the host resubmits in waves, every wave
//      a key buffer of exactly its keys' bytes + 16;
//   f  guber_dump into buffers of exactly the sizes it asks for, and one item / one byte short (GUBER_E_NOMEM, nothing written);
//   i  guber_move_items_by_hash of 200 keys of up to 200 bytes from a table with max_key_bytes 256 into one with 128: the staging rows are
//      min(max_key_bytes) + 16 bytes, padded by hand; keys of 129 bytes are taken, refused and put back, keys of 200 bytes never leave.
// Every "device" buffer is a host allocation here, so a staging row padded past its stride, or a key copied past the buffer it came in, is a
// report.  Every key the caller passes lives in an allocation of exactly its length.  State is compared with a std::map model.
#define FAKEHIP_RUNTIME
#include <hip/hip_runtime.h>
#include "fakehip/fiber_runtime.h"
#include "../../gubernator_amd/csrc/guber_engine.hip"

#include <map>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "cache_ops_main: line %d: %s (%s)\n", __LINE__, #x, guber_last_error()); return 1; } } while (0)

static const int64_t HOUR = 3600000, NOW0 = 1700000000000ll;
typedef std::map<std::string, int64_t> Model;                              // key -> the limit of the last item added under it

static std::string key_of(const char* tag, unsigned i, size_t len) {
    char head[32];
    const int h = snprintf(head, sizeof head, "%s_%u", tag, i);
    std::string s(head, (size_t)h);
    for (size_t b = s.size(); b < len; ++b) s.push_back((char)('a' + (i * 7u + b * 13u) % 26u));
    return s;
}

struct Items {                                                             // guber_item_t array whose keys are allocations of exactly their length
    std::vector<guber_item_t> v; std::vector<uint8_t*> keys;
    void add(const std::string& k, int64_t limit) {
        uint8_t* p = (uint8_t*)malloc(k.size());
        memcpy(p, k.data(), k.size());
        keys.push_back(p);
        guber_item_t it{};
        it.algorithm = 0; it.key = p; it.key_len = (uint32_t)k.size(); it.limit = limit; it.duration = HOUR; it.remaining = limit / 2;
        it.stamp = NOW0; it.expire_at = NOW0 + HOUR;
        v.push_back(it);
    }
    ~Items() { for (uint8_t* p : keys) free(p); }
};

// guber_dump, sizes first, then into allocations of exactly those sizes -> the engine's items as a Model; the protocol's refusals on the way
static int dump_model(guber_engine_t* e, Model& out) {
    uint64_t n = 99, a = 99, n2 = 0, a2 = 0;
    const int rc0 = guber_dump(e, nullptr, 0, nullptr, 0, &n, &a);
    CHECK(rc0 == (n ? GUBER_E_NOMEM : GUBER_OK));
    guber_item_t* items = (guber_item_t*)malloc(n ? n * sizeof(guber_item_t) : 1);
    uint8_t* arena = (uint8_t*)malloc(a ? a : 1);
    if (n) {                                                               // one short: the counts again, nothing written (nothing to write into)
        CHECK(guber_dump(e, items, n - 1, arena, a, &n2, &a2) == GUBER_E_NOMEM && n2 == n && a2 == a);
        CHECK(guber_dump(e, items, n, arena, a - 1, &n2, &a2) == GUBER_E_NOMEM && n2 == n && a2 == a);
    }
    CHECK(guber_dump(e, items, n, arena, a, &n2, &a2) == GUBER_OK && n2 == n && a2 == a);
    out.clear();
    uint64_t bytes = 0;
    for (uint64_t i = 0; i < n; ++i) {
        CHECK(items[i].key >= arena && items[i].key + items[i].key_len <= arena + a);
        CHECK(items[i].remaining == items[i].limit / 2 && items[i].expire_at == NOW0 + HOUR);
        CHECK(out.emplace(std::string((const char*)items[i].key, items[i].key_len), items[i].limit).second);
        bytes += items[i].key_len;
    }
    CHECK(bytes == a);
    free(items); free(arena);
    return 0;
}

static guber_engine_t* engine(uint64_t cache, uint32_t max_key, uint32_t flags, void* stream = nullptr) {
    guber_config_t cfg{};
    cfg.struct_size = sizeof(cfg); cfg.cache_size = cache; cfg.max_key_bytes = max_key; cfg.max_batch = 256; cfg.flags = flags; cfg.stream = stream;
    guber_engine_t* e = nullptr;
    return guber_engine_create(&cfg, &e) == GUBER_OK ? e : nullptr;
}

int main() {
    static const size_t LEN[5] = {0, 0, 63, 64, 200};
    unsigned long long items_added = 0;
    {   // b + f: Add with long keys and duplicates under the weak hash; the dump's capacities
        guber_engine_t* e = engine(4096, 0, GUBER_FLAG_TEST_WEAK_HASH); CHECK(e);
        Model M, got;
        CHECK(dump_model(e, got) == 0 && got.empty());                      // an empty engine: OK with 0 / 0
        Items in;
        std::vector<uint8_t> want;
        for (unsigned j = 0; j < 1500; ++j) {                               // 1 200 keys; every fifth position repeats an earlier key
            const unsigned i = j % 5 == 4 ? (j * 7u) % (j - j / 5) : j - j / 5;
            const std::string k = key_of("ci", i, LEN[i % 5]);
            want.push_back(M.count(k) ? 1 : 0);
            M[k] = 10000 + j;
            in.add(k, 10000 + j);
        }
        CHECK(M.size() == 1200);
        std::vector<uint8_t> existed(in.v.size(), 9);
        CHECK(guber_add_items(e, in.v.data(), (uint32_t)in.v.size(), existed.data()) == GUBER_OK);
        CHECK(existed == want);
        CHECK(guber_size(e) == (int64_t)M.size());
        CHECK(dump_model(e, got) == 0 && got == M);
        for (unsigned i = 0; i < 1200; i += 97) {                           // Get and Remove of long and short keys
            const std::string k = key_of("ci", i, LEN[i % 5]);
            guber_item_t it{}; int found = 0;
            CHECK(guber_get_item(e, (const uint8_t*)in.keys[0], 0, NOW0, &it, &found) == GUBER_OK && !found);
            uint8_t* p = (uint8_t*)malloc(k.size()); memcpy(p, k.data(), k.size());
            CHECK(guber_get_item(e, p, (uint32_t)k.size(), NOW0, &it, &found) == GUBER_OK && found && it.limit == M[k]);
            CHECK(guber_remove_item(e, p, (uint32_t)k.size()) == GUBER_OK);
            CHECK(guber_get_item(e, p, (uint32_t)k.size(), NOW0, &it, &found) == GUBER_OK && !found);
            free(p);
            M.erase(k);
        }
        CHECK(guber_compact(e, NOW0) == GUBER_OK);
        CHECK(dump_model(e, got) == 0 && got == M);
        items_added += in.v.size();
        guber_engine_destroy(e);
    }
    {   // i: 200 keys of up to 200 bytes into a destination that holds 128
        static const size_t MV[5] = {0, 70, 128, 129, 200};
        guber_engine_t* from = engine(4096, 256, 0); CHECK(from);
        guber_engine_t* to = engine(4096, 128, 0, guber_engine_stream(from)); CHECK(to);
        Model M, in_from, in_to;
        Items in;
        std::vector<uint64_t> hashes;
        for (unsigned i = 0; i < 200; ++i) {
            const std::string k = key_of("mv", i, MV[i % 5]);
            M[k] = 500 + i;
            in.add(k, 500 + i);
            hashes.push_back(guber_xxhash64((const uint8_t*)k.data(), k.size(), 0));
        }
        hashes.insert(hashes.begin() + 3, hashes[2]);                       // one hash twice, one that names nothing
        hashes.push_back(0x1234567890abcdefull);
        CHECK(guber_add_items(from, in.v.data(), 200, nullptr) == GUBER_OK);
        uint32_t moved = 0;
        uint64_t* hp = (uint64_t*)malloc(hashes.size() * 8);
        memcpy(hp, hashes.data(), hashes.size() * 8);
        CHECK(guber_move_items_by_hash(from, to, hp, (uint32_t)hashes.size(), &moved) == GUBER_E_TABLE_FULL);   // the keys of 129 bytes went back
        free(hp);
        CHECK(dump_model(from, in_from) == 0 && dump_model(to, in_to) == 0);
        CHECK(moved == 120 && in_to.size() == 120 && in_from.size() == 80);
        CHECK(guber_size(from) == 80 && guber_size(to) == 120);
        for (auto& kv : M) {
            const bool fits = kv.first.size() <= 128;
            CHECK(in_to.count(kv.first) == (fits ? 1u : 0u) && in_from.count(kv.first) == (fits ? 0u : 1u));
            CHECK((fits ? in_to : in_from)[kv.first] == kv.second);
        }
        // and back: the source holds every key
        uint32_t back = 0;
        CHECK(guber_move_items_by_hash(to, from, hashes.data(), (uint32_t)hashes.size(), &back) == GUBER_OK && back == 120);
        CHECK(dump_model(from, in_from) == 0 && in_from == M && dump_model(to, in_to) == 0 && in_to.empty());
        items_added += 200;
        guber_engine_destroy(to); guber_engine_destroy(from);
    }
    printf("CACHE OPS MAIN OK: %llu items\n", items_added);
    return 0;
}
