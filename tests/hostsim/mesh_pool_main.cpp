// mesh_pool_main.cpp — TEST-ONLY, stand-alone (tests/test_mesh_pool_asan_cpu.py compiles it under AddressSanitizer through mesh_pool.mk and runs
// it): the engine — gubernator_amd/csrc/guber_engine.hip, host code and kernels — compiled for the host against tests/hostsim/fakehip, the way
// enginesim.cpp includes it, with a main() that drives guber_wire_mesh_pool_*: a mesh of three ranks, six caller threads (two per rank), each
// sending RPCS payloads of ONE length L, a multiple of 16, to its rank.  max_payload_bytes is exactly L, so every RPC fills its stage's
// staging buffer to its last 16 bytes, and the rank's other caller, when it asks while the set is open, seals the set;
// every response buffer is an allocation of exactly guber_wire_mesh_pool_response_bound bytes (cap = the bound), and every second RPC carries
// an item with an empty unique_key, so that the caller marshals it through the host transcoder at that cap.  The "device" buffers are host
// allocations here: a byte behind any of them, behind a staging buffer or behind a response is a report.  Checked: the number of answers
// per RPC, the countdown of every caller's own key, the statistics.  Parity of the bytes is the Python tests' job.  Nothing is preloaded.
#define FAKEHIP_RUNTIME
#include <hip/hip_runtime.h>
#include "fakehip/fiber_runtime.h"
#include "../../gubernator_amd/csrc/guber_engine.hip"

#include <string>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "mesh_pool_main: line %d: %s (%s)\n", __LINE__, #x, guber_last_error()); return 1; } } while (0)

static void put_varint(std::string& s, uint64_t v) { while (v >= 0x80) { s.push_back((char)(v | 0x80)); v >>= 7; } s.push_back((char)v); }
static void put_str(std::string& s, uint8_t tag, const std::string& v) { s.push_back((char)tag); put_varint(s, v.size()); s += v; }
static void put_int(std::string& s, uint8_t tag, uint64_t v) { if (v) { s.push_back((char)tag); put_varint(s, v); } }
static void put_request(std::string& msg, const std::string& name, const std::string& ukey, int64_t limit) {
    std::string r;
    put_str(r, 0x0a, name); put_str(r, 0x12, ukey); put_int(r, 0x18, 1); put_int(r, 0x20, (uint64_t)limit); put_int(r, 0x28, 600000);
    msg.push_back(0x0a); put_varint(msg, r.size()); msg += r;
}
static bool get_varint(const uint8_t*& p, const uint8_t* e, uint64_t& v) {
    v = 0;
    for (int sh = 0; p < e && sh < 64; sh += 7) { const uint8_t b = *p++; v |= (uint64_t)(b & 0x7f) << sh; if (!(b & 0x80)) return true; }
    return false;
}
// the answers of a GetRateLimitsResp: how many, and `remaining` (field 3) of answer `at`
static bool read_response(const uint8_t* p, size_t len, uint32_t at, uint32_t* count, uint64_t* remaining) {
    const uint8_t* e = p + len;
    *count = 0;
    while (p < e) {
        uint64_t L;
        if (*p++ != 0x0a || !get_varint(p, e, L) || L > (uint64_t)(e - p)) return false;
        const uint8_t* q = p; const uint8_t* qe = p + L;
        while (q < qe) {
            uint64_t tag, v;
            if (!get_varint(q, qe, tag)) return false;
            if ((tag & 7) == 2) { if (!get_varint(q, qe, v) || v > (uint64_t)(qe - q)) return false; q += v; }
            else { if (!get_varint(q, qe, v)) return false; if (tag == 0x18 && *count == at) *remaining = v; }
        }
        p += L; ++*count;
    }
    return p == e;
}

int main() {
    const uint32_t W = 3, T = 6, RPCS = 12, ITEMS = 40, MAXKEY = 40;
    guber_engine_t* eng[W]; guber_front_t* fronts[W];
    for (uint32_t r = 0; r < W; ++r) {
        guber_config_t cfg{};
        cfg.struct_size = sizeof(cfg); cfg.cache_size = 1 << 14; cfg.max_batch = 1024; cfg.max_key_bytes = MAXKEY;
        CHECK(guber_engine_create(&cfg, &eng[r]) == GUBER_OK);
        CHECK(guber_front_create(&eng[r], 1, nullptr, 1024, 3, &fronts[r]) == GUBER_OK);
    }
    const std::string a0 = "gpu0:808080", a1 = std::string(123, 'b') + ":8081", a2 = std::string(259, 'c') + ":8082";
    const char* names[W] = {a0.c_str(), a1.c_str(), a2.c_str()};
    guber_ring_t* ring = nullptr;
    CHECK(guber_ring_create(names, W, 512, 0, &ring) == GUBER_OK);
    guber_mesh_t* mesh = nullptr;
    CHECK(guber_mesh_create_local(fronts, W, ring, 1024, &mesh) == GUBER_OK);
    // every payload has the same length: keys of six digits, a bad item's unique_key is empty and its name six bytes longer; the caller's own
    // key is padded until that length is a multiple of 16
    std::string pad;
    auto payload_of = [&](uint32_t t, uint32_t q) {
        std::string m;
        for (uint32_t i = 0; i < ITEMS; ++i) {
            char buf[32];
            if (i == t) { snprintf(buf, sizeof buf, "own%03u", t); put_request(m, "k", buf + pad, 100000); }
            else if ((q & 1) && i == ITEMS - 1) put_request(m, "kkkkkkk", "", 7);
            else { snprintf(buf, sizeof buf, "%06u", ((q * ITEMS + i) * 37u + t * 1009u) % 3000u * 37u); put_request(m, "k", buf, 7); }
        }
        return m;
    };
    pad.assign((16 - payload_of(0, 0).size() % 16) % 16, 'z');
    const size_t L = payload_of(0, 0).size();
    CHECK(L % 16 == 0 && payload_of(5, 1).size() == L && payload_of(3, 2).size() == L);
    guber_wire_mesh_pool_config_t wc{};
    wc.sets = 2; wc.max_items = 1024; wc.max_rpcs = 8; wc.max_payload_bytes = (uint32_t)L; wc.batch_wait_us = 2000; wc.wrap_errors = 1;
    guber_wire_mesh_pool_t* pool = nullptr;
    CHECK(guber_wire_mesh_pool_create(mesh, names, &wc, &pool) == GUBER_OK);
    CHECK(guber_wire_mesh_pool_set_clock(pool, 1700000000000ll) == GUBER_OK);
    std::atomic<int> bad{0};
    auto caller = [&](uint32_t t) {
        for (uint32_t q = 0; q < RPCS; ++q) {
            const std::string m = payload_of(t, q);
            const size_t bound = guber_wire_mesh_pool_response_bound(pool, (const uint8_t*)m.data(), m.size());
            uint8_t* resp = (uint8_t*)malloc(bound);                  // exactly the bound: a byte behind it is a report
            size_t n = 0;
            const int rc = guber_wire_mesh_pool_get_rate_limits(pool, t % W, (const uint8_t*)m.data(), m.size(), resp, bound, &n);
            uint32_t count = 0; uint64_t rem = 0;
            if (rc != GUBER_OK || n > bound || !read_response(resp, n, t, &count, &rem) || count != ITEMS || rem != 100000u - 1u - q) {
                fprintf(stderr, "mesh_pool_main: caller %u RPC %u: rc %d, %zu bytes, %u answers, own key at %llu (%s)\n", t, q, rc, n, count, (unsigned long long)rem, guber_last_error());
                bad++;
            }
            free(resp);
        }
    };
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < T; ++t) th.emplace_back(caller, t);
    for (auto& x : th) x.join();
    CHECK(bad.load() == 0);
    // more than a stage's bytes is turned away at the door, and a cap below the bound before the RPC joins a set
    {
        std::string big = payload_of(0, 0) + payload_of(0, 2);
        std::vector<uint8_t> resp(guber_wire_mesh_pool_response_bound(pool, (const uint8_t*)big.data(), big.size()));
        size_t n = 0;
        CHECK(guber_wire_mesh_pool_get_rate_limits(pool, 0, (const uint8_t*)big.data(), big.size(), resp.data(), resp.size(), &n) == GUBER_E_WIRE_FULL);
        const std::string m = payload_of(0, 0);
        CHECK(guber_wire_mesh_pool_get_rate_limits(pool, 0, (const uint8_t*)m.data(), m.size(), resp.data(), 10, &n) == GUBER_E_NOMEM);
    }
    guber_wire_mesh_pool_stats_t st{};
    CHECK(guber_wire_mesh_pool_stats(pool, &st) == GUBER_OK);
    CHECK(st.rpcs == (uint64_t)T * RPCS && st.items == (uint64_t)T * RPCS * ITEMS && st.host_rpcs == (uint64_t)T * RPCS / 2 && st.sets <= st.rpcs && st.forwarded > 0);
    CHECK(st.sealed_full + st.sealed_wait + st.sealed_idle == st.sets);
    guber_wire_mesh_pool_destroy(pool);
    guber_mesh_destroy(mesh);
    guber_ring_destroy(ring);
    for (uint32_t r = 0; r < W; ++r) { guber_front_destroy(fronts[r]); guber_engine_destroy(eng[r]); }
    printf("MESH POOL MAIN OK: %llu RPCs in %llu sets (full %llu, wait %llu, idle %llu), %llu forwarded\n", (unsigned long long)st.rpcs, (unsigned long long)st.sets,
           (unsigned long long)st.sealed_full, (unsigned long long)st.sealed_wait, (unsigned long long)st.sealed_idle, (unsigned long long)st.forwarded);
    return 0;
}
