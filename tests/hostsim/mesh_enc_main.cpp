// mesh_enc_main.cpp — TEST-ONLY, stand-alone (tests/test_mesh_enc_asan_cpu.py compiles it under AddressSanitizer through mesh_enc.mk and runs
// it): the engine — gubernator_amd/csrc/guber_engine.hip, host code and kernels — compiled for the host against tests/hostsim/fakehip, the
// way enginesim.cpp includes it, with a main() that drives guber_wire_dev_eval_mesh_enc in the shape of tests/mesh_enc_cases.py's case a: a
// mesh of three ranks (two engines each), a decoder per rank, RPCs of 0, 1, 3, 4, 5, 63, 64, 65, P - 1, P, P + 1 and 2 P + 1 items (P = the
// piece of k_wire_enc_owner) mixed across the ranks of a call and moving one rank on from call to call, a rank without a decoder, a
// decoder that decoded nothing, peers with addresses of 11, 128 and 264 bytes.  Every buf, off, len and owner_rank the caller hands over
// is an allocation of exactly its required size — buf: guber_wire_dev_mesh_enc_bound bytes — so a byte written behind any of them is a
// report, as is a kernel (k_mx_count's item_owner[], k_wire_enc_owner) or a copy that leaves a "device" buffer: they are host allocations
// here.  Checked against guber_ring_route: owner_rank, the forwarded count, and per RPC the number of answers and the address behind every
// answer another rank owns; parity of the bytes with the protobuf runtime is the Python tests' job.  Nothing is preloaded.
#define FAKEHIP_RUNTIME
#include <hip/hip_runtime.h>
#include "fakehip/fiber_runtime.h"
#include "../../gubernator_amd/csrc/guber_engine.hip"

#include <string>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "mesh_enc_main: line %d: %s (%s)\n", __LINE__, #x, guber_last_error()); return 1; } } while (0)

static void put_varint(std::string& s, uint64_t v) { while (v >= 0x80) { s.push_back((char)(v | 0x80)); v >>= 7; } s.push_back((char)v); }
static void put_str(std::string& s, uint8_t tag, const std::string& v) { s.push_back((char)tag); put_varint(s, v.size()); s += v; }
static void put_int(std::string& s, uint8_t tag, uint64_t v) { if (v) { s.push_back((char)tag); put_varint(s, v); } }
// one RateLimitReq of a GetRateLimitsReq: name "k", unique_key, hits 1, limit, duration (gubernator.proto:137-182)
static void put_request(std::string& msg, const std::string& ukey, int64_t limit) {
    std::string r;
    put_str(r, 0x0a, "k"); put_str(r, 0x12, ukey); put_int(r, 0x18, 1); put_int(r, 0x20, (uint64_t)limit); put_int(r, 0x28, 600000);
    msg.push_back(0x0a); put_varint(msg, r.size()); msg += r;
}
static bool get_varint(const uint8_t*& p, const uint8_t* e, uint64_t& v) {
    v = 0;
    for (int sh = 0; p < e && sh < 64; sh += 7) { const uint8_t b = *p++; v |= (uint64_t)(b & 0x7f) << sh; if (!(b & 0x80)) return true; }
    return false;
}

int main() {
    const uint32_t W = 3, NE = 2, MAXKEY = 40, P = guber::WEO_P, CALLS = 6;
    const uint32_t S[12] = {0, 1, 3, 4, 5, 63, 64, 65, P - 1, P, P + 1, 2 * P + 1};
    guber_engine_t* eng[W][NE]; guber_placement_t* place[W]; guber_front_t* fronts[W]; guber_wire_dev_t* dec[W];
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
        CHECK(guber_front_create(eng[r], NE, &rule, 1024, 3, &fronts[r]) == GUBER_OK);
        CHECK(guber_wire_dev_create(eng[r][0], 1024, 1 << 18, 16, &dec[r]) == GUBER_OK);
    }
    const std::string a0 = "gpu0:808080", a1 = std::string(123, 'b') + ":8081", a2 = std::string(259, 'c') + ":8082";
    CHECK(a0.size() == 11 && a1.size() == 128 && a2.size() == GUBER_WIRE_OWNER_ADDR_MAX);
    const char* names[W] = {a0.c_str(), a1.c_str(), a2.c_str()};
    guber_ring_t* ring = nullptr;
    CHECK(guber_ring_create(names, W, 512, 0, &ring) == GUBER_OK);
    guber_mesh_t* mesh = nullptr;
    CHECK(guber_mesh_create_local(fronts, W, ring, 1024, &mesh) == GUBER_OK);
    const int64_t now = 1700000000000ll;
    uint64_t forwarded = 0, requests = 0, answers_with_owner = 0;
    for (uint32_t c = 0; c < CALLS; ++c) {
        guber_wire_dev_t* decs[W]; guber_wire_mesh_resp_t out[W];
        std::vector<uint32_t> owner[W], counts[W];
        uint32_t n_items[W] = {0, 0, 0};
        for (uint32_t r = 0; r < W; ++r) {
            decs[r] = dec[r]; out[r] = guber_wire_mesh_resp_t{};
            std::vector<std::string> msgs; std::vector<uint8_t> kb; std::vector<uint32_t> off(1, 0);
            const bool none = c % 4 == 1 && r == c % 3, nothing = c % 4 == 3 && r == c % 3;
            for (uint32_t k = 0; k < 4 && !none && !nothing; ++k) {
                const uint32_t cnt = S[(c + 3 * k + r) % 12];
                std::string m;
                for (uint32_t i = 0; i < cnt; ++i) {
                    char buf[32];
                    snprintf(buf, sizeof buf, "%06u", ((n_items[r] + i) * 37u + r * 1009u + c * 131u) % 5000u * 37u);
                    put_request(m, buf, 7);
                    const std::string key = std::string("k_") + buf;
                    kb.insert(kb.end(), key.begin(), key.end()); off.push_back((uint32_t)kb.size());
                }
                msgs.push_back(m); counts[r].push_back(cnt); n_items[r] += cnt;
            }
            if (none) { decs[r] = nullptr; continue; }
            std::vector<const uint8_t*> ptr; std::vector<uint32_t> len;
            for (auto& m : msgs) { ptr.push_back((const uint8_t*)m.data()); len.push_back((uint32_t)m.size()); }
            std::vector<int32_t> st(msgs.size() + 1); uint32_t n = 0;
            CHECK(guber_wire_dev_decode(dec[r], ptr.data(), len.data(), (uint32_t)msgs.size(), nullptr, 4096, now, st.data(), nullptr, nullptr, &n) == GUBER_OK);
            CHECK(n == n_items[r]);
            for (size_t q = 0; q < msgs.size(); ++q) CHECK(st[q] == GUBER_OK);
            owner[r].resize(n);
            if (n) {
                kb.resize(kb.size() + 8, 0xA5);
                CHECK(guber_ring_route(ring, kb.data(), off.data(), n, owner[r].data()) == GUBER_OK);
                for (uint32_t i = 0; i < n; ++i) if (owner[r][i] != r) ++forwarded;
            }
            requests += n;
            // exactly the required sizes, each ending at its allocation's last byte
            const size_t bound = guber_wire_dev_mesh_enc_bound(dec[r], names, W);
            CHECK((bound == 0) == (n == 0));
            out[r].buf = (uint8_t*)malloc(bound ? bound : 1); out[r].cap = bound;
            out[r].off = (uint32_t*)malloc(msgs.size() ? msgs.size() * 4 : 1); out[r].len = (uint32_t*)malloc(msgs.size() ? msgs.size() * 4 : 1);
            out[r].owner_rank = (uint8_t*)malloc(n ? n : 1);
        }
        CHECK(guber_wire_dev_eval_mesh_enc(decs, mesh, names, 1, out) == GUBER_OK);
        for (uint32_t r = 0; r < W; ++r) {
            if (!decs[r]) continue;
            CHECK(guber_wire_dev_mesh_enc_host_rpcs(dec[r]) == 0);
            uint32_t i = 0; size_t end = 0;
            for (size_t q = 0; q < counts[r].size(); ++q) {
                CHECK(out[r].off[q] == end);
                const uint8_t* p = out[r].buf + out[r].off[q]; const uint8_t* e = p + out[r].len[q];
                uint32_t got = 0;
                while (p < e) {
                    uint64_t L;
                    CHECK(*p++ == 0x0a && get_varint(p, e, L) && L <= (uint64_t)(e - p));
                    CHECK(out[r].owner_rank[i] == owner[r][i]);
                    const std::string& a = owner[r][i] == 0 ? a0 : owner[r][i] == 1 ? a1 : a2;
                    const bool has = L >= a.size() && memcmp(p + L - a.size(), a.data(), a.size()) == 0 && memchr(p, 'o', L) != nullptr;
                    CHECK(has == (owner[r][i] != r));
                    answers_with_owner += has;
                    p += L; ++got; ++i;
                }
                CHECK(p == e && got == counts[r][q]);
                end += out[r].len[q];
            }
            CHECK(i == n_items[r] && end <= out[r].cap);
            free(out[r].buf); free(out[r].off); free(out[r].len); free(out[r].owner_rank);
        }
    }
    guber_mesh_stats_t st{};
    CHECK(guber_mesh_stats(mesh, &st) == GUBER_OK);
    CHECK(st.calls == CALLS && st.requests == requests && st.forwarded == forwarded && forwarded > 0 && answers_with_owner == forwarded);
    guber_mesh_destroy(mesh);
    guber_ring_destroy(ring);
    for (uint32_t r = 0; r < W; ++r) {
        guber_wire_dev_destroy(dec[r]);
        guber_front_destroy(fronts[r]);
        guber_placement_destroy(place[r]);
        for (uint32_t j = 0; j < NE; ++j) guber_engine_destroy(eng[r][j]);
    }
    printf("MESH ENC MAIN OK: %llu requests, %llu forwarded\n", (unsigned long long)requests, (unsigned long long)forwarded);
    return 0;
}
