// wire_fuzz_asan.cpp — memory-safety fuzz of the wire front end (the only code of the library that parses bytes from the
// network): mutated GetRateLimitsReq / UpdatePeerGlobalsReq payloads through decode + encode under AddressSanitizer and
// UBSan.  Semantics are checked elsewhere (tests/test_wire_cpu.py against the protobuf runtime); this looks for out-of-bounds
// reads / writes and undefined behaviour only — and for the one thing no other test can see: whether the three walks of a payload's top
// level agree.  The host transcoder (guber_wire_decode_requests), the device decoder's framing (scan_toplevel) and the payload stage's
// item bound (wpl_item_bound: the places an RPC reserves in its stage BEFORE any decoder has seen it) run on the same bytes:
//   scan_toplevel's verdict and count == the host transcoder's;
//   whatever scan_toplevel accepts with `count` records: wpl_item_bound(p, len, cap) >= min(count, cap) for cap 4 / 1000 / 4096 — a bound
//   below the count overfills a stage other callers share — and, below GUBER_WPL_WALK_MAX bytes, == min(count, cap): the stage's occupancy
//   and the choice of the caller's own evaluation rest on the exact number.
// The second half of the run feeds them STRUCTURED top-level chains (records, unknown fields of every wire type and tag width, groups
// empty / filled / nested, their malformed siblings) and mutations of those: byte mutation of plain payloads almost never makes a valid
// group.  An optional file adds chains built elsewhere (tests/wire_shapes.py via tests/test_wire_bound_cpu.py): records of
// u32 length | u32 records expected (0xffffffff: must be turned away) | bytes; the run is then this half alone.  Disagreements are counted, the first few printed; exit 1.
// Build + run:  g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -I include -I tests/hostsim/fakehip
//                   tools/wire_fuzz_asan.cpp gubernator_amd/csrc/wire.cpp -o /tmp/wire_fuzz && /tmp/wire_fuzz 2000000 [shapes.bin]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/guber_wire.h"
// the device decoder's framing logic (scan_toplevel: a host/device template) over a bounds-checked host byte source, and the shared
// record parser it hands the bodies to: the SAME source the kernels k_wire_scan / k_wire_fill compile
#define GUBER_FAKEHIP 1
#include "../tests/hostsim/fakehip/hip/hip_runtime.h"
#include "../gubernator_amd/csrc/guber_kernels_wire.h"

// the few non-wire symbols wire.cpp links against, stubbed (no device here)
extern "C" void* guber_alloc_pinned(size_t) { return nullptr; }
extern "C" void guber_free_pinned(void*) {}
extern "C" int guber_gregorian_expiration(int64_t now_ns, int64_t d, int64_t* out) { *out = now_ns / 1000000 + 1000; return d > 5 ? -3 : 0; }
extern "C" int guber_gregorian_duration(int64_t, int64_t d, int64_t* out) { *out = 60000; return d > 5 ? -3 : 0; }
extern "C" const char* guber_item_strerror(uint8_t e) { return e == 1 ? "Invalid rate limit algorithm '%d'" : "some item error"; }
extern "C" int guber_eval_batch(guber_engine_t*, const guber_batch_t*, guber_result_t*) { return 0; }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static void put_varint(std::string& s, uint64_t v) { while (v >= 0x80) { s.push_back((char)(v | 0x80)); v >>= 7; } s.push_back((char)v); }

static std::string make_requests(int n) {
    std::string payload;
    for (int i = 0; i < n; ++i) {
        std::string r;
        std::string name = (rnd() % 9) ? "ns_" + std::to_string(rnd() % 5) : "";
        std::string uk = (rnd() % 9) ? "acct:\xc3\xa9" + std::to_string(rnd() % 1000) : "";
        r.push_back(0x0a); put_varint(r, name.size()); r += name;
        r.push_back(0x12); put_varint(r, uk.size()); r += uk;
        r.push_back(0x18); put_varint(r, rnd() % 3 ? 1 : rnd());
        r.push_back(0x20); put_varint(r, rnd() % 200);
        r.push_back(0x28); put_varint(r, rnd() % 4 ? 60000 : rnd() % 8);
        if (rnd() % 3 == 0) { r.push_back(0x30); put_varint(r, rnd() % 4); }
        if (rnd() % 3 == 0) { r.push_back(0x38); put_varint(r, rnd() % 64); }
        if (rnd() % 5 == 0) { std::string e = "\x0a\x01k\x12\x01v"; r.push_back(0x4a); put_varint(r, e.size()); r += e; }
        if (rnd() % 4 == 0) { r.push_back(0x50); put_varint(r, rnd()); }
        payload.push_back(0x0a); put_varint(payload, r.size()); payload += r;
    }
    return payload;
}
static std::string make_globals(int n) {
    std::string payload;
    for (int i = 0; i < n; ++i) {
        std::string st;
        st.push_back(0x08); put_varint(st, rnd() % 2); st.push_back(0x10); put_varint(st, rnd() % 100); st.push_back(0x18); put_varint(st, rnd());
        st.push_back(0x20); put_varint(st, 1700000000000ull + rnd() % 100000);
        std::string g, key = "glob_" + std::to_string(rnd() % 100);
        g.push_back(0x0a); put_varint(g, key.size()); g += key;
        g.push_back(0x12); put_varint(g, st.size()); g += st;
        g.push_back(0x18); put_varint(g, rnd() % 3); g.push_back(0x20); put_varint(g, rnd() % 100000); g.push_back(0x28); put_varint(g, rnd());
        payload.push_back(0x0a); put_varint(payload, g.size()); payload += g;
    }
    return payload;
}
static void mutate(std::string& p) {
    const int ops = rnd() % 4;
    for (int k = 0; k < ops && !p.empty(); ++k) {
        const size_t i = rnd() % p.size();
        switch (rnd() % 5) {
        case 0: p[i] ^= (char)(1u << (rnd() % 8)); break;
        case 1: p.insert(p.begin() + i, (char)rnd()); break;
        case 2: p.erase(p.begin() + i); break;
        case 3: p.resize(i); break;
        default: { std::string junk; for (int j = 0, m = 1 + rnd() % 8; j < m; ++j) junk.push_back((char)rnd()); p.insert(i, junk); }
        }
    }
}

namespace fakehip { State S; void yield() {} void barrier() {} unsigned long long wave_exchange(unsigned long long, int, unsigned long long*, unsigned long long*) { return 0; } }
// the device decoder's verdict on one payload: GUBER_OK / GUBER_E_WIRE_MALFORMED and the item count; framed: the top level alone was accepted
static int device_logic(const std::vector<uint8_t>& m, uint32_t& count, bool* framed = nullptr) {
    guber::MemReader rd{m.data(), (uint32_t)m.size()};
    std::vector<std::pair<uint32_t, uint32_t>> recs;
    int32_t st = guber::scan_toplevel(rd, rd.len, 1u << 20, count, [&](uint32_t, uint32_t bo, uint32_t bl) { recs.push_back({bo, bl}); });
    if (framed) *framed = st == guber::WIRE_OK;
    if (st != guber::WIRE_OK) return st;
    for (auto& r : recs) {
        guber::wire::ReqFields f;
        if (!guber::wire::parse_req(m.data() + r.first, m.data() + r.first + r.second, f)) return guber::WIRE_MALFORMED;
    }
    return GUBER_OK;
}


// ---- the payload stage's item bound against the decoders
static long n_undercount = 0, n_inexact = 0, n_verdict = 0, n_printed = 0;
static void show(const char* what, const std::vector<uint8_t>& m) {
    if (n_printed++ >= 8) return;
    printf("%s: %zu bytes", what, m.size());
    for (size_t i = 0; i < m.size() && i < 48; ++i) printf(" %02x", m[i]);
    printf(m.size() > 48 ? " ...\n" : "\n");
}
// a payload whose top level scan_toplevel accepted with `count` records
static void check_bound(const std::vector<uint8_t>& m, uint32_t count) {
    bool low = false, off = false;
    for (uint32_t cap : {4u, 1000u, 4096u}) {
        const uint32_t b = wpl_item_bound(m.data(), m.size(), cap), want = count < cap ? count : cap;
        low = low || b < want;
        off = off || (m.size() < GUBER_WPL_WALK_MAX && b != want);
    }
    if (low) { ++n_undercount; char w[96]; snprintf(w, sizeof w, "item bound BELOW the decoders' count %u (bound %u)", count, wpl_item_bound(m.data(), m.size(), 4096)); show(w, m); }
    else if (off) { ++n_inexact; char w[96]; snprintf(w, sizeof w, "item bound above the decoders' count %u (bound %u)", count, wpl_item_bound(m.data(), m.size(), 4096)); show(w, m); }
}
// (of a payload whose top level was accepted)
static bool has_toplevel_group(const std::vector<uint8_t>& m) {
    const uint8_t* p = m.data(); const uint8_t* e = p + m.size();
    uint64_t tag;
    while (p < e && guber::wire::get_varint(p, e, tag)) {
        if ((tag & 7) == 3) return true;
        if (!guber::wire::skip_field(p, e, (uint32_t)(tag & 7), tag >> 3)) break;
    }
    return false;
}
static void put_tag(std::string& s, uint64_t field, uint32_t wt) { put_varint(s, (field << 3) | wt); }
static uint64_t any_field() { const uint64_t k = rnd() % 8; return k < 5 ? 1 + rnd() % 15 : k == 5 ? 16 + rnd() % 2032 : k == 6 ? (1ull << 25) + rnd() % 1000 : (1ull << 29) - 1 - rnd() % 3; }
static void put_unknown(std::string& s, int depth);
static void put_group(std::string& s, int depth) {
    const uint64_t f = any_field();
    put_tag(s, f, 3);
    for (int k = 0, m = depth < 3 ? rnd() % 4 : 0; k < m; ++k) put_unknown(s, depth + 1);
    if (rnd() % 4 == 0) { std::string r = make_requests(1); s += r; }                  // what looks like a record, inside: never an item
    put_tag(s, rnd() % 40 ? f : any_field(), rnd() % 60 ? 4 : 3);                        // (now and then: another field's END_GROUP, no end at all)
}
static void put_unknown(std::string& s, int depth) {
    switch (rnd() % 6) {
    case 0: put_tag(s, any_field(), 0); put_varint(s, rnd() >> (rnd() % 64)); break;
    case 1: put_tag(s, any_field(), 1); for (int k = 0; k < 8; ++k) s.push_back((char)rnd()); break;
    case 2: put_tag(s, any_field(), 5); for (int k = 0; k < 4; ++k) s.push_back((char)rnd()); break;
    case 3: { uint64_t f = any_field(); if (depth == 0 && f == 1) f = 2; put_tag(s, f, 2); const int n = rnd() % 12; put_varint(s, n); for (int k = 0; k < n; ++k) s.push_back((char)rnd()); break; }
    default: put_group(s, depth);
    }
}
static std::string make_chain() {
    std::string p;
    for (int k = 0, m = 1 + rnd() % 8; k < m; ++k) {
        if (rnd() % 2) p += make_requests(1 + rnd() % 3);
        else if (rnd() % 50) put_unknown(p, 0);
        else put_tag(p, any_field(), rnd() % 3 == 0 ? 4 : 6 + rnd() % 2);               // a stray END_GROUP, a reserved wire type
    }
    return p;
}
struct Shape { std::string bytes; uint32_t expect; };                                  // expect: records, 0xffffffff = must be turned away, 0xfffffffe = unknown
static bool load_shapes(const char* path, std::vector<Shape>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint32_t h[2];
    while (fread(h, 4, 2, f) == 2) {
        Shape sh; sh.bytes.resize(h[0]); sh.expect = h[1];
        if (h[0] && fread(&sh.bytes[0], 1, h[0], f) != h[0]) { fclose(f); return false; }
        out.push_back(sh);
    }
    fclose(f);
    return true;
}
// structured chains and their mutations through the three walks
static int bound_fuzz(long iters, const char* shapes_path) {
    guber_wire_batch_t* b = nullptr;
    if (guber_wire_batch_create(8192, 1u << 20, 0, &b)) return 2;
    std::vector<Shape> shapes;
    if (shapes_path && !load_shapes(shapes_path, shapes)) { printf("cannot read %s\n", shapes_path); return 2; }
    const size_t from_file = shapes.size();
    for (int i = 0; i < 256; ++i) shapes.push_back({make_chain(), 0xfffffffeu});
    long accepted = 0, with_group = 0, pristine_ok = 0;
    for (long it = 0; it < iters; ++it) {
        const bool pristine = (size_t)it < from_file;                                  // every shape of the file once as it is, then mutations
        const size_t k = pristine ? (size_t)it : rnd() % shapes.size();
        if (!pristine && k >= from_file && rnd() % 4 == 0) shapes[k].bytes = make_chain();
        std::string p = shapes[k].bytes;
        const bool mutated = !pristine && rnd() % 4 != 0;
        if (mutated) mutate(p);
        std::vector<uint8_t> exact(p.begin(), p.end());                                // exact-size heap copy: any read past the payload is an ASan error
        guber_wire_batch_reset(b, 1700000000000ll);
        uint32_t first = 0, count = 0, dcount = 0; bool framed = false;
        const int rc = guber_wire_decode_requests(b, exact.data(), exact.size(), 0, 1, &first, &count);
        const int drc = device_logic(exact, dcount, &framed);
        if ((drc == GUBER_OK) != (rc == GUBER_OK) || (rc == GUBER_OK && dcount != count)) { ++n_verdict; show("device framing disagrees with the host transcoder", exact); }
        if (pristine && shapes[k].expect != (rc == GUBER_OK ? count : 0xffffffffu)) { ++n_verdict; show("a built shape is not decoded as it was built", exact); }
        pristine_ok += pristine;
        if (framed) {
            ++accepted;
            with_group += has_toplevel_group(exact);
            check_bound(exact, dcount);
        } else (void)wpl_item_bound(exact.data(), exact.size(), 4096);                 // (any answer will do; the walk stays inside the payload)
    }
    printf("bound fuzz: %ld chains (%zu from the file), %ld accepted by the device framing, %ld of them with a group at the top level: %ld item bounds below the count, %ld above it, %ld verdicts apart\n",
           iters, from_file, accepted, with_group, n_undercount, n_inexact, n_verdict);
    guber_wire_batch_destroy(b);
    return n_undercount || n_inexact || n_verdict ? 1 : 0;
}

// mutated runtime-shaped payloads through decode + encode (and the three walks)
static int parser_fuzz(long iters) {
    guber_wire_batch_t* b = nullptr; guber_wire_items_t* w = nullptr;
    if (guber_wire_batch_create(64, 600, 0, &b) || guber_wire_items_create(24, 200, &w)) return 2;   // tight capacities: FULL paths get exercised
    std::vector<std::string> reqs, globs;
    for (int i = 0; i < 32; ++i) { reqs.push_back(make_requests(1 + rnd() % 12)); globs.push_back(make_globals(1 + rnd() % 10)); }
    long ok = 0, bad = 0, full = 0;
    std::vector<uint8_t> out;
    for (long it = 0; it < iters; ++it) {
        std::string p = reqs[rnd() % reqs.size()];
        mutate(p);
        // exact-size heap copy: any read past the payload is an ASan error
        std::vector<uint8_t> exact(p.begin(), p.end());
        if (rnd() % 7 == 0) guber_wire_batch_reset(b, 1700000000000ll);
        uint32_t first = 0, count = 0;
        const int rc = guber_wire_decode_requests(b, exact.data(), exact.size(), rnd() % 4 ? 0 : 8, rnd() & 1, &first, &count);
        {   // the device decoder's logic must reach the same verdict (capacity aside) and the same item count
            uint32_t dcount = 0;
            bool framed = false;
            const int drc = device_logic(exact, dcount, &framed);
            if (framed) check_bound(exact, dcount);
            const bool host_ok = rc == GUBER_OK || rc == GUBER_E_WIRE_FULL || rc == GUBER_E_WIRE_TOO_LARGE;
            if ((drc == GUBER_OK) != host_ok || (rc == GUBER_OK && dcount != count)) { printf("device framing disagrees with the host transcoder: host rc %d count %u, device rc %d count %u\n", rc, count, drc, dcount); return 1; }
        }
        if (rc == GUBER_OK) {
            ++ok;
            guber_result_t* r = guber_wire_batch_result(b);
            for (uint32_t i = first; i < first + count; ++i) { r->status[i] = rnd() & 1; r->limit[i] = (int64_t)rnd(); r->remaining[i] = (int64_t)rnd(); r->reset_time[i] = (int64_t)rnd(); r->err[i] = rnd() % 6 == 0 ? 1 + rnd() % 3 : 0; }
            out.resize(guber_wire_encode_bound(b, first, count));
            size_t n = 0;
            if (guber_wire_encode_responses(b, first, count, rnd() & 1, out.data(), out.size(), &n) != GUBER_OK || n > out.size()) { printf("encode failed within its own bound\n"); return 1; }
            std::vector<uint8_t> tight(n ? n - 1 : 0);
            size_t need = 0;
            if (n && guber_wire_encode_responses(b, first, count, 0, tight.data(), tight.size(), &need) != GUBER_E_NOMEM && need > tight.size()) { printf("short buffer not reported\n"); return 1; }
            (void)guber_wire_batch_view(b);
        } else if (rc == GUBER_E_WIRE_FULL) { ++full; guber_wire_batch_reset(b, 1700000000000ll); }
        else ++bad;
        std::string q = globs[rnd() % globs.size()];
        mutate(q);
        std::vector<uint8_t> exact2(q.begin(), q.end());
        const guber_item_t* items = nullptr; uint32_t cnt = 0;
        const int rc2 = guber_wire_decode_globals(w, exact2.data(), exact2.size(), 1700000000000ll, &items, &cnt);
        if (rc2 == GUBER_OK) for (uint32_t i = 0; i < cnt; ++i) { volatile uint8_t sink = items[i].key_len ? items[i].key[items[i].key_len - 1] : 0; (void)sink; }
    }
    guber_wire_batch_destroy(b); guber_wire_items_destroy(w);
    printf("wire fuzz: %ld iterations, %ld decoded, %ld rejected, %ld full\n", iters, ok, bad, full);
    return 0;
}

int main(int argc, char** argv) {
    const long iters = argc > 1 ? atol(argv[1]) : 200000;
    const char* shapes_path = argc > 2 ? argv[2] : nullptr;          // (with a file the run is the structured half alone)
    int rc = shapes_path ? 0 : parser_fuzz(iters);
    if (!rc) rc = bound_fuzz(iters, shapes_path);
    if (rc) return rc;
    printf("no sanitizer report\n");
    return 0;
}
