/* peer_abi_c99.c — the calls go/wire_server.go's getPeerRateLimits and updatePeerGlobals handlers make, in plain C99 against the public
 * headers (cgo compiles the binding's preamble as C): gcc -std=c99 -pedantic -Werror must take it and it must link against the product
 * library (tests/test_gpu_wire_peer.py runs it with --gpu; tests/test_wire_peer_cpu.py compiles it and runs it without a device, where engine
 * creation must fail with GUBER_E_NO_DEVICE — never evaluate on the CPU). */
#include <stdio.h>
#include <string.h>

#include "guber_gpu.h"
#include "guber_wire.h"

/* one RateLimitResp of a response: 0a <len> { 08 status  10 limit  18 remaining  20 reset_time  2a <len> error } — single-byte varints but reset_time */
typedef struct { unsigned status, limit, remaining, has_error; } row_t;
static int parse_rows(const uint8_t* p, size_t n, row_t* rows, int cap) {
    int k = 0;
    size_t i = 0;
    while (i < n) {
        size_t end;
        if (p[i] != 0x0a || k == cap) return -1;
        end = i + 2 + p[i + 1];
        if (p[i + 1] >= 0x80 || end > n) return -1;
        memset(&rows[k], 0, sizeof rows[k]);
        i += 2;
        while (i < end) {
            const uint8_t tag = p[i++];
            if (tag == 0x2a) { rows[k].has_error = 1; i += 1 + p[i]; continue; }
            if (tag == 0x20) { while (p[i] & 0x80) ++i; ++i; continue; }
            if (tag == 0x08) rows[k].status = p[i];
            else if (tag == 0x10) rows[k].limit = p[i];
            else if (tag == 0x18) rows[k].remaining = p[i];
            else return -1;
            if (p[i++] & 0x80) return -1;
        }
        ++k;
    }
    return k;
}

static int peer_sequence(int want_gpu) {
    /* GetPeerRateLimitsReq: RateLimitReq{name "n", unique_key "g", hits H, limit 100, duration 60000, behavior GLOBAL} x 2 (H = 60, then 50: more than
     * remains — the peer RPC drains), then {name "n", unique_key "" (absent), hits 1, limit 100, duration 60000}: served on the key "n_" */
    static const uint8_t req[] = {0x0a, 16, 0x0a, 1, 'n', 0x12, 1, 'g', 0x18, 60, 0x20, 100, 0x28, 0xe0, 0xd4, 0x03, 0x38, 2,
                                  0x0a, 16, 0x0a, 1, 'n', 0x12, 1, 'g', 0x18, 50, 0x20, 100, 0x28, 0xe0, 0xd4, 0x03, 0x38, 2,
                                  0x0a, 11, 0x0a, 1, 'n', 0x18, 1, 0x20, 100, 0x28, 0xe0, 0xd4, 0x03};
    /* UpdatePeerGlobalsReq: UpdatePeerGlobal{key "n_u", status {limit 9, remaining 4, reset_time 1700000060000}, algorithm TOKEN (absent), duration 60000} */
    static const uint8_t upd[] = {0x0a, 22, 0x0a, 3, 'n', '_', 'u', 0x12, 11, 0x10, 9, 0x18, 4, 0x20, 0xe0, 0xa4, 0x99, 0xff, 0xbc, 0x31, 0x20, 0xe0, 0xd4, 0x03};
    /* the read of it: {name "n", unique_key "u", hits 0 (absent), limit 9, duration 60000, behavior GLOBAL} */
    static const uint8_t rd[] = {0x0a, 14, 0x0a, 1, 'n', 0x12, 1, 'u', 0x20, 9, 0x28, 0xe0, 0xd4, 0x03, 0x38, 2};
    guber_config_t cfg;
    guber_engine_t* eng[2] = {NULL, NULL};
    guber_placement_t* place = NULL;
    guber_wire_pool_t* pool = NULL;
    guber_wire_pool_config_t wc;
    struct guber_route_rule rule;
    uint8_t resp[2048];
    row_t rows[4];
    size_t n = 0;
    uint32_t installed = 0;
    int rc, k;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = (uint32_t)sizeof cfg; cfg.cache_size = 4096; cfg.max_batch = 1024; cfg.max_key_bytes = 64;
    rc = guber_engine_create(&cfg, &eng[0]);
    if (rc != GUBER_OK) {
        printf("engine: %s (%s)\n", guber_strerror(rc), guber_last_error());
        return want_gpu ? rc : (rc == GUBER_E_NO_DEVICE ? GUBER_OK : rc);
    }
    cfg.stream = guber_engine_stream(eng[0]);
    rc = guber_engine_create(&cfg, &eng[1]);
    if (rc == GUBER_OK) rc = guber_placement_create(2, 0, &place);
    if (rc == GUBER_OK) rc = guber_placement_export(place, &rule);
    memset(&wc, 0, sizeof wc);
    wc.stages = 2; wc.max_items = 1024; wc.max_payload_bytes = 1u << 16; wc.max_rpcs = 8;
    if (rc == GUBER_OK) { rule.global_engine = -1; rc = guber_wire_pool_create(eng, 2, &rule, &wc, &pool); }
    if (rc == GUBER_OK) rc = guber_wire_pool_set_clock(pool, 1700000000000LL);
    /* getPeerRateLimits */
    if (rc == GUBER_OK && guber_wire_pool_response_bound(req, sizeof req) > sizeof resp) rc = GUBER_E_NOMEM;
    if (rc == GUBER_OK) rc = guber_wire_pool_get_peer_rate_limits(pool, req, sizeof req, resp, sizeof resp, &n);
    if (rc == GUBER_OK) {
        k = parse_rows(resp, n, rows, 4);
        if (k != 3 || rows[0].has_error || rows[0].status != 0 || rows[0].limit != 100 || rows[0].remaining != 40 ||
            rows[1].has_error || rows[1].status != 1 || rows[1].limit != 100 || rows[1].remaining != 0 ||      /* drained */
            rows[2].has_error || rows[2].status != 0 || rows[2].limit != 100 || rows[2].remaining != 99) {     /* "n_": a bucket, not an error */
            printf("get_peer_rate_limits: unexpected answer (%d rows: %u/%u %u/%u %u/%u err %u)\n", k, rows[0].status, rows[0].remaining, rows[1].status,
                   rows[1].remaining, rows[2].status, rows[2].remaining, rows[2].has_error);
            rc = GUBER_E_INVALID_ARG;
        }
    }
    /* updatePeerGlobals: a truncated message is turned away whole, the whole one is installed and read back through the peer RPC */
    if (rc == GUBER_OK && guber_wire_pool_update_peer_globals(pool, upd, sizeof upd - 2, &installed) != GUBER_E_WIRE_MALFORMED) rc = GUBER_E_INVALID_ARG;
    if (rc == GUBER_OK && installed != 0) rc = GUBER_E_INVALID_ARG;
    if (rc == GUBER_OK) rc = guber_wire_pool_update_peer_globals(pool, upd, sizeof upd, &installed);
    if (rc == GUBER_OK && installed != 1) rc = GUBER_E_INVALID_ARG;
    if (rc == GUBER_OK) rc = guber_wire_pool_get_peer_rate_limits(pool, rd, sizeof rd, resp, sizeof resp, &n);
    if (rc == GUBER_OK) {
        k = parse_rows(resp, n, rows, 4);
        if (k != 1 || rows[0].has_error || rows[0].status != 0 || rows[0].limit != 9 || rows[0].remaining != 4) {
            printf("update_peer_globals: the installed global reads %d rows: status %u limit %u remaining %u\n", k, rows[0].status, rows[0].limit, rows[0].remaining);
            rc = GUBER_E_INVALID_ARG;
        }
    }
    if (rc != GUBER_OK) printf("peer handlers: %s (%s)\n", guber_strerror(rc), guber_last_error());
    else printf("peer handlers ok\n");
    guber_wire_pool_destroy(pool);
    guber_placement_destroy(place);
    if (eng[1]) guber_engine_destroy(eng[1]);
    if (eng[0]) guber_engine_destroy(eng[0]);
    return rc;
}

int main(int argc, char** argv) {
    const int want_gpu = argc > 1 && !strcmp(argv[1], "--gpu");
    return peer_sequence(want_gpu) == GUBER_OK ? 0 : 1;
}
