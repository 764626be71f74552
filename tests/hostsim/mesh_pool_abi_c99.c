/* mesh_pool_abi_c99.c — TEST-ONLY: the calls go/wire_server.go's MeshWireServer makes (NewMeshWireServer, getRateLimitsMeshRaw, Close) and the
 * set-up a daemon does around them, compiled as C99 against the two public headers and run on the GPU by tests/test_gpu_mesh_pool.py: two
 * logical ranks of device 0 (an engine and a front each), the ring of their addresses, the mesh, the payload stage over it; one serialized
 * GetRateLimitsReq of three requests (a, b, a: limit 2) handed to rank 0 and then to rank 1, the GetRateLimitsResp bytes checked field by
 * field — with metadata{"owner": <address>} exactly on the answers whose key the ring (guber_ring_route) gives to the other rank. */
#include <stdio.h>
#include <string.h>

#include "guber_gpu.h"
#include "guber_wire.h"

static const char* const ADDR[2] = {"gpu0:8080", "gpu1:8080"};

/* one RateLimitResp as both protobuf runtimes write it: status, limit, remaining (zero fields are not written), reset_time 1700000060000,
 * and the owner's metadata entry behind field 5's place when another rank owns the key */
static size_t put_answer(uint8_t* out, unsigned status, unsigned remaining, uint32_t owner, uint32_t rank) {
    static const uint8_t reset[] = {0x20, 0xe0, 0xa4, 0x99, 0xff, 0xbc, 0x31};
    uint8_t body[64];
    size_t b = 0, alen = strlen(ADDR[owner]);
    if (status) { body[b++] = 0x08; body[b++] = (uint8_t)status; }
    body[b++] = 0x10; body[b++] = 2;
    if (remaining) { body[b++] = 0x18; body[b++] = (uint8_t)remaining; }
    memcpy(body + b, reset, sizeof reset); b += sizeof reset;
    if (owner != rank) {
        body[b++] = 0x32; body[b++] = (uint8_t)(2 + 5 + 2 + alen);
        body[b++] = 0x0a; body[b++] = 5; memcpy(body + b, "owner", 5); b += 5;
        body[b++] = 0x12; body[b++] = (uint8_t)alen; memcpy(body + b, ADDR[owner], alen); b += alen;
    }
    out[0] = 0x0a; out[1] = (uint8_t)b;
    memcpy(out + 2, body, b);
    return 2 + b;
}

int main(void) {
    /* RateLimitReq{name "n", unique_key "a"|"b", hits 1, limit 2, duration 60000}: 0a <len> { 0a 01 6e  12 01 61  18 01  20 02  28 e0 d4 03 } */
    static const uint8_t req[] = {0x0a, 14, 0x0a, 1, 'n', 0x12, 1, 'a', 0x18, 1, 0x20, 2, 0x28, 0xe0, 0xd4, 0x03,
                                  0x0a, 14, 0x0a, 1, 'n', 0x12, 1, 'b', 0x18, 1, 0x20, 2, 0x28, 0xe0, 0xd4, 0x03,
                                  0x0a, 14, 0x0a, 1, 'n', 0x12, 1, 'a', 0x18, 1, 0x20, 2, 0x28, 0xe0, 0xd4, 0x03};
    static const uint8_t keys[] = {'n', '_', 'a', 'n', '_', 'b', 0, 0, 0, 0, 0, 0, 0, 0};
    static const uint32_t key_off[] = {0, 3, 6};
    guber_config_t cfg;
    guber_engine_t* eng[2] = {NULL, NULL};
    guber_front_t* front[2] = {NULL, NULL};
    guber_ring_t* ring = NULL;
    guber_mesh_t* mesh = NULL;
    guber_wire_mesh_pool_t* pool = NULL;
    guber_wire_mesh_pool_config_t wc;
    guber_wire_mesh_pool_stats_t st;
    uint32_t owner[2] = {0, 0}, rank, next = 0;
    uint8_t resp[4096], want[256];
    size_t n = 0, bound, w;
    int rc = GUBER_OK, r;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = (uint32_t)sizeof cfg; cfg.cache_size = 1000; cfg.max_batch = 1024;
    for (r = 0; r < 2 && rc == GUBER_OK; ++r) {
        rc = guber_engine_create(&cfg, &eng[r]);
        if (rc == GUBER_OK) rc = guber_front_create(&eng[r], 1, NULL, 1024, 0, &front[r]);
    }
    if (rc == GUBER_OK) rc = guber_ring_create(ADDR, 2, 512, 0, &ring);
    if (rc == GUBER_OK) rc = guber_ring_route(ring, keys, key_off, 2, owner);
    if (rc == GUBER_OK) rc = guber_mesh_create_local(front, 2, ring, 1024, &mesh);
    /* NewMeshWireServer */
    memset(&wc, 0, sizeof wc);
    wc.sets = 2; wc.max_items = 1024; wc.max_payload_bytes = 1u << 16; wc.max_rpcs = 8; wc.wrap_errors = 1;
    if (rc == GUBER_OK) rc = guber_wire_mesh_pool_create(mesh, ADDR, &wc, &pool);
    if (rc == GUBER_OK) rc = guber_wire_mesh_pool_set_clock(pool, 1700000000000LL);
    /* getRateLimitsMeshRaw, twice: rank = a counter modulo the ranks */
    for (r = 0; r < 2 && rc == GUBER_OK; ++r) {
        rank = next++ % 2u;
        bound = guber_wire_mesh_pool_response_bound(pool, req, sizeof req);
        if (bound == 0 || bound > sizeof resp) rc = GUBER_E_NOMEM;
        if (rc == GUBER_OK) rc = guber_wire_mesh_pool_get_rate_limits(pool, rank, req, sizeof req, resp, bound, &n);
        if (rc != GUBER_OK) break;
        /* first RPC: a 1 left, b 1 left, a 0 left; second: a OVER_LIMIT, b 0 left, a OVER_LIMIT */
        w = 0;
        w += put_answer(want + w, r ? 1u : 0u, r ? 0u : 1u, owner[0], rank);
        w += put_answer(want + w, 0u, r ? 0u : 1u, owner[1], rank);
        w += put_answer(want + w, r ? 1u : 0u, 0u, owner[0], rank);
        if (n != w || memcmp(resp, want, n) != 0) {
            size_t i;
            printf("mesh pool: unexpected response at rank %u (%u bytes, %u expected):", (unsigned)rank, (unsigned)n, (unsigned)w);
            for (i = 0; i < n; ++i) printf(" %02x", resp[i]);
            printf("\n");
            rc = GUBER_E_INVALID_ARG;
        }
    }
    if (rc == GUBER_OK) rc = guber_wire_mesh_pool_stats(pool, &st);
    if (rc == GUBER_OK && (st.rpcs != 2 || st.items != 6 || st.sets != 2 || st.host_rpcs != 0 ||
                           st.forwarded != (uint64_t)(2 * (owner[0] != 0) + (owner[1] != 0) + 2 * (owner[0] != 1) + (owner[1] != 1)))) {
        printf("mesh pool: unexpected statistics (rpcs %llu items %llu sets %llu forwarded %llu)\n", (unsigned long long)st.rpcs, (unsigned long long)st.items,
               (unsigned long long)st.sets, (unsigned long long)st.forwarded);
        rc = GUBER_E_INVALID_ARG;
    }
    if (rc != GUBER_OK) printf("mesh pool: %s (%s)\n", guber_strerror(rc), guber_last_error());
    /* Close */
    guber_wire_mesh_pool_destroy(pool);
    guber_mesh_destroy(mesh);
    guber_ring_destroy(ring);
    for (r = 1; r >= 0; --r) {
        if (front[r]) guber_front_destroy(front[r]);
        if (eng[r]) guber_engine_destroy(eng[r]);
    }
    if (rc == GUBER_OK) printf("MESH POOL ABI C99 OK\n");
    return rc == GUBER_OK ? 0 : 1;
}
