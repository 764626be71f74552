// guber_kernels_front_observe.h — what a front sees of its own traffic, reduced on the device (guber_front_observe /
// guber_front_observation / guber_front_rebalance, guber_front.h).  Included by guber_kernels.h behind guber_kernels_front.h.
#pragma once

namespace guber {

// ---- the traffic of a sampled generation, per placement slot and per hot-key candidate -----------------------------------------------
// The reference picks a request's worker from the XXH64 of its HashKey (workers.go:180-184 getWorker); guber_placement generalises that
// to slots plus individually placed hot keys, fitted to OBSERVED traffic — which for a front lies in HBM, at rates no host loop follows.
//   k_fr_observe      a sampled generation, on the routing stream behind its k_fr_count: per request the key as k_fr_count fetches and
//                     hashes it, left out exactly where FR_ENGINE does not consult the hash; per tile of 1 024 requests ONE add per distinct
//                     key on the key's cell of the window's candidate table and ONE add per distinct slot on the slot's word
//   k_fr_observe_top  at a window's end, twice: the cells at or above the threshold, the slot words and the totals to pinned host memory;
//                     then the word the host polls (the kernel boundary between them is the order)
// No workgroup waits for another and none takes a ticket: the order between the steps is the stream's (see route_rank_tile's note).
constexpr uint32_t FO_CELLS = 1u << 16;            // cells of the candidate table (a power of two; 1 MB)
constexpr uint32_t FO_PROBE = 32;                  // a key that finds neither its cell nor a free one this far from home is counted in its slot only
constexpr uint32_t FO_TOP_MAX = 2048;              // candidates a window reports.  The bar is max(1, floor(observed / (engines x 64))): fewer than
                                                   // 2 x engines x 64 keys can reach it (observed / floor(x) < 2 x engines x 64 for x >= 1; below, observed
                                                   // itself is smaller), so with at most 16 engines none is ever left out and the report is deterministic
constexpr uint32_t FO_LDS = 2 * FR_TILE;           // cells of a tile's tables in LDS: at most half full, so a probe always ends
constexpr uint32_t FO_STRIPES = 64;                // the totals, striped by tile: a thousand tiles on one word would queue up behind each other
struct FrObsCell { unsigned long long h; uint32_t c, pad_; };
enum { FO_OBSERVED = 0, FO_SKIPPED = 1, FO_DROPPED = 2 };
struct FrObsTot { unsigned long long w[4]; };      // a stripe of the totals: w[FO_OBSERVED], w[FO_SKIPPED], w[FO_DROPPED], one word of padding
struct FrObs {
    uint32_t n, max_key, key_stride, cmask, no_agg;
    const uint8_t* key_bytes; const uint32_t *key_off, *key_len, *behavior;                   // the generation, as FrIn has it
    uint32_t* slot_w; FrObsCell* cell; FrObsTot* tot;                                         // the window: [n_shards x per], [cmask + 1], [FO_STRIPES]
    RouteRule R;
};

// a key's cell of the window's candidate table takes `cnt` more requests; false: no cell within FO_PROBE of its home
__device__ __forceinline__ bool fo_cell_add(const FrObs& A, unsigned long long h, uint32_t cnt) {
    uint32_t pos = (uint32_t)((h * 0x9E3779B97F4A7C15ull) >> 32) & A.cmask;
    for (uint32_t step = 0; step < FO_PROBE; ++step, pos = (pos + 1u) & A.cmask) {
        // (a look before the atomic: only a key's first tile of a window finds its cell empty)
        unsigned long long t = ld_agent(&A.cell[pos].h);
        if (t == 0ull) { const unsigned long long old = atomicCAS(&A.cell[pos].h, 0ull, h); t = old == 0ull ? h : old; }
        if (t == h) { atomicAdd(&A.cell[pos].c, cnt); return true; }
    }
    return false;
}

// LDS: the tile's keys (2 048 x 12 bytes) and slots (2 048 x 8) = 40 KB + the tile's totals: two workgroups of sixteen waves per CU, which is
// what its wave slots hold anyway.
__global__ __launch_bounds__(FR_TILE) void k_fr_observe(FrObs A) {
    __shared__ unsigned long long kh[FO_LDS];
    __shared__ uint32_t kc[FO_LDS], sk[FO_LDS], sc[FO_LDS], tot[3];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, i = blockIdx.x * FR_TILE + tid;
    for (uint32_t c = tid; c < FO_LDS; c += FR_TILE) { kh[c] = 0ull; kc[c] = 0u; sk[c] = 0u; sc[c] = 0u; }
    if (tid < 3) tot[tid] = 0u;
    __syncthreads();
    bool obs = false;
    unsigned long long h = 0ull;
    if (i < A.n) {
        // k_fr_count's key fetch: the same guess, the same readable end (a packed buffer: 8 bytes past the last key; a row: its key_stride bytes)
        const uint32_t len0 = wave_uniform(A.key_stride ? A.key_len[0] : A.key_off[1] - A.key_off[0]);
        const uint32_t o0 = A.key_stride ? 0u : A.key_off[0], oend = A.key_stride ? 0u : A.key_off[A.n];
        const uint32_t off_g = A.key_stride ? i * A.key_stride : o0 + i * len0;
        uint64_t kw[4] = {0, 0, 0, 0};
        const bool spec = key_fetch_spec(A.key_bytes, off_g, len0, A.key_stride ? (uint64_t)off_g + A.key_stride : (uint64_t)oend + 8, kw);
        const uint32_t off = A.key_stride ? i * A.key_stride : A.key_off[i], len = A.key_stride ? A.key_len[i] : A.key_off[i + 1] - off;
        // FR_ENGINE's conditions, in its order: a GLOBAL request of a rule with a global_engine, an empty key and one above max_key never reach the hash
        if (A.R.global_engine >= 0 && A.behavior && (A.behavior[i] & 2u)) obs = false;
        else obs = len != 0 && len <= A.max_key && A.R.n_shards > 1;
        if (obs) h = (spec && off == off_g && len == len0) ? xxhash64_words4_uniform(kw, len0, 0) : xxhash64(A.key_bytes + off, len, 0);
    }
    const unsigned long long bo = __ballot(obs), bs = __ballot(i < A.n && !obs);
    if (lane == 0) { if (bo) atomicAdd(&tot[0], (uint32_t)__popcll(bo)); if (bs) atomicAdd(&tot[1], (uint32_t)__popcll(bs)); }
    if (obs && (h == 0ull || A.no_agg)) {
        // a hash of 0 is an empty cell's mark (as in the placement's own sketch): the key is counted in its slot only.  no_agg: the laboratory's
        // measure of what the tile's tables are worth — every request goes to the window by itself
        atomicAdd(&A.slot_w[route_slot(A.R, h)], 1u);
        if (h == 0ull || !fo_cell_add(A, h, 1u)) atomicAdd(&tot[2], 1u);
    } else if (obs) {
        for (uint32_t p = (uint32_t)(h >> 20) & (FO_LDS - 1u);; p = (p + 1u) & (FO_LDS - 1u)) {
            unsigned long long t = kh[p];
            if (t == 0ull) { const unsigned long long old = atomicCAS(&kh[p], 0ull, h); t = old == 0ull ? h : old; }
            if (t == h) { atomicAdd(&kc[p], 1u); break; }
        }
    }
    __syncthreads();
    // every distinct key of the tile: one add on its cell; its requests join those of its slot
    for (uint32_t c = tid; c < FO_LDS; c += FR_TILE) {
        const unsigned long long k = kh[c];
        if (k == 0ull) continue;
        const uint32_t cnt = kc[c], slot1 = route_slot(A.R, k) + 1u;
        for (uint32_t p = (slot1 * 0x9E3779B1u) >> 21;; p = (p + 1u) & (FO_LDS - 1u)) {
            uint32_t t = sk[p];
            if (t == 0u) { const uint32_t old = atomicCAS(&sk[p], 0u, slot1); t = old == 0u ? slot1 : old; }
            if (t == slot1) { atomicAdd(&sc[p], cnt); break; }
        }
        if (!fo_cell_add(A, k, cnt)) atomicAdd(&tot[2], cnt);
    }
    __syncthreads();
    // every distinct slot of the tile: one add on its word
    for (uint32_t c = tid; c < FO_LDS; c += FR_TILE) if (sk[c] != 0u) atomicAdd(&A.slot_w[sk[c] - 1u], sc[c]);
    if (tid < 3 && tot[tid] != 0u) atomicAdd(&A.tot[blockIdx.x & (FO_STRIPES - 1u)].w[tid], (unsigned long long)tot[tid]);
}
static_assert((0xffffffffu >> 21) == FO_LDS - 1u, "a slot's home in the tile's table is the top eleven bits of its product");

struct FrObsTop {
    uint32_t cells, n_slots, threshold, seq, phase;
    const FrObsCell* cell; const uint32_t* slot_w; const FrObsTot* tot; uint32_t* n_top;      // the window (n_top: a device word, 0 at its start)
    // pinned host memory: the candidates, compacted (FO_TOP_MAX of each), the slot words, observed / skipped / dropped, and the word the host
    // polls: seq << 32 | candidates (relaxed, system scope: the word carries the number, as FrontHost's do)
    unsigned long long* h_hash; uint32_t* h_count; uint32_t* h_slot_w; unsigned long long* h_tot; unsigned long long* h_word;
};
__global__ __launch_bounds__(256) void k_fr_observe_top(FrObsTop A) {
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
    if (A.phase) {
        // (what phase 0 wrote is in host memory: its kernel has ended)
        if (gid == 0) {
            const uint32_t k = *A.n_top;
            __hip_atomic_store(A.h_word, (unsigned long long)A.seq << 32 | (k < FO_TOP_MAX ? k : FO_TOP_MAX), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    for (uint32_t c = gid; c < A.cells; c += stride) {
        const FrObsCell x = A.cell[c];
        if (x.h == 0ull || x.c < A.threshold) continue;
        const uint32_t k = atomicAdd(A.n_top, 1u);                  // (at most observed / threshold of them, fewer than FO_TOP_MAX: the bar keeps this word quiet)
        if (k < FO_TOP_MAX) { A.h_hash[k] = x.h; A.h_count[k] = x.c; }
    }
    for (uint32_t s = gid; s < A.n_slots; s += stride) A.h_slot_w[s] = A.slot_w[s];
    if (gid < 3) {
        unsigned long long v = 0;
        for (uint32_t q = 0; q < FO_STRIPES; ++q) v += A.tot[q].w[gid];
        A.h_tot[gid] = v;
    }
}

}  // namespace guber
