// guber_kernels_front_store.h — the Store side channel of a generation routed on the device (guber_front_probe_missing_dev /
// guber_front_eval_store_dev, guber_front.h).  Included by guber_kernels.h behind guber_kernels_front.h, whose FrIn / FrTile it uses.
#pragma once

namespace guber {

// ---- which Store.Get calls are due, and where a generation must be cut --------------------------------------------------------
// Config.Store (store.go:49-65): the reference asks Store.Get on every cache miss (algorithms.go:45-51, :274-280) and a token
// RESET_REMAINING removes the item from cache and store (algorithms.go:78-90), so the key's next request misses again.  For a
// generation that k_fr_count / k_fr_scan / k_fr_scatter have routed (er[i] = engine << 10 | rank), on the routing stream behind them:
//   k_fr_elect     per request: the key's cell in an insert-only, open-addressed election table (tag = XXH64 of the key under the first
//                  engine's hash_mask, with the engine the request was routed to folded in: a key's Behavior_GLOBAL requests live in
//                  another table and are another identity); first = the smallest index among the cell's requests, first_reset = the
//                  smallest among those that carry Behavior_RESET_REMAINING
//   k_fr_missing   per request: its key's BYTES (and engine) against those of requests `first` and `first_reset` — a mismatch is two
//                  identities in one cell: the generation's `collision` word goes up and the host decides from the keys themselves;
//                  otherwise the request that IS `first` probes its engine's table read-only (probe() and k_probe_missing's predicate)
//                  and raises its ask flag, and a request behind its cell's first_reset lowers cut_at to itself
//   k_fr_ask       twice: per tile of 1 024 requests the ballot count of the ask flags below cut_at; then every tile adds up the counts
//                  of the tiles before it (at most 1 024: one per thread) and writes its flagged requests, in order, to index[] / engine[]
// No workgroup waits for another and none takes a ticket: the order between the steps is the stream's.
constexpr uint32_t FR_STORE_MAX_N = 1u << 20;        // requests per store generation (k_fr_ask: one thread per tile of the tiles before)
constexpr uint32_t FR_NONE = 0xffffffffu;
struct FrStoreTabs { Table t[MULTI_MEM_MAX]; };      // the engines' tables as they are under the engines' locks: one argument block in HBM
struct FrStoreCtl { uint32_t cut_at, collision, n_ask, pad_; };
struct FrStore {
    unsigned long long* tag; uint32_t *first, *first_reset; uint32_t cmask;   // the election table: cleared per generation (tag 0, first / first_reset FR_NONE)
    uint64_t hash_mask;                                                        // the first engine's Table::hash_mask (GUBER_FLAG_TEST_WEAK_HASH reaches the election)
    uint32_t* cell;                                                            // [n] where request i's key was elected
    const FrStoreTabs* tabs; int64_t now;
    uint8_t* ask;                                                              // [n] 1: Store.Get is due for request i (before the cut is applied)
    FrStoreCtl* ctl; uint32_t* tile_cnt;                                       // [tiles]
    uint32_t* index; uint8_t* engine; uint32_t cap;                            // the ask list, ascending
    uint32_t all;                                                              // k_fr_missing: every request reads its residency (the host decides the rest)
};
static_assert(sizeof(FrIn) + sizeof(FrStore) <= 4096, "kernel arguments are limited to 4 KB");

__device__ __forceinline__ uint32_t fr_store_home(unsigned long long tag) {
    const unsigned long long m = tag * 0x9E3779B97F4A7C15ull;     // (a weak hash keeps six bits: spread them and the engine over the table)
    return (uint32_t)(m >> 32);
}

__global__ __launch_bounds__(256) void k_fr_elect(FrIn A, FrStore E) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    const uint32_t e = A.M.er[i] >> FR_RANK_BITS;
    const uint32_t off = fr_key_off(A, i), len = fr_key_len(A, i, off);
    const unsigned long long h = (xxhash64(A.key_bytes + off, len, 0) & E.hash_mask) ^ ((unsigned long long)(e + 1u) << 56);
    const unsigned long long tag = h ? h : 1ull;
    const bool reset = A.behavior && (A.behavior[i] & 8u);       // Behavior_RESET_REMAINING, whatever the algorithm
    uint32_t pos = fr_store_home(tag) & E.cmask, at = FR_NONE;
    // (at most n tags in >= 2 n cells: an empty or matching cell is met before the table has gone round)
    for (uint32_t step = 0; step <= E.cmask; ++step, pos = (pos + 1u) & E.cmask) {
        unsigned long long t = ld_agent(&E.tag[pos]);
        if (t == 0ull) { const unsigned long long old = atomicCAS(&E.tag[pos], 0ull, tag); t = old == 0ull ? tag : old; }
        if (t == tag) { at = pos; break; }
    }
    E.cell[i] = at;
    if (at == FR_NONE) { atomicExch(&E.ctl->collision, 1u); return; }   // (cannot happen; the host then decides from the keys)
    // (a look before the atomic: a hot key's requests arrive in roughly ascending order, so all but the first few find a smaller index there —
    //  without it a key that takes a quarter of a generation of 40 000 kept one word busy for 120 us, measured)
    if (__hip_atomic_load(&E.first[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > i) atomicMin(&E.first[at], i);
    if (reset && __hip_atomic_load(&E.first_reset[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > i) atomicMin(&E.first_reset[at], i);
}

// request i's key and engine against request q's
__device__ __forceinline__ bool fr_same_key(const FrIn& A, uint32_t e, const uint8_t* key, uint32_t len, uint32_t q) {
    if ((uint32_t)(A.M.er[q] >> FR_RANK_BITS) != e) return false;
    const uint32_t qoff = fr_key_off(A, q);
    if (fr_key_len(A, q, qoff) != len) return false;
    const uint8_t* other = A.key_bytes + qoff;
    uint32_t b = 0;
    for (; b + 8u <= len; b += 8u) if (ld_key_word(key + b) != ld_key_word(other + b)) return false;
    for (; b < len; ++b) if (key[b] != other[b]) return false;
    return true;
}

__global__ __launch_bounds__(256) void k_fr_missing(FrIn A, FrStore E) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    const uint32_t e = A.M.er[i] >> FR_RANK_BITS;
    const uint32_t off = fr_key_off(A, i), len = fr_key_len(A, i, off);
    const uint8_t* key = A.key_bytes + off;
    bool look = E.all != 0u;
    if (!look) {
        const uint32_t at = E.cell[i];
        if (at == FR_NONE) { E.ask[i] = 0; return; }
        const uint32_t first = E.first[at], fres = E.first_reset[at];
        bool same = first <= i && (first == i || fr_same_key(A, e, key, len, first));
        if (same && fres != FR_NONE && fres != i && fres != first) same = fres < A.n && fr_same_key(A, e, key, len, fres);
        if (!same) { if (__hip_atomic_load(&E.ctl->collision, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) atomicExch(&E.ctl->collision, 1u); E.ask[i] = 0; return; }
        if (fres < i) atomicMin(&E.ctl->cut_at, i);
        look = first == i;
    }
    uint8_t m = 0;
    if (look && len != 0u) {                                      // (an empty key is never asked for; one longer than max_key_bytes is, as k_probe_missing reports it)
        const Table& T = E.tabs->t[e];
        m = 1;
        if (len <= T.max_key) {
            uint32_t slot = 0;
            const uint32_t pr = probe(T, key, len, xxhash64(key, len, 0), false, slot);
            if (pr & PR_FOUND) {
                const Rec s = T.buckets[slot].rec;
                m = (rec_kind(s) == K_ABSENT || rec_expired(s, E.now)) ? 1 : 0;
            }
        }
    }
    E.ask[i] = m;
}

// write = 0: tile_cnt[tile] = the tile's flagged requests below cut_at.  write = 1: the same ballots again, the tile's place from the
// counts of the tiles before it (thread t adds tile t's: n <= FR_STORE_MAX_N makes that at most one per thread), the list entries, and
// the last tile leaves the list's length.
__global__ __launch_bounds__(FR_TILE) void k_fr_ask(FrStore E, const uint16_t* er, uint32_t n, uint32_t write) {
    __shared__ uint32_t wcnt[FR_TILE / 64], wsum[FR_TILE / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, tile = blockIdx.x, i = tile * FR_TILE + tid;
    const uint32_t cut = E.ctl->cut_at;
    const bool flag = i < n && i < cut && E.ask[i] != 0;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(b);
    const uint32_t before = (write && tid < tile) ? E.tile_cnt[tid] : 0u;
    const uint32_t ws = (uint32_t)wave_sum((int)before);
    if (lane == 0) wsum[wave] = ws;
    __syncthreads();
    uint32_t total = 0, mine = 0, base = 0;
    for (uint32_t w = 0; w < FR_TILE / 64; ++w) { total += wcnt[w]; mine += w < wave ? wcnt[w] : 0u; base += wsum[w]; }
    if (!write) { if (tid == 0) E.tile_cnt[tile] = total; return; }
    if (flag) {
        const uint32_t k = base + mine + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (k < E.cap) { E.index[k] = i; E.engine[k] = (uint8_t)(er[i] >> FR_RANK_BITS); }
    }
    if (tile == gridDim.x - 1u && tid == 0) E.ctl->n_ask = base + total;
}

// ---- the answers' last hop of a store generation ------------------------------------------------------------------------------
// What k_fr_out does, with the side channel: fr_out_tile<true> (guber_kernels_front.h).
struct FrOutStore { FrOut O; FrOutSide X; };
__global__ __launch_bounds__(256) void k_fr_out_store(FrOutStore S) { fr_out_tile<true>(S.O, S.X); }

}  // namespace guber
