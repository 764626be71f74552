// guber_kernels_front.h — the device-resident front of a GPU's logical shards (guber_front_*, guber_front.h).
// Included by guber_kernels.h (and, like the batch pipelines, compiled for the host by the tests' fiber emulation).
#pragma once

namespace guber {

// ---- one generation of requests in ARRIVAL order -> the shards' shares -> the answers in ARRIVAL order --------------------------
// What the reference does per request — WorkerPool.GetRateLimit picks the worker from the XXH64 of the HashKey (workers.go:261-289,
// getWorker :180-184) and GetRateLimits answers in request order (gubernator.proto:51-54, gubernator.go:203-300) — done for a whole
// generation of requests that already lie in HBM:
//   k_fr_count    per request: XXH64 of the key, the placement's rule -> engine, its rank among the tile's requests of that engine
//                 (stable: arrival order); per tile of 1 024 requests the requests per engine
//   k_fr_scan     one workgroup: where every tile's part of every share starts; places the shares (base[engine]), hands the shares'
//                 sizes to the host and releases the flag it polls
//   k_fr_scatter  request i -> place d = base[engine] + tile_base + rank of the mirror: every engine's share is
//                 contiguous and in arrival order (requests of one key keep their order), the fused pipelines run on the shares as
//                 on any batch; fwd[i] = d.  The tile is put into the shares' order in LDS first (the place there is computed:
//                 lbase[engine] + rank), so consecutive threads store consecutive d of a run.  Keys of ONE width (<= 32 bytes:
//                 every front end that formats its keys) travel with their requests as 8-byte words through the same LDS —
//                 share j's keys are packed, key d at d x width (no offsets are written: BatchView::key_width says it), so k_part's
//                 speculative key fetch applies without loading any —
//                 other keys stay where they are and the share carries offset + length (BatchView.key_len)
//   k_fr_out      the same, mirrored: consecutive threads load consecutive share answers of a run, LDS, answer i from the place
//                 er[i] gives: coalesced reads in the shares' order, coalesced writes in arrival order (fwd is not read)
constexpr uint32_t FR_PER = 4;                     // requests per thread of the copy kernels
constexpr uint32_t FR_TILE = 256 * FR_PER;         // requests per tile
constexpr uint32_t FR_RANK_BITS = 10;              // er[i] = engine << 10 | rank among the tile's requests of that engine
static_assert((1u << FR_RANK_BITS) >= FR_TILE && (MULTI_MEM_MAX << FR_RANK_BITS) <= 65536, "engine and rank share sixteen bits");
constexpr uint32_t FR_SCAN_T = 1024;               // threads of k_fr_scan's workgroups
constexpr uint32_t FR_SCAN_PER = 4;                // tiles per thread, at most
constexpr uint32_t FR_MAX_N = FR_SCAN_T * FR_SCAN_PER * FR_TILE;   // 4 194 304 requests per generation
constexpr uint32_t FR_KEY_COPY_MAX = 32;           // keys of one width up to this many bytes are copied into the shares

struct FrontCtl {                                   // per slot, device memory, zeroed once
    uint32_t tot[MULTI_MEM_MAX];                    // the shares' sizes (a share starts where the shares before it end)
    uint32_t ragged_seq;                            // == seq of the generation: its keys are not of one width (or wider than FR_KEY_COPY_MAX)
    uint32_t pad_[15];
};
// device-visible host memory, one per slot: every word carries the generation's seq in its upper half, so the host needs no fence on the
// device's side to know a word is this generation's (a system-scope release makes the workgroup write back its XCD's whole L2 first:
// measured 66 - 100 us in k_fr_scan behind a generation's kernels); w[k] = seq << 32 | size of engine k's share, w[16] = seq << 32 |
// ragged << 8 | min(key width, 255)
struct FrontHost { unsigned long long w[MULTI_MEM_MAX + 1]; unsigned long long pad_[15]; };
static_assert(sizeof(FrontHost) == 256, "four lines of pinned memory per slot");

// the routing scratch of a slot (or of a mesh's rank): what count, scan, place and report share.  Carved in one place (route_carve,
// guber_front.h) and handed from the routing's arguments to the last hop's in one assignment.
struct RouteMap {
    uint16_t* er;                                   // [n] destination << FR_RANK_BITS | rank among the tile's requests of that destination
    uint32_t *tile_cnt, *tile_base;                 // [tiles][MULTI_MEM_MAX] a tile's requests per destination; where its run starts in the share
    FrontCtl* ctl; FrontHost* host;
};

struct FrIn {
    uint32_t n, n_engines, max_key, seq;
    // the generation as the caller holds it (HBM, arrival order); burst / created_at / is_owner may be null
    const uint8_t* key_bytes; const uint32_t* key_off;
    // keys as rows instead (the device wire decoder's output): key i = key_bytes + i * key_stride, key_len[i] bytes; key_stride a multiple of 8
    uint32_t key_stride; const uint32_t* key_len;
    const int64_t *hits, *limit, *duration, *burst, *created_at; const uint32_t* behavior; const uint8_t *algorithm, *is_owner;
    RouteMap M;                                     // scratch of the slot
    // the mirror: the shares, engine after engine (d_key_off / d_key_len are written for a ragged generation only — a packed one's pieces carry
    // BatchView::key_width; d_fwd is null unless the answers' last hop is k_wire_enc, its one reader)
    uint32_t *d_key_off, *d_key_len, *d_fwd; int64_t *d_hits, *d_limit, *d_duration, *d_burst, *d_created_at; uint32_t* d_behavior; uint8_t *d_algorithm, *d_is_owner;
    uint8_t* d_keys;
    RouteRule R;
};
static_assert(sizeof(FrIn) <= 4096, "kernel arguments are limited to 4 KB");
__device__ __forceinline__ uint32_t fr_key_off(const FrIn& A, uint32_t i) { return A.key_stride ? i * A.key_stride : A.key_off[i]; }
__device__ __forceinline__ uint32_t fr_key_len(const FrIn& A, uint32_t i, uint32_t off) { return A.key_stride ? A.key_len[i] : A.key_off[i + 1] - off; }
// the width the generation's keys have if they all have one (the first key's), and where its keys end
__device__ __forceinline__ uint32_t fr_len0(const FrIn& A) { return A.key_stride ? A.key_len[0] : A.key_off[1] - A.key_off[0]; }

// No workgroup waits for another and none takes a ticket: the order between the three steps is the stream's (a device-scope ticket per
// workgroup was 25 ns each, one after the other: 50 us for a generation of 2 048 tiles, and the scans ran behind it — round 6's first form
// took 157 us for 524 288 requests with nothing else on the GPU).
// A tile is FR_TILE = 1 024 requests (round 6's second form; the first had 256): a generation has a quarter of the tiles and scan
// steps, and the runs the copy kernels move (a tile's requests of one engine, consecutive in the share) are four times as long — about
// 85 elements with twelve engines.  k_fr_scatter / k_fr_out take four requests per thread (request k of thread t: tile x 1024 + k x 256 + t
// on the arrival side, sorted element k x 256 + t on the shares' side — both coalesced; see "the copy kernels" below).

// ---- the routing core: what the front (k_fr_*) and the mesh of fronts (k_mx_*, guber_kernels_mesh.h) share ----------------------------
// Both sort a generation by destination — an engine here, a rank there — in the same steps: a stable rank per request and the counts per
// tile (route_rank_tile), the scan of the tiles' counts and the totals' way to the host (route_scan), the tile's order in LDS (FrTile,
// fr_place, fr_sorted_places below).  A kernel of either keeps what is its own: how a destination is found, what is moved.

// The tail of a count kernel, a workgroup of FR_TILE threads, thread `tid` with request i = tile x FR_TILE + tid of n and its destination e
// (0xff behind the generation's end): er[i] = e << FR_RANK_BITS | the request's rank among the tile's requests of e, in arrival order
// (stable), and tile_cnt[tile][*].  Two barriers: the workgroup meets at the call, and between the waves' totals and their sums.
// The lanes of the wave that go to the same destination: four ballots (one per bit of its number) instead of one per destination; a
// lane's rank among them follows the arrival order, the group's first lane leaves the group's size.  Lanes behind the generation's end
// carry 0xff, whose four low bits are destination 15's: they are in nobody's group, or 15's count in the generation's last wave would
// include them.
__device__ __forceinline__ void route_rank_tile(uint32_t e, const RouteMap& M, uint32_t i, uint32_t n) {
    __shared__ uint32_t wtot[FR_TILE / 64][MULTI_MEM_MAX];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid < (FR_TILE / 64) * MULTI_MEM_MAX) (&wtot[0][0])[tid] = 0u;
    __syncthreads();
    unsigned long long same = __ballot(e <= 15u);
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) { const unsigned long long m = __ballot((e >> b) & 1u); same &= ((e >> b) & 1u) ? m : ~m; }
    if (e > 15u) same = 0ull;                                        // (lanes behind the generation's end)
    uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    if (same && rank == 0) wtot[wave][e] = (uint32_t)__popcll(same);
    __syncthreads();
    if (i < n) {
        for (uint32_t w = 0; w < wave; ++w) rank += wtot[w][e];
        M.er[i] = (uint16_t)(e << FR_RANK_BITS | rank);
    }
    if (tid < MULTI_MEM_MAX) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < FR_TILE / 64; ++w) c += wtot[w][tid];
        M.tile_cnt[blockIdx.x * MULTI_MEM_MAX + tid] = c;
    }
}

// The scan kernel's body.  FOUR workgroups of FR_SCAN_T threads, one per four destinations (one 16-byte word of a tile's counts): the
// exclusive scan of the tiles' counts (thread t takes `per` consecutive tiles of nt) and the shares' sizes, which go to ctl->tot and to
// the host: it polls for words of this `seq` (relaxed, system scope: the word carries the number, the host needs no fence from the device
// — FrontHost).  The shares' places are the prefix over the destinations, which every workgroup of the copy kernels adds up for itself
// (sixteen numbers).
// A dozen live registers, no scratch: with all sixteen destinations in registers and the tile loops unrolled the compiler spilled 250
// registers, and a kernel with 1 MB of scratch cost the queue 80 us (measured).
__device__ __forceinline__ void route_scan(const RouteMap& M, uint32_t seq, uint32_t nt, uint32_t per) {
    __shared__ uint32_t wsum[FR_SCAN_T / 64][4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, q = blockIdx.x;
    const uint32_t t0 = tid * per, t1 = t0 + per < nt ? t0 + per : nt;
    uint32_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) { const uint4 v = ((const uint4*)(M.tile_cnt + (size_t)t * MULTI_MEM_MAX))[q]; m0 += v.x; m1 += v.y; m2 += v.z; m3 += v.w; }
    const uint32_t i0 = (uint32_t)wave_incl_scan_i32((int)m0), i1 = (uint32_t)wave_incl_scan_i32((int)m1);
    const uint32_t i2 = (uint32_t)wave_incl_scan_i32((int)m2), i3 = (uint32_t)wave_incl_scan_i32((int)m3);
    if (lane == 63) { wsum[wave][0] = i0; wsum[wave][1] = i1; wsum[wave][2] = i2; wsum[wave][3] = i3; }
    __syncthreads();
    uint32_t e0 = i0 - m0, e1 = i1 - m1, e2 = i2 - m2, e3 = i3 - m3;
    for (uint32_t w = 0; w < wave; ++w) { e0 += wsum[w][0]; e1 += wsum[w][1]; e2 += wsum[w][2]; e3 += wsum[w][3]; }
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) {
        const uint4 v = ((const uint4*)(M.tile_cnt + (size_t)t * MULTI_MEM_MAX))[q];
        ((uint4*)(M.tile_base + (size_t)t * MULTI_MEM_MAX))[q] = make_uint4(e0, e1, e2, e3);
        e0 += v.x; e1 += v.y; e2 += v.z; e3 += v.w;
    }
    if (tid < 4) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < FR_SCAN_T / 64; ++w) all += wsum[w][tid];
        M.ctl->tot[4 * q + tid] = all;
        __hip_atomic_store(&M.host->w[4 * q + tid], (unsigned long long)seq << 32 | all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The front's rule for one request, k_fr_count's and k_mx_small's (guber_kernels_small.h) alike, in ONE place.  A macro, not a function:
// k_fr_count's instruction stream is part of what the benchmark measures, and the statements below are the ones it has always had — a
// function taking the hash as a callable compiled to another stream.  E = the engine of request I with a key of LEN bytes (HASH: the
// expression of its XXH64, evaluated only when the rule looks at it).  A key no engine takes (empty, above MAX_KEY) goes to engine 0
// and earns its item error there.
#define FR_ENGINE(E, R, N_ENGINES, MAX_KEY, BEHAVIOR, I, LEN, HASH)                                                                         \
    E = 0;                                                                                                                                  \
    if ((R).global_engine >= 0 && (BEHAVIOR) && ((BEHAVIOR)[I] & 2u)) E = (uint32_t)(R).global_engine;   /* Behavior_GLOBAL: the device's GLOBAL engine */ \
    else if ((LEN) != 0 && (LEN) <= (MAX_KEY) && (R).n_shards > 1) E = route_engine((R), (HASH));                                           \
    if (E >= (N_ENGINES)) E = 0;

__global__ __launch_bounds__(FR_TILE) void k_fr_count(FrIn A) {
    // one request per thread, 1 024 threads: the chain offsets -> key -> hot-key list -> slot table is four dependent trips, and what hides
    // them is waves in flight (four requests per thread, a quarter of the waves: 24 us instead of 20 for a million requests)
    const uint32_t i = blockIdx.x * FR_TILE + threadIdx.x;
    uint32_t e = 0xffu;
    if (i < A.n) {
        // keys of one width: the key's words are requested at the place the first two offsets suggest, together with the request's own
        // offsets, and used if those confirm the guess (key_fetch_spec, guber_table.h, as k_part does: one dependent trip less, and only
        // the words a key of that width has)
        // (keys as rows: a row's place is known, its length is the guess; a row is readable to its end, key_stride bytes)
        const uint32_t len0 = wave_uniform(fr_len0(A));
        const uint32_t o0 = A.key_stride ? 0u : A.key_off[0], oend = A.key_stride ? 0u : A.key_off[A.n];
        const uint32_t off_g = A.key_stride ? i * A.key_stride : o0 + i * len0;
        uint64_t kw[4] = {0, 0, 0, 0};
        // (a packed buffer is readable 8 bytes past the last key; of a row, its key_stride bytes)
        const bool spec = key_fetch_spec(A.key_bytes, off_g, len0, A.key_stride ? (uint64_t)off_g + A.key_stride : (uint64_t)oend + 8, kw);
        const uint32_t off = fr_key_off(A, i), len = fr_key_len(A, i, off);
        // (the hash is not handed on to k_part: a column for it costs the copy kernels 32 B per request, measured -2 % on the routed rate with
        //  k_part hashing less — the pipeline is closer to its transactions than to its instructions: profiles/r06_pass_hash_ab.txt)
        FR_ENGINE(e, A.R, A.n_engines, A.max_key, A.behavior, i, len,
                  (spec && off == off_g && len == len0) ? xxhash64_words4_uniform(kw, len0, 0) : xxhash64(A.key_bytes + off, len, 0))
        if (len != len0 || off != off_g || len0 == 0 || len0 > FR_KEY_COPY_MAX) {
            if (__hip_atomic_load(&A.M.ctl->ragged_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != A.seq) atomicExch(&A.M.ctl->ragged_seq, A.seq);
        }
    }
    route_rank_tile(e, A.M, i, A.n);
}

// route_scan, and the front's own word: whether the generation's keys are of one width, and which
__global__ __launch_bounds__(FR_SCAN_T) void k_fr_scan(FrIn A, uint32_t nt, uint32_t per) {
    route_scan(A.M, A.seq, nt, per);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t ragged = __hip_atomic_load(&A.M.ctl->ragged_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == A.seq ? 1u : 0u;
        const uint32_t len0 = fr_len0(A);
        __hip_atomic_store(&A.M.host->w[MULTI_MEM_MAX], (unsigned long long)A.seq << 32 | ragged << 8 | (len0 < 255u ? len0 : 255u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- the copy kernels: a tile is put into the shares' order in LDS, so that consecutive threads move consecutive elements of a run ------
// A tile's requests of engine e are one RUN of the share: tile_cnt[tile][e] consecutive places from sbase[e] + tile_base[tile][e], in
// arrival order.  Sorted by engine (stable), the tile's request i = (e, rank) has the local place p = lbase[e] + rank — lbase the exclusive
// prefix of the tile's sixteen counts: computed, never searched for — and sorted element j lies at d = dofs[e] + j of the mirror, dofs[e] =
// sbase[e] + tile_base[tile][e] - lbase[e].  A column goes through LDS: arrival order on the side of the caller's arrays (thread t:
// t, t + 256, ... — coalesced), sorted order on the side of the shares (thread t: sorted elements t, t + 256, ... — consecutive d inside a
// run: a wave's access covers whole sectors except at the ends of the dozen runs it touches; before, lane by lane in arrival order, every
// access of every column fell into a dozen runs of about five elements each).
struct FrTile { uint32_t lbase[MULTI_MEM_MAX + 1], dofs[MULTI_MEM_MAX]; };
// sixteen threads: the places of the shares (the prefix over the shares' sizes) and of the tile's runs; the workgroup meets behind it
__device__ __forceinline__ void fr_tile_bases(FrTile& T, const RouteMap& M, uint32_t tile) {
    const uint32_t e = threadIdx.x;
    if (e < MULTI_MEM_MAX) {
        const uint32_t* cnt = M.tile_cnt + (size_t)tile * MULTI_MEM_MAX;
        uint32_t s = 0, l = 0;
        for (uint32_t k = 0; k < e; ++k) { s += M.ctl->tot[k]; l += cnt[k]; }
        T.lbase[e] = l; T.dofs[e] = s + M.tile_base[(size_t)tile * MULTI_MEM_MAX + e] - l;
        if (e == MULTI_MEM_MAX - 1) T.lbase[MULTI_MEM_MAX] = l + cnt[e];
    }
    __syncthreads();
}
// the tile-local place of a request, er = its engine << FR_RANK_BITS | rank (0xffffffff: no place in the tile — cannot happen, the ranks
// are a permutation; nothing is accessed out of bounds)
__device__ __forceinline__ uint32_t fr_place(const FrTile& T, uint32_t er) {
    const uint32_t p = T.lbase[er >> FR_RANK_BITS] + (er & ((1u << FR_RANK_BITS) - 1u));
    return p < FR_TILE ? p : 0xffffffffu;
}
// the engine of sorted element j < lbase[16]: the LAST one whose run starts at or before j (engines without requests in the tile have
// the lbase of their successor: counting the starts <= j steps over them) — fifteen compares, no loop over memory
__device__ __forceinline__ uint32_t fr_engine_of(const FrTile& T, uint32_t j) {
    uint32_t e = 0;
#pragma unroll
    for (uint32_t q = 1; q < MULTI_MEM_MAX; ++q) e += T.lbase[q] <= j ? 1u : 0u;
    return e;
}
// the mirror's place of the thread's sorted elements (0xffffffff: behind the tile's last request)
__device__ __forceinline__ void fr_sorted_places(const FrTile& T, uint32_t n, uint32_t (&dd)[FR_PER]) {
    const uint32_t cnt = T.lbase[MULTI_MEM_MAX] < FR_TILE ? T.lbase[MULTI_MEM_MAX] : FR_TILE;
#pragma unroll
    for (int k = 0; k < FR_PER; ++k) {
        const uint32_t j = threadIdx.x + k * 256u, d = T.dofs[fr_engine_of(T, j)] + j;
        dd[k] = j < cnt && d < n ? d : 0xffffffffu;                  // (d >= n cannot happen: the ranks are a permutation; nothing is accessed out of bounds)
    }
}

// LDS: two buffers of 1 024 x 8 bytes taken in turn, one column at a time (a barrier per column: a buffer is written again two columns
// later, behind the barrier of the column between) + FrTile = 16 520 bytes — nine workgroups would fit a CU's 160 KB; the 80 registers
// (no scratch) leave six of four waves each.  All columns at once (up to 11 x 8 KB) would leave one.
// Measured under the bench's load (one kernel trace each, same box): 63.4 -> 41.9 us per 1 048 576 requests (profiles/front_runs_ab.txt).
__global__ __launch_bounds__(256) void k_fr_scatter(FrIn A) {
    __shared__ FrTile T;
    __shared__ uint64_t stg[2][FR_TILE];
    const uint32_t tile = blockIdx.x, tid = threadIdx.x, i0 = tile * FR_TILE + tid;
    fr_tile_bases(T, A.M, tile);
    const bool packed = A.M.ctl->ragged_seq != A.seq;                   // keys of one width: they travel with their requests
    // packed: request i's key is where the first two offsets say (k_fr_count has compared every request's): no offsets are loaded
    const uint32_t len0 = fr_len0(A), ko0 = A.key_stride ? 0u : A.key_off[0], kstep = A.key_stride ? A.key_stride : len0;
    uint32_t p[FR_PER], o0[FR_PER], klen[FR_PER]; uint64_t hits[FR_PER], limit[FR_PER], duration[FR_PER], misc[FR_PER], kw[FR_PER];
    // where key word w lies in a key of len bytes: whole words, the last one overlapping the one before (nothing is read or written behind
    // the key, whose neighbour's first bytes are another thread's); a key below 8 bytes is one word of which `len` bytes are stored
    auto word_at = [](uint32_t w, uint32_t len) { return 8u * w + 8u <= len || len < 8u ? 8u * w : len - 8u; };
#pragma unroll
    for (int k = 0; k < FR_PER; ++k) {                               // the loads of the thread's four requests, arrival order: coalesced
        const uint32_t i = i0 + k * 256u;
        p[k] = 0xffffffffu; o0[k] = klen[k] = 0; hits[k] = limit[k] = duration[k] = misc[k] = kw[k] = 0;
        if (i >= A.n) continue;
        const uint32_t er = A.M.er[i];
        if (packed) { o0[k] = ko0 + i * kstep; klen[k] = len0; kw[k] = ld_key_word(A.key_bytes + o0[k]); }   // (a key buffer is readable 8 bytes past its last key)
        else { o0[k] = fr_key_off(A, i); klen[k] = fr_key_len(A, i, o0[k]); }
        hits[k] = (uint64_t)A.hits[i]; limit[k] = (uint64_t)A.limit[i]; duration[k] = (uint64_t)A.duration[i];
        misc[k] = (A.behavior ? A.behavior[i] : 0u) | (uint64_t)(A.algorithm ? A.algorithm[i] : (uint8_t)0) << 32 | (uint64_t)(A.is_owner ? A.is_owner[i] : (uint8_t)0) << 40;
        p[k] = fr_place(T, er);
        // (with no place — which the ranks, a permutation of the tile, never give — d wraps to the run's start - 1: still below n or 0)
        const uint32_t d = T.dofs[er >> FR_RANK_BITS] + p[k];
        if (A.d_fwd) A.d_fwd[i] = d < A.n ? d : 0u;                 // (arrival order; only the payload stage's k_wire_enc reads it: null for every other front)
    }
    uint32_t dd[FR_PER];
    fr_sorted_places(T, A.n, dd);
    uint32_t turn = 0;
    // a column: the thread's four values to their sorted places, a barrier, the thread's four sorted elements back
    auto through = [&](const uint64_t (&v)[FR_PER], uint64_t (&o)[FR_PER]) {
        uint64_t* buf = stg[turn++ & 1u];
#pragma unroll
        for (int k = 0; k < FR_PER; ++k) if (p[k] != 0xffffffffu) buf[p[k]] = v[k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < FR_PER; ++k) o[k] = dd[k] != 0xffffffffu ? buf[threadIdx.x + k * 256u] : 0ull;
    };
    auto column = [&](const uint64_t (&v)[FR_PER], int64_t* dst) {
        uint64_t o[FR_PER];
        through(v, o);
#pragma unroll
        for (int k = 0; k < FR_PER; ++k) if (dd[k] != 0xffffffffu) dst[dd[k]] = (int64_t)o[k];
    };
    // (the optional columns are requested a column ahead of their turn: every load of the kernel at its start would be sixty more registers)
    uint64_t opt[FR_PER] = {0, 0, 0, 0}, o[FR_PER];
    auto request = [&](const int64_t* src) {
#pragma unroll
        for (int k = 0; k < FR_PER; ++k) if (p[k] != 0xffffffffu) opt[k] = (uint64_t)src[i0 + k * 256u];
    };
    column(hits, A.d_hits);
    column(limit, A.d_limit);
    if (A.burst) request(A.burst);
    column(duration, A.d_duration);
    if (A.burst) column(opt, A.d_burst);
    if (A.created_at) request(A.created_at);
    through(misc, o);
#pragma unroll
    for (int k = 0; k < FR_PER; ++k) {
        if (dd[k] == 0xffffffffu) continue;
        A.d_behavior[dd[k]] = (uint32_t)o[k]; A.d_algorithm[dd[k]] = (uint8_t)(o[k] >> 32);
        if (A.is_owner) A.d_is_owner[dd[k]] = (uint8_t)(o[k] >> 40);
    }
    if (A.created_at) column(opt, A.d_created_at);
    if (packed) {
        // the keys as 8-byte words, a word a column: a run's keys are contiguous in d_keys (d x len0), so are the words neighbouring threads store
        const uint32_t nw = (len0 + 7u) >> 3;
        for (uint32_t w = 0; w < nw; ++w) {
            uint64_t next[FR_PER] = {0, 0, 0, 0};
            if (w + 1 < nw) {                                        // (the next word is on its way while this one goes through LDS)
#pragma unroll
                for (int k = 0; k < FR_PER; ++k) if (p[k] != 0xffffffffu) next[k] = ld_key_word(A.key_bytes + o0[k] + word_at(w + 1, len0));
            }
            through(kw, o);
#pragma unroll
            for (int k = 0; k < FR_PER; ++k) {
                kw[k] = next[k];
                if (dd[k] == 0xffffffffu) continue;
                uint8_t* dst = A.d_keys + (size_t)dd[k] * len0;
                if (len0 >= 8) __builtin_memcpy(dst + word_at(w, len0), &o[k], 8);
                else for (uint32_t q = 0; q < len0; ++q) dst[q] = (uint8_t)(o[k] >> (8 * q));
            }
        }
        // (no offsets: key d of the mirror is d x len0, which the shares' views say with BatchView::key_width — guber_front.h)
    } else {
        // other keys stay where they are: offset and length travel
        uint64_t ol[FR_PER];
#pragma unroll
        for (int k = 0; k < FR_PER; ++k) ol[k] = o0[k] | (uint64_t)klen[k] << 32;
        through(ol, o);
#pragma unroll
        for (int k = 0; k < FR_PER; ++k) if (dd[k] != 0xffffffffu) { A.d_key_off[dd[k]] = (uint32_t)o[k]; A.d_key_len[dd[k]] = (uint32_t)(o[k] >> 32); }
    }
}

// The answers' last hop, mirrored: sorted element j loads its answer from the shares (consecutive threads, consecutive d), arrival
// position i takes it from LDS at p(i) = lbase[engine] + rank (er[i]: 2 bytes per request instead of fwd's 4) and stores in arrival order.
// The slot's routing scratch (M) is still this generation's here, because the slot is routed into again only behind this kernel —
// front_route waits for the slot's ev_out, which front_out records behind k_fr_out on every stream but the routing's own (where the
// stream's order says the same).
struct FrOut {
    uint32_t n; RouteMap M;
    const uint8_t *d_status, *d_err; const int64_t *d_limit, *d_remaining, *d_reset_time;      // the mirror's answers, in the shares' order
    uint8_t *status, *err; int64_t *limit, *remaining, *reset_time;                           // the caller's result arrays, arrival order
};
// The Store side channel of a store generation's last hop (guber_kernels_front_store.h): store_flags[d] rides with status and error as
// one 32-bit column, and the 64-byte Rec store_after[d] — one full sector per request — is loaded by the sorted side (consecutive
// threads, consecutive d) and stored by the same thread at the request's arrival place, which it learns from a 16-bit column going the
// other way (arrival position -> LDS at p(i) -> sorted element).  A Rec travels only when its request's GUBER_STORE_ONCHANGE bit is set
// (nothing else reads it).
struct FrOutSide {
    const uint8_t* d_flags; const Rec* d_after;                   // the shares' order (Work::store_flags / store_after)
    uint8_t* flags; Rec* after;                                   // arrival order
};
// the narrow columns beside the two 8-byte buffers: status | err << 8, with the side channel | flags << 16 and the way back
template <bool STORE> struct FrOutCols { typedef uint16_t se_t; se_t sse[FR_TILE]; };
template <> struct FrOutCols<true> { typedef uint32_t se_t; se_t sse[FR_TILE]; uint16_t inv[FR_TILE]; };
// One body for k_fr_out (STORE = false: X is not looked at) and k_fr_out_store.  Three 8-byte columns take turns through stg[0], stg[1],
// stg[0], a barrier each: a buffer is written again two columns later, behind the barrier of the column between.
// LDS: the two buffers of k_fr_scatter + the narrow columns + FrTile = 18 568 bytes, 39 registers, no scratch: eight workgroups per CU
// (its wave slots); with the side channel 4 KB + 2 KB in the 2 KB's place and 60 registers.  Under the bench's load 35.1 -> 27.9 us per 1 048 576
// requests (profiles/front_runs_ab.txt).
template <bool STORE> __device__ __forceinline__ void fr_out_tile(const FrOut& A, const FrOutSide& X) {
    typedef typename FrOutCols<STORE>::se_t se_t;
    __shared__ FrTile T;
    __shared__ uint64_t stg[2][FR_TILE];
    __shared__ FrOutCols<STORE> C;
    const uint32_t tile = blockIdx.x, tid = threadIdx.x, i0 = tile * FR_TILE + tid;
    fr_tile_bases(T, A.M, tile);
    uint32_t dd[FR_PER], p[FR_PER]; se_t se[FR_PER]; int64_t l[FR_PER], r[FR_PER], t[FR_PER];
    fr_sorted_places(T, A.n, dd);
#pragma unroll
    for (int k = 0; k < FR_PER; ++k) {                               // every load before the first store
        p[k] = i0 + k * 256u < A.n ? fr_place(T, A.M.er[i0 + k * 256u]) : 0xffffffffu;
        se[k] = 0; l[k] = r[k] = t[k] = 0;
        if (dd[k] == 0xffffffffu) continue;
        const uint32_t err = A.d_err[dd[k]];
        se[k] = (se_t)(A.d_status[dd[k]] | err << 8);
        // (a request to be re-submitted carries no events: engine_host.inl does the same)
        if constexpr (STORE) se[k] |= (err == IE_RETRY ? 0u : (uint32_t)X.d_flags[dd[k]]) << 16;
        l[k] = A.d_limit[dd[k]]; r[k] = A.d_remaining[dd[k]]; t[k] = A.d_reset_time[dd[k]];
    }
#pragma unroll
    for (int k = 0; k < FR_PER; ++k) {
        stg[0][tid + k * 256u] = (uint64_t)l[k]; C.sse[tid + k * 256u] = se[k];
        if constexpr (STORE) if (p[k] != 0xffffffffu) C.inv[p[k]] = (uint16_t)(tid + k * 256u);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FR_PER; ++k) {
        if (p[k] == 0xffffffffu) continue;
        const uint32_t i = i0 + k * 256u; const se_t v = C.sse[p[k]];
        A.limit[i] = (int64_t)stg[0][p[k]]; A.status[i] = (uint8_t)v; A.err[i] = (uint8_t)(v >> 8);
        if constexpr (STORE) X.flags[i] = (uint8_t)(v >> 16);
    }
    if constexpr (STORE) {
#pragma unroll
        for (int k = 0; k < FR_PER; ++k) {                           // the sorted side: its request's record to the arrival place
            if (dd[k] == 0xffffffffu || !((se[k] >> 16) & 1u)) continue;
            const uint32_t i = tile * FR_TILE + C.inv[tid + k * 256u];
            if (i < A.n) X.after[i] = X.d_after[dd[k]];
        }
    }
#pragma unroll
    for (int k = 0; k < FR_PER; ++k) stg[1][tid + k * 256u] = (uint64_t)r[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FR_PER; ++k) if (p[k] != 0xffffffffu) A.remaining[i0 + k * 256u] = (int64_t)stg[1][p[k]];
#pragma unroll
    for (int k = 0; k < FR_PER; ++k) stg[0][tid + k * 256u] = (uint64_t)t[k];      // (everybody has passed the second barrier: nobody reads the first column any more)
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FR_PER; ++k) if (p[k] != 0xffffffffu) A.reset_time[i0 + k * 256u] = (int64_t)stg[0][p[k]];
}
__global__ __launch_bounds__(256) void k_fr_out(FrOut A) { fr_out_tile<false>(A, FrOutSide{}); }

}  // namespace guber
