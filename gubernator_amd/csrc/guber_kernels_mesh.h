// guber_kernels_mesh.h — the kernels of a mesh of fronts (guber_mesh_*, guber_mesh.h): a rank's generation in ARRIVAL order -> request
// records grouped by owning rank -> (exchange) -> request columns for the owner's front -> answer records -> (exchange) -> the
// answers in ARRIVAL order.  Included by guber_kernels.h (and, like the front's kernels, compiled for the host by the tests' fiber emulation).
#pragma once

namespace guber {

// What the reference does per request between peers — V1Instance.GetRateLimits picks the owner from the ring (gubernator.go:236-283,
// replicated_hash.go:104-119), forwards what it does not own (GetPeerRateLimits, evaluated there as the owner: gubernator.go:486) and
// answers in request order (gubernator.proto:51-54) — for a whole generation per rank:
//   k_mx_count   per request: fnv1 / fnv1a of the key, the ring's point -> destination rank, its rank among the tile's requests of that
//                destination (stable: arrival order); per tile of 1 024 requests the requests per destination.  GLOBAL requests
//                (gubernator.go:258-270: never forwarded) and keys the ring cannot place (empty, over-long) have destination self;
//                own[i] = the is_owner the request is evaluated with; item_owner[i] (optional) = the peer the ring names, 0xFF = none
//   k_mx_scan    route_scan: tile bases and the totals per destination, to ctl->tot and — stamped with the call's sequence
//                number — to pinned memory
//   k_mx_pack    the tile sorted by destination in LDS (the place is computed: lbase[dest] + rank), one fixed-width record per request
//                into the send buffer: destination after destination, arrival order inside; consecutive threads write consecutive records
//   k_mx_unpack  the receiver: records -> request columns (the keys stay in the records: the front takes them as rows)
//   k_mx_apack   the receiver's answers (its front's result columns, inflow order) -> 32-byte answer records
//   k_mx_out     k_fr_out's form: the answer of request i lies at the place its request record had in the send buffer (the answers come
//                back slice by slice in the order the requests left): sorted element j loads record j (coalesced), arrival position i
//                takes it from LDS at lbase[dest] + rank (er[i]) and stores in arrival order
// Count, scan, place and report are the front's routing core (guber_kernels_front.h: RouteMap, route_rank_tile, route_scan, fr_place),
// and its lessons hold: no per-workgroup tickets, no system-scope release at a kernel's end, no scratch.
// KEYS.  k_mx_count and k_mx_pack are the two kernels that look at a key, and each exists twice: <false> finds request i's key packed
// (key_bytes + key_off[i], key_off[i + 1] - key_off[i] bytes: what a caller of structure-of-arrays streams holds), <true> finds it in
// ROWS (key_bytes + i * key_stride, key_len[i] bytes: what the device wire decoder leaves, guber_kernels_wire.h).  k_mx_count asks for a
// key's words ahead of its offsets through key_fetch_spec (guber_table.h), with what k_fr_count passes: the guess is the first key's
// width — packed, key i at key_off[0] + i x width; rows, at its row's start — and only the words a key of that width has are
// requested, 8 x ceil(width / 8) bytes, which must end at or before readable_end: 8 bytes behind a packed buffer's last key, the
// row's end for a row (so rows closer than 32 bytes speculate too, when the guess fits a row).  A guess of 0 or of 32 bytes and more,
// or one the request's own offset and length do not confirm, leaves the key to be hashed from memory, its own bytes alone.  So no byte
// outside [row, row + key_stride) is read — the padding behind a key is the caller's and need not be zero — and nothing at or past 8
// bytes behind a packed buffer's last key.  A row cannot hold more than key_stride bytes: a key_len above it is an over-long key.
// The form is the instantiation's, not a branch (profiles/mesh_kernels.txt).
// (dest[i], place[i]) of a request are er[i] and the tile's bases, as in the front: 2 bytes per request instead of 8.
//
// A request record: 64 bytes of columns, then the key row —
//   +0 key_len (u32; an over-long key travels as max_key + 1 bytes: it only ever earns its item error)  +4 behavior (u32)
//   +8 hits  +16 limit  +24 duration  +32 burst  +40 created_at  +48 algorithm | is_owner << 8 (u32)  +56 zero
//   +64 the key, zero-padded to whole 8-byte words (at least four: k_fr_count's speculative hash reads 32 bytes of a row)
// the layout of the GLOBAL hit rows' columns (guber_global_sync.h); rec_bytes = 64 + (max_key_bytes rounded up to 8, plus 8), rounded
// up to 64: a record is whole 64-byte sectors.
constexpr uint32_t MX_COLS = 64;                   // bytes of columns in front of a record's key row
constexpr uint32_t MX_ANS = 32;                    // an answer record: status | err << 8 (u64), limit, remaining, reset_time

struct MxIn {
    uint32_t n, self, world, max_key, seq, npts, kind, ring_lds;
    const uint8_t* key_bytes; const uint32_t* key_off;
    const int64_t *hits, *limit, *duration, *burst, *created_at; const uint32_t* behavior; const uint8_t* algorithm;
    int64_t now_ms;
    const uint64_t* ring_hash; const uint8_t* ring_owner;          // the ring's sorted points (replicated_hash.go:90) and their peers
    RouteMap M; uint8_t* own;
    uint8_t* send; uint32_t rec_bytes;
    uint32_t key_stride; const uint32_t* key_len;                   // <true> only: the rows' distance (a multiple of 8) and the keys' lengths
    uint8_t* item_owner;                                             // optional (null: not wanted): [n] the RING's owner of request i — not its destination — 0xFF where the ring cannot place the key
};

// fnv1 / fnv1a (segmentio/fasthash, as replicated_hash.go uses them) over a key of len < 32 bytes held in four words
__device__ __forceinline__ uint64_t mx_fnv_words4(const uint64_t (&w)[4], uint32_t len, uint32_t kind) {
    uint64_t h = 0xcbf29ce484222325ULL;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t nb = len > 8 * q ? (len - 8 * q < 8 ? len - 8 * q : 8u) : 0u;
        uint64_t v = w[q];
        for (uint32_t b = 0; b < nb; ++b, v >>= 8) {
            if (kind == 1) { h ^= v & 0xffu; h *= 0x100000001b3ULL; } else { h *= 0x100000001b3ULL; h ^= v & 0xffu; }
        }
    }
    return h;
}

// The decision per request, k_mx_count's and k_mx_small's (guber_kernels_small.h) alike, in ONE place.  A macro, not a function: k_mx_count's
// instruction stream is part of what the benchmark measures, and the statements below are the ones it has always had — a function taking
// the hash as a callable compiled to another stream.  For a request that arrived at rank SELF with a key of LEN bytes (HASH: the expression
// of its fnv1 / fnv1a, evaluated only when the key is not over-long; GLOBAL: Behavior_GLOBAL is set) it declares
//   stay   the request is not forwarded: GLOBAL (gubernator.go:258-270), or a key the ring cannot place (empty, above MAX_KEY)
//   owner  the ring's peer for the key — ReplicatedConsistentHash.Get (replicated_hash.go:104-119): the first point at or behind the key's
//          hash, wrapping to point 0 (an over-long key is not hashed: nobody looks at the owner of a request that only earns its item error)
// and MX_EVAL_RANK / MX_IS_OWNER / MX_ITEM_OWNER below say what follows from the two.
#define MX_DECIDE(stay, owner, GLOBAL, LEN, SELF, MAX_KEY, NPTS, LH, RING_OWNER, HASH)                                                     \
    const bool stay = (GLOBAL) || (LEN) == 0 || (LEN) > (MAX_KEY);                                                                        \
    uint32_t owner = (SELF);                                                                                                              \
    if ((LEN) <= (MAX_KEY)) {                                                                                                             \
        const uint64_t h = (HASH);                                                                                                        \
        uint32_t lo = 0, hi = (NPTS);                                                                                                     \
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if ((LH)[mid] >= h) hi = mid; else lo = mid + 1; }                  \
        if (lo == (NPTS)) lo = 0;                                                                                                         \
        owner = (RING_OWNER)[lo];                                                                                                         \
    }
// the rank that evaluates the request
#define MX_EVAL_RANK(stay, owner, SELF, WORLD) ((stay) || (owner) >= (WORLD) ? (SELF) : (owner))
// the is_owner it is evaluated with (forwarded or owned here: evaluated as the owner, gubernator.go:247-256, :486)
#define MX_IS_OWNER(stay, owner, SELF) ((stay) ? (uint8_t)((owner) == (SELF)) : (uint8_t)1)
// who the ring names, for the caller that tells its client (metadata "owner", gubernator.go:267-268, :379-381): a GLOBAL request's too,
// although it stays; a key the ring cannot place (empty, over-long) has none
#define MX_ITEM_OWNER(LEN, MAX_KEY, owner) (((LEN) == 0 || (LEN) > (MAX_KEY)) ? (uint8_t)0xffu : (uint8_t)(owner))

template <bool ROWS> __global__ __launch_bounds__(FR_TILE) void k_mx_count(MxIn A) {
    GUBER_DYN_LDS(smem);                                             // the ring's hashes (npts x 8 bytes) when they fit beside route_rank_tile's 1 KB
    const uint32_t tid = threadIdx.x, i = blockIdx.x * FR_TILE + tid;
    const uint64_t* lh = A.ring_hash;
    if (A.ring_lds) {
        uint64_t* l = (uint64_t*)smem;
        for (uint32_t j = tid; j < A.npts; j += FR_TILE) l[j] = A.ring_hash[j];
        lh = l;
        __syncthreads();
    }
    uint32_t e = 0xffu;
    if (i < A.n) {
        // keys of one width: the key's words are requested where the first key's width suggests, together with the request's own offsets,
        // and used if those confirm the guess (key_fetch_spec; KEYS above)
        uint32_t off, len; uint64_t off_g, readable_end;
        const uint32_t len0 = wave_uniform(ROWS ? A.key_len[0] : A.key_off[1] - A.key_off[0]);
        if constexpr (ROWS) { off_g = (uint64_t)i * A.key_stride; readable_end = off_g + A.key_stride; }
        else { off_g = (uint64_t)A.key_off[0] + (uint64_t)i * len0; readable_end = (uint64_t)A.key_off[A.n] + 8; }
        uint64_t kw[4] = {0, 0, 0, 0};
        const bool spec = key_fetch_spec(A.key_bytes, off_g, len0, readable_end, kw);
        if constexpr (ROWS) {
            off = (uint32_t)off_g; len = A.key_len[i];
            if (len > A.key_stride) len = A.max_key + 1u;            // (more than a row holds: over-long, never read)
        } else { off = A.key_off[i]; len = A.key_off[i + 1] - off; }
        MX_DECIDE(stay, owner, A.behavior && (A.behavior[i] & 2u), len, A.self, A.max_key, A.npts, lh, A.ring_owner,
                  (spec && off == off_g && len == len0) ? mx_fnv_words4(kw, len, A.kind)
                                                        : (A.kind == 1 ? fnv1a_64(A.key_bytes + off, len) : fnv1_64(A.key_bytes + off, len)))
        e = MX_EVAL_RANK(stay, owner, A.self, A.world);
        A.own[i] = MX_IS_OWNER(stay, owner, A.self);
        // As d_fwd in the front: stored only when wanted.
        if (A.item_owner) A.item_owner[i] = MX_ITEM_OWNER(len, A.max_key, owner);
    }
    route_rank_tile(e, A.M, i, A.n);
}

// one rank: no routing runs, and the ring has one peer — item_owner[i] = 0, or 0xFF for a key no ring places.  Rows only (lengths as
// k_mx_count<true> reads them): the one caller that asks for the column hands over a decoder's rows.
__global__ __launch_bounds__(256) void k_mx_owner_one(uint32_t n, const uint32_t* key_len, uint32_t key_stride, uint32_t max_key, uint8_t* item_owner) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t len = key_len[i];                                // (more than a row holds: over-long, as any length above max_key)
    item_owner[i] = (len == 0 || len > max_key || len > key_stride) ? (uint8_t)0xffu : (uint8_t)0;
}

__global__ __launch_bounds__(FR_SCAN_T) void k_mx_scan(MxIn A, uint32_t nt, uint32_t per) { route_scan(A.M, A.seq, nt, per); }

// LDS: the tile's requests in the destinations' order (2 KB) + FrTile.  Sorted element j gathers its request's columns (the tile's 1 024
// requests: lines its neighbours load too) and writes record dofs[dest] + j: consecutive threads, consecutive records, whole sectors.
template <bool ROWS> __global__ __launch_bounds__(256) void k_mx_pack(MxIn A) {
    __shared__ FrTile T;
    __shared__ uint16_t src[FR_TILE];
    const uint32_t tile = blockIdx.x, tid = threadIdx.x, i0 = tile * FR_TILE + tid;
    fr_tile_bases(T, A.M, tile);
#pragma unroll
    for (int k = 0; k < FR_PER; ++k) {
        const uint32_t i = i0 + k * 256u;
        if (i >= A.n) continue;
        const uint32_t p = fr_place(T, A.M.er[i]);
        if (p != 0xffffffffu) src[p] = (uint16_t)(tid + k * 256u);
    }
    __syncthreads();
    uint32_t dd[FR_PER];
    fr_sorted_places(T, A.n, dd);
    const uint32_t area_words = (A.rec_bytes - MX_COLS) >> 3;
#pragma unroll 1
    for (int k = 0; k < FR_PER; ++k) {
        if (dd[k] == 0xffffffffu) continue;
        const uint32_t i = tile * FR_TILE + src[tid + k * 256u];
        if (i >= A.n) continue;                                      // (cannot happen: the places are a permutation of the tile's requests)
        uint32_t off, len;
        if constexpr (ROWS) { off = i * A.key_stride; len = A.key_len[i]; if (len > A.key_stride) len = A.max_key + 1u; }
        else { off = A.key_off[i]; len = A.key_off[i + 1] - off; }
        const uint32_t lenc = len <= A.max_key ? len : A.max_key + 1u;
        uint64_t* r = (uint64_t*)(A.send + (size_t)dd[k] * A.rec_bytes);
        r[0] = lenc | (uint64_t)(A.behavior ? A.behavior[i] : 0u) << 32;
        r[1] = (uint64_t)A.hits[i]; r[2] = (uint64_t)A.limit[i]; r[3] = (uint64_t)A.duration[i];
        r[4] = A.burst ? (uint64_t)A.burst[i] : 0ull;
        r[5] = (uint64_t)(A.created_at ? A.created_at[i] : A.now_ms);           // (gubernator.go:218-220: a request without CreatedAt takes the arrival rank's clock)
        r[6] = (uint64_t)(A.algorithm ? A.algorithm[i] : (uint8_t)0) | (uint64_t)A.own[i] << 8;
        r[7] = 0ull;
        const uint32_t nw = (lenc + 7u) >> 3;
        uint32_t nwr = nw < 4u ? 4u : nw;
        if (nwr > area_words) nwr = area_words;
        const uint8_t* kp = A.key_bytes + off;
        for (uint32_t w = 0; w < nwr; ++w) {
            uint64_t v = 0ull;
            // (packed: nothing is read more than 7 bytes behind the key; rows: a word that would start at or behind the row's end is zero, not loaded)
            if (w < nw && (!ROWS || 8u * w < A.key_stride)) { v = ld_key_word(kp + 8 * w); if (w == nw - 1) v &= tail_mask(lenc - 8 * w); }
            r[8 + w] = v;
        }
    }
}

struct MxUnpack {
    uint32_t m, rec_bytes; const uint8_t* recv;
    uint32_t* key_len; int64_t *hits, *limit, *duration, *burst, *created_at; uint32_t* behavior; uint8_t *algorithm, *is_owner;
};
__global__ __launch_bounds__(256) void k_mx_unpack(MxUnpack U) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= U.m) return;
    const uint4* r = (const uint4*)(U.recv + (size_t)q * U.rec_bytes);
    const uint4 a = r[0], b = r[1], c = r[2], d = r[3];
    U.key_len[q] = a.x; U.behavior[q] = a.y;
    U.hits[q] = (int64_t)((uint64_t)a.z | (uint64_t)a.w << 32);
    U.limit[q] = (int64_t)((uint64_t)b.x | (uint64_t)b.y << 32); U.duration[q] = (int64_t)((uint64_t)b.z | (uint64_t)b.w << 32);
    U.burst[q] = (int64_t)((uint64_t)c.x | (uint64_t)c.y << 32); U.created_at[q] = (int64_t)((uint64_t)c.z | (uint64_t)c.w << 32);
    U.algorithm[q] = (uint8_t)d.x; U.is_owner[q] = (uint8_t)(d.x >> 8);
}

struct MxAns {
    uint32_t m; const uint8_t *status, *err; const int64_t *limit, *remaining, *reset_time; uint8_t* out;
};
__global__ __launch_bounds__(256) void k_mx_apack(MxAns S) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= S.m) return;
    const uint64_t se = (uint64_t)S.status[q] | (uint64_t)S.err[q] << 8, l = (uint64_t)S.limit[q], rm = (uint64_t)S.remaining[q], t = (uint64_t)S.reset_time[q];
    uint4* o = (uint4*)(S.out + (size_t)q * MX_ANS);
    o[0] = make_uint4((uint32_t)se, 0u, (uint32_t)l, (uint32_t)(l >> 32));
    o[1] = make_uint4((uint32_t)rm, (uint32_t)(rm >> 32), (uint32_t)t, (uint32_t)(t >> 32));
}

// LDS: the tile's answer records in slice order (32 KB) + FrTile: four workgroups of four waves per CU.
struct MxOut {
    uint32_t n; RouteMap M;
    const uint8_t* ans;                                              // the answer records as they came back: the send buffer's order
    uint8_t *status, *err; int64_t *limit, *remaining, *reset_time; // the caller's result arrays, arrival order
};
__global__ __launch_bounds__(256) void k_mx_out(MxOut A) {
    __shared__ FrTile T;
    __shared__ uint4 stg[FR_TILE][2];
    const uint32_t tile = blockIdx.x, tid = threadIdx.x, i0 = tile * FR_TILE + tid;
    fr_tile_bases(T, A.M, tile);
    uint32_t dd[FR_PER];
    fr_sorted_places(T, A.n, dd);
#pragma unroll
    for (int k = 0; k < FR_PER; ++k) {
        if (dd[k] == 0xffffffffu) continue;
        const uint4* a = (const uint4*)(A.ans + (size_t)dd[k] * MX_ANS);
        stg[tid + k * 256u][0] = a[0]; stg[tid + k * 256u][1] = a[1];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FR_PER; ++k) {
        const uint32_t i = i0 + k * 256u;
        if (i >= A.n) continue;
        const uint32_t p = fr_place(T, A.M.er[i]);
        if (p == 0xffffffffu) continue;
        const uint4 x = stg[p][0], y = stg[p][1];
        A.status[i] = (uint8_t)x.x; A.err[i] = (uint8_t)(x.x >> 8);
        A.limit[i] = (int64_t)((uint64_t)x.z | (uint64_t)x.w << 32);
        A.remaining[i] = (int64_t)((uint64_t)y.x | (uint64_t)y.y << 32);
        A.reset_time[i] = (int64_t)((uint64_t)y.z | (uint64_t)y.w << 32);
    }
}

}  // namespace guber
