// guber_mesh.h — guber_mesh_*: a mesh of fronts.  Every rank (peer r of a guber_ring_t, one guber_front_t over the engines of one
// device) hands over the generation that ARRIVED at it; every request is evaluated on the rank the ring names and answered, in arrival
// order, on the rank where it arrived.  Part of guber_engine.hip's translation unit, behind guber_front.h (it drives the fronts through
// front_eval) and guber_global_sync.h (whose local transport this one follows).
//
// Reference: V1Instance.GetRateLimits (gubernator.go:236-283) picks the owner of a request from the ring (replicated_hash.go:104-119),
// evaluates what it owns with IsOwner (gubernator.go:247-256), forwards the rest to the owner through GetPeerRateLimits, where it is
// evaluated as the owner's own (gubernator.go:486), and answers in request order (gubernator.proto:51-54).  Requests with
// Behavior_GLOBAL are never forwarded (gubernator.go:258-270, 395-421): they stay on the arrival rank with is_owner = (owner == rank)
// and go to its front's global_engine.  A request the ring cannot place (empty key, key above the rank's max_key_bytes) stays too and
// earns the front's item error.
// ORDER.  The reference fans the forwarded items out concurrently (gubernator.go:498) and fixes no order between peers; this one does:
// per call, owner o evaluates the slices from source 0, 1, ... W-1 — its own in its place in that sequence — each in arrival order.  The
// requests of one key from one source keep their order; across sources the lower rank goes first.
//
// One call:
//   rank s, its front's routing stream   k_mx_count  k_mx_scan  k_mx_pack                                        [event pack(s)]
//   host                                 waits for the W x W counts (pinned memory, stamped with the call's number) — nothing else
//   rank o                               wait pack(s) | copy slice s -> o, s = 0 .. W-1 | k_mx_unpack | the front: the inflow in pieces
//                                        of at most its max_n (front_eval, count = pieces) | k_mx_apack              [event ans(o)]
//   rank s                               wait ans(o) | copy answer slice o -> s, o = 0 .. W-1 | k_mx_out          [event done(s)]
// TRANSPORT.  Two functions, counts and slices (mesh_exchange_counts, mesh_exchange), as gs_exchange_counts / gs_exchange: this is
// their local mode — every rank in this process, hipMemcpyAsync device-to-device on the RECEIVER's stream, correct for logical ranks
// that share a GPU as well.  The grouped ncclSend / ncclRecv form and one rank per process belong behind the same two functions and
// are not built.
// LOCKS.  The mesh's own mutex for the call; every front's mutex and the engines' (address order, EngineLocks, group by group) are taken
// where front_eval takes them — the mesh's kernels touch no engine state, and sixteen ranks of sixteen engines are more than one
// EngineLocks holds.
#pragma once

struct guber_mesh {
    std::mutex mu;
    uint32_t W = 0, max_n = 0, seq = 0, rec_bytes = 0, npts = 0, kind = 0; bool ring_lds = false;
    struct Rank {
        guber_front* f = nullptr; int device = 0; hipStream_t st = nullptr;
        uint32_t max_key = 0, cap_in = 0;                            // cap_in: the largest inflow (W x max_n records)
        DevBuf<uint8_t> scratch, send, recv, cols, ans_send, ans_recv, ring_o; DevBuf<uint64_t> ring_h; CohBuf<FrontHost> host;
        MxIn in{}; MxUnpack un{}; MxAns an{};
        hipEvent_t ev_pack = nullptr, ev_ans = nullptr, ev_done = nullptr; std::vector<hipEvent_t> ev_eng; bool done_recorded = false;
        uint32_t n = 0;
    };
    std::vector<Rank> ranks;
    guber_mesh_stats_t st{};
    std::vector<uint64_t> ring_hh; std::vector<uint8_t> ring_o8;     // the ring's points on the host (guber_mesh_eval_small uploads them for a mesh of one rank)
    // the one-launch path's state (guber_mesh_eval_small, below), allocated by its first call
    struct Small {
        uint8_t* arena = nullptr; uint32_t key_cap = 0, seq = 0; bool ready = false;
        // the arena's columns (FT requests), see mesh_small_carve
        int64_t *hits = nullptr, *limit = nullptr, *duration = nullptr, *burst = nullptr, *created_at = nullptr, *o_limit = nullptr, *o_remaining = nullptr, *o_reset = nullptr;
        uint32_t *key_off = nullptr, *behavior = nullptr, *where = nullptr, *src_start = nullptr, *taken = nullptr;
        uint8_t *algorithm = nullptr, *own = nullptr, *o_status = nullptr, *o_err = nullptr, *keys = nullptr, *outs = nullptr;
        struct PerRank {
            DevBuf<uint32_t> src_max; DevBuf<uint8_t> gen;            // the ranks' max_key_bytes; the wholesale fall-back's device copy of a generation
            std::vector<hipEvent_t> ev;                              // one per engine stream: the launch goes behind what is enqueued there
        };
        std::vector<PerRank> ranks;
        guber_mesh_small_stats_t st{};
    } sm;
};

extern "C" void guber_mesh_destroy(guber_mesh_t* m) {
    if (!m) return;
    for (auto& R : m->ranks) {
        (void)hipSetDevice(R.device);
        if (R.st) (void)hipStreamSynchronize(R.st);
        R.scratch.release(); R.send.release(); R.recv.release(); R.cols.release(); R.ans_send.release(); R.ans_recv.release();
        R.ring_o.release(); R.ring_h.release(); R.host.release();
        for (hipEvent_t ev : {R.ev_pack, R.ev_ans, R.ev_done}) if (ev) (void)hipEventDestroy(ev);
        for (hipEvent_t ev : R.ev_eng) if (ev) (void)hipEventDestroy(ev);
    }
    for (size_t r = 0; r < m->sm.ranks.size(); ++r) {                // (the one-launch path's: its streams were synchronised above)
        auto& P = m->sm.ranks[r];
        (void)hipSetDevice(m->ranks[r].device);
        P.src_max.release(); P.gen.release();
        for (hipEvent_t ev : P.ev) if (ev) (void)hipEventDestroy(ev);
    }
    if (m->sm.arena) (void)hipHostFree(m->sm.arena);
    delete m;
}

extern "C" int guber_mesh_create_local(guber_front_t* const* fronts, uint32_t n_ranks, const guber_ring_t* ring, uint32_t max_n, guber_mesh_t** out) {
    // (every check before the first HIP call, and before a front is looked into)
    if (!fronts || !ring || !out) return fail(GUBER_E_INVALID_ARG, "null argument");
    *out = nullptr;
    if (n_ranks == 0 || n_ranks > (uint32_t)MULTI_MEM_MAX) return fail(GUBER_E_INVALID_ARG, "1 .. 16 ranks per mesh");
    if (max_n == 0 || max_n > FR_MAX_N) return fail(GUBER_E_BATCH_TOO_LARGE, "a generation holds at most 4 194 304 requests");
    const uint32_t npts = guber_ring_points(ring, nullptr, nullptr, 0);
    if (npts == 0 || npts > (1u << 20)) return fail(GUBER_E_INVALID_ARG, "guber_mesh: the ring is empty or has more than 2^20 points");
    std::vector<uint64_t> hh(npts); std::vector<uint32_t> oo(npts);
    guber_ring_points(ring, hh.data(), oo.data(), npts);
    uint32_t peers = 0;
    for (uint32_t o : oo) peers = std::max(peers, o + 1);
    if (peers != n_ranks) return fail(GUBER_E_INVALID_ARG, "guber_mesh: rank r is peer r of the ring — the ring has another number of peers");
    for (uint32_t r = 0; r < n_ranks; ++r) {
        if (!fronts[r]) return fail(GUBER_E_INVALID_ARG, "null front");
        for (uint32_t q = 0; q < r; ++q) if (fronts[q] == fronts[r]) return fail(GUBER_E_INVALID_ARG, "a front twice in one mesh");
    }
    std::unique_ptr<guber_mesh, void (*)(guber_mesh*)> m(new guber_mesh(), [](guber_mesh* p) { guber_mesh_destroy(p); });
    m->W = n_ranks; m->max_n = max_n; m->npts = npts; m->kind = (uint32_t)guber_ring_kind(ring);
    // the ring's hashes in LDS while they fit beside k_mx_count's 1 KB in the 64 KB every launch may take (fifteen peers of 512
    // replicas do); a larger ring is searched where it lies — 64 KB that stay in the L2
    m->ring_lds = (size_t)npts * 8 + 2048 <= 64 * 1024;
    uint32_t max_key = 0;
    for (uint32_t r = 0; r < n_ranks; ++r) max_key = std::max(max_key, fronts[r]->max_key);
    m->rec_bytes = (MX_COLS + ((max_key + 7u) & ~7u) + 8u + 63u) & ~63u;
    std::vector<uint8_t> o8(npts);
    for (uint32_t j = 0; j < npts; ++j) o8[j] = (uint8_t)oo[j];
    m->ring_hh = hh; m->ring_o8 = o8;
    m->ranks.resize(n_ranks);
    const size_t cap_in = (size_t)n_ranks * max_n, rb = m->rec_bytes;
    for (uint32_t r = 0; r < n_ranks; ++r) {
        auto& R = m->ranks[r];
        guber_front* f = fronts[r];
        R.f = f; R.device = f->device; R.st = f->rs; R.max_key = f->max_key; R.cap_in = (uint32_t)std::min<size_t>(cap_in, 0xffffffffu);
        // (the front addresses a piece's key rows with 32-bit offsets)
        if ((uint64_t)std::min<size_t>(f->cap, cap_in) * rb > 0xffffffffull) return fail(GUBER_E_BATCH_TOO_LARGE, "guber_mesh: a front's generation of key rows exceeds 4 GB");
        if (n_ranks == 1) continue;                                  // (one rank: the front alone, no exchange)
        if (hipSetDevice(R.device) != hipSuccess) return fail(GUBER_E_HIP, "hipSetDevice");
        // the inflow's request columns and its answers
        auto carve_cols = [&](uint8_t* base) {
            ColCarver c{(uintptr_t)base};
            MxUnpack& U = R.un;
            U.hits = c.take<int64_t>(cap_in); U.limit = c.take<int64_t>(cap_in); U.duration = c.take<int64_t>(cap_in);
            U.burst = c.take<int64_t>(cap_in); U.created_at = c.take<int64_t>(cap_in);
            U.key_len = c.take<uint32_t>(cap_in); U.behavior = c.take<uint32_t>(cap_in);
            U.algorithm = c.take<uint8_t>(cap_in); U.is_owner = c.take<uint8_t>(cap_in);
            MxAns& S = R.an;
            S.limit = c.take<int64_t>(cap_in); S.remaining = c.take<int64_t>(cap_in); S.reset_time = c.take<int64_t>(cap_in);
            S.status = c.take<uint8_t>(cap_in); S.err = c.take<uint8_t>(cap_in);
            return (size_t)(c.at - (uintptr_t)base);
        };
        // the routing scratch, and own[] behind it (the routing scratch is carved as one piece)
        auto carve_scratch = [&](uint8_t* base) {
            ColCarver c{(uintptr_t)base};
            R.in.M = route_carve(c, max_n, R.host.p); R.in.own = c.take<uint8_t>(max_n);
            return (size_t)(c.at - (uintptr_t)base);
        };
        if (R.scratch.ensure(carve_scratch(nullptr)) || R.send.ensure((size_t)max_n * rb + 64) || R.recv.ensure(cap_in * rb + 64) ||
            R.cols.ensure(carve_cols(nullptr)) || R.ans_send.ensure(cap_in * MX_ANS + 64) || R.ans_recv.ensure((size_t)max_n * MX_ANS + 64) ||
            R.ring_h.ensure(npts) || R.ring_o.ensure(npts) || R.host.ensure(1)) return GUBER_E_NOMEM;
        memset((void*)R.host.p, 0, sizeof(FrontHost));
        carve_cols(R.cols.p); carve_scratch(R.scratch.p);
        MxIn& A = R.in;
        A.send = R.send.p; A.rec_bytes = m->rec_bytes;
        A.self = r; A.world = n_ranks; A.max_key = R.max_key; A.npts = npts; A.kind = m->kind; A.ring_lds = m->ring_lds ? 1u : 0u;
        A.ring_hash = R.ring_h.p; A.ring_owner = R.ring_o.p;
        R.un.rec_bytes = m->rec_bytes; R.un.recv = R.recv.p; R.an.out = R.ans_send.p;
        HIPCHK(hipMemcpyAsync(R.ring_h.p, hh.data(), (size_t)npts * 8, hipMemcpyHostToDevice, R.st));
        HIPCHK(hipMemcpyAsync(R.ring_o.p, o8.data(), npts, hipMemcpyHostToDevice, R.st));
        HIPCHK(hipMemsetAsync(A.M.ctl, 0, sizeof(FrontCtl), R.st));
        HIPCHK(hipMemsetAsync(R.recv.p, 0, cap_in * rb + 64, R.st));      // (key rows are read as 8-byte words: every byte of a row is defined)
        HIPCHK(hipEventCreateWithFlags(&R.ev_pack, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&R.ev_ans, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&R.ev_done, hipEventDisableTiming));
        for (size_t q = 0; q < f->streams.size() + 1; ++q) { hipEvent_t ev = nullptr; HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); R.ev_eng.push_back(ev); }
        HIPCHK(hipStreamSynchronize(R.st));
    }
    *out = m.release();
    return GUBER_OK;
}

// table[s * W + o] = requests rank s sends rank o: the host waits for every sender's k_mx_scan words of THIS call — the only wait of a call
static int mesh_exchange_counts(guber_mesh* m, std::vector<uint32_t>& table) {
    const uint32_t W = m->W;
    table.assign((size_t)W * W, 0);
    for (uint32_t s = 0; s < W; ++s) {
        auto& R = m->ranks[s];
        if (R.n == 0) continue;
        const int rc = route_wait_reported(R.host.p, MULTI_MEM_MAX, m->seq, R.device, R.st, "guber_mesh: the routing of a generation did not report");
        if (rc) return rc;
        uint64_t tot = 0;
        for (uint32_t o = 0; o < (uint32_t)MULTI_MEM_MAX; ++o) {
            const uint32_t c = (uint32_t)R.host.p->w[o];
            if (o < W) table[(size_t)s * W + o] = c;
            tot += c;
        }
        if (tot != R.n) return fail(GUBER_E_HIP, "guber_mesh: the slices do not add up to the generation");
    }
    return 0;
}
// rank `to` receives from every rank the slice meant for it, in rank order, on ITS stream behind the sender's event: request records
// (answers = false: sender s's slice for `to` lies behind its slices for the ranks below `to`) or answer records (answers = true: owner
// o's answers for `to` lie behind its answers for the sources below `to` — the transpose)
static int mesh_exchange(guber_mesh* m, const std::vector<uint32_t>& table, uint32_t to, bool answers) {
    const uint32_t W = m->W;
    auto& R = m->ranks[to];
    const size_t rb = answers ? MX_ANS : m->rec_bytes;
    uint8_t* dst = answers ? R.ans_recv.p : R.recv.p;
    size_t roff = 0;
    for (uint32_t p = 0; p < W; ++p) {
        auto& P = m->ranks[p];
        const size_t cnt = answers ? table[(size_t)to * W + p] : table[(size_t)p * W + to];
        if (!cnt) continue;
        size_t soff = 0;
        for (uint32_t q = 0; q < to; ++q) soff += answers ? table[(size_t)q * W + p] : table[(size_t)p * W + q];
        if (p != to) HIPCHK(hipStreamWaitEvent(R.st, answers ? P.ev_ans : P.ev_pack, 0));
        HIPCHK(hipMemcpyAsync(dst + roff * rb, (answers ? P.ans_send.p : P.send.p) + soff * rb, cnt * rb, hipMemcpyDeviceToDevice, R.st));
        if (p != to) { m->st.forwarded += answers ? 0 : cnt; m->st.bytes_moved += cnt * rb; }
        roff += cnt;
    }
    return 0;
}

// generation b in pieces of at most the front's max_n, through the count argument of front_eval
static int mesh_front_pieces(guber_mesh* m, guber_front* f, const FrontGen& g, const guber_result_t& r) {
    std::vector<FrontGen> gens; std::vector<guber_result_t> res;
    const uint32_t n = g.b.n, step = f->cap;
    for (uint32_t pos = 0; pos < n; pos += step) {
        FrontGen p = g;
        p.b.n = std::min(step, n - pos);
        if (g.key_stride) { p.b.key_bytes = g.b.key_bytes + (size_t)pos * g.key_stride; p.key_len = g.key_len + pos; }
        else p.b.key_off = g.b.key_off + pos;
        p.b.hits += pos; p.b.limit += pos; p.b.duration += pos;
        if (p.b.burst) p.b.burst += pos;
        if (p.b.created_at) p.b.created_at += pos;
        if (p.b.behavior) p.b.behavior += pos;
        if (p.b.algorithm) p.b.algorithm += pos;
        if (p.b.is_owner) p.b.is_owner += pos;
        guber_result_t q{};
        q.status = r.status + pos; q.err = r.err + pos; q.limit = r.limit + pos; q.remaining = r.remaining + pos; q.reset_time = r.reset_time + pos;
        gens.push_back(p); res.push_back(q);
    }
    m->st.inflow_pieces += gens.size();
    uint32_t done = 0;
    return front_eval(f, gens.data(), res.data(), (uint32_t)gens.size(), &done);
}

// item_owner: NULL, or per rank NULL or n bytes on the rank's device — the ring's owner of every arrival item (k_mx_count's optional output)
static int mesh_eval(guber_mesh* m, const guber_batch_t* gens, const guber_mesh_rows_t* rows, guber_result_t* results, uint8_t* const* item_owner = nullptr) {
    const uint32_t W = m->W;
    uint64_t total = 0;
    for (uint32_t r = 0; r < W; ++r) { m->ranks[r].n = gens[r].n; total += gens[r].n; clear_aggregates(results[r]); }
    m->st.calls++; m->st.requests += total;
    if (W == 1) {
        if (gens[0].n == 0) return 0;
        if (item_owner && item_owner[0]) {
            auto& R = m->ranks[0];
            if (!rows || !rows[0].key_stride) return fail(GUBER_E_INVALID_ARG, "guber_mesh: the owner column is written for key rows");
            HIPCHK(hipSetDevice(R.device));
            hipLaunchKernelGGL(k_mx_owner_one, dim3((gens[0].n + 255u) / 256u), dim3(256), 0, R.st, gens[0].n, rows[0].key_len, rows[0].key_stride, R.f->max_key, item_owner[0]);
            if (hipGetLastError() != hipSuccess) return fail(GUBER_E_HIP, "kernel launch");
        }
        FrontGen g; g.b = gens[0];
        if (rows && rows[0].key_stride) { g.key_stride = rows[0].key_stride; g.key_len = rows[0].key_len; }   // (the front takes rows itself)
        return mesh_front_pieces(m, m->ranks[0].f, g, results[0]);
    }
    if (++m->seq == 0) m->seq = 1;
    // routing: count, scan, pack on every rank's stream
    for (uint32_t r = 0; r < W; ++r) {
        auto& R = m->ranks[r];
        HIPCHK(hipSetDevice(R.device));
        // (the last call's copies on the other ranks' streams have read what this call writes: its request and answer records)
        for (uint32_t q = 0; q < W; ++q) if (q != r && m->ranks[q].done_recorded) HIPCHK(hipStreamWaitEvent(R.st, m->ranks[q].ev_done, 0));
        const guber_batch_t& b = gens[r];
        if (b.n) {
            MxIn& A = R.in;
            A.n = b.n; A.seq = m->seq; A.now_ms = b.now_ms;
            A.key_bytes = b.key_bytes; A.key_off = b.key_off; A.hits = b.hits; A.limit = b.limit; A.duration = b.duration; A.burst = b.burst;
            A.created_at = b.created_at; A.behavior = b.behavior; A.algorithm = b.algorithm;
            const bool in_rows = rows && rows[r].key_stride;         // (a rank's form is its own: each launches its own routing kernels)
            A.key_stride = in_rows ? rows[r].key_stride : 0u; A.key_len = in_rows ? rows[r].key_len : nullptr;
            A.item_owner = item_owner ? item_owner[r] : nullptr;
            const uint32_t tiles = (b.n + FR_TILE - 1u) / FR_TILE;
            const size_t ring_bytes = m->ring_lds ? (size_t)m->npts * 8 : 0;
            if (in_rows) hipLaunchKernelGGL(k_mx_count<true>, dim3(tiles), dim3(FR_TILE), ring_bytes, R.st, A);
            else hipLaunchKernelGGL(k_mx_count<false>, dim3(tiles), dim3(FR_TILE), ring_bytes, R.st, A);
            hipLaunchKernelGGL(k_mx_scan, dim3(MULTI_MEM_MAX / 4), dim3(FR_SCAN_T), 0, R.st, A, tiles, (tiles + FR_SCAN_T - 1) / FR_SCAN_T);
            if (in_rows) hipLaunchKernelGGL(k_mx_pack<true>, dim3(tiles), dim3(256), 0, R.st, A);
            else hipLaunchKernelGGL(k_mx_pack<false>, dim3(tiles), dim3(256), 0, R.st, A);
            if (hipGetLastError() != hipSuccess) return fail(GUBER_E_HIP, "kernel launch");
        }
        HIPCHK(hipEventRecord(R.ev_pack, R.st));
    }
    std::vector<uint32_t> table;
    { const int rc = mesh_exchange_counts(m, table); if (rc) return rc; }
    // every owner: its inflow, its front, its answers as records
    int rc = 0;
    for (uint32_t o = 0; o < W; ++o) {
        auto& R = m->ranks[o];
        guber_front* f = R.f;
        HIPCHK(hipSetDevice(R.device));
        uint64_t inflow = 0;
        for (uint32_t s = 0; s < W; ++s) inflow += table[(size_t)s * W + o];
        if (inflow > R.cap_in) return fail(GUBER_E_HIP, "guber_mesh: an inflow larger than every rank's generation together");
        if (inflow) {
            { const int r2 = mesh_exchange(m, table, o, false); if (r2) return r2; }
            MxUnpack U = R.un; U.m = (uint32_t)inflow;
            hipLaunchKernelGGL(k_mx_unpack, dim3((U.m + 255u) / 256u), dim3(256), 0, R.st, U);
            if (hipGetLastError() != hipSuccess) return fail(GUBER_E_HIP, "kernel launch");
            if (f->rs != R.st || f->rs2 != R.st) {                   // (the front routes on a stream that is not the one the mesh was created on)
                HIPCHK(hipEventRecord(R.ev_eng.back(), R.st));
                for (hipStream_t st : {f->rs, f->rs2}) if (st != R.st) HIPCHK(hipStreamWaitEvent(st, R.ev_eng.back(), 0));
            }
            FrontGen g;
            g.b = guber_batch_t{};
            g.b.n = U.m; g.b.key_bytes = R.recv.p + MX_COLS; g.b.hits = U.hits; g.b.limit = U.limit; g.b.duration = U.duration; g.b.burst = U.burst;
            g.b.created_at = U.created_at; g.b.algorithm = U.algorithm; g.b.behavior = U.behavior; g.b.is_owner = U.is_owner; g.b.now_ms = gens[0].now_ms;
            g.key_stride = m->rec_bytes; g.key_len = U.key_len;
            guber_result_t ar{};
            ar.status = (uint8_t*)R.an.status; ar.err = (uint8_t*)R.an.err; ar.limit = (int64_t*)R.an.limit; ar.remaining = (int64_t*)R.an.remaining; ar.reset_time = (int64_t*)R.an.reset_time;
            rc = mesh_front_pieces(m, f, g, ar);
            if (rc) return rc;
            // the answers' records behind everything the front has enqueued: its engines' streams and its own
            HIPCHK(hipSetDevice(R.device));
            size_t q = 0;
            for (hipStream_t st : f->streams) if (st != R.st) { HIPCHK(hipEventRecord(R.ev_eng[q], st)); HIPCHK(hipStreamWaitEvent(R.st, R.ev_eng[q], 0)); ++q; }
            for (hipStream_t st : {f->rs, f->rs2, f->os}) if (st && st != R.st) { HIPCHK(hipEventRecord(R.ev_eng.back(), st)); HIPCHK(hipStreamWaitEvent(R.st, R.ev_eng.back(), 0)); }
            MxAns S = R.an; S.m = U.m;
            hipLaunchKernelGGL(k_mx_apack, dim3((S.m + 255u) / 256u), dim3(256), 0, R.st, S);
            if (hipGetLastError() != hipSuccess) return fail(GUBER_E_HIP, "kernel launch");
        }
        HIPCHK(hipEventRecord(R.ev_ans, R.st));
    }
    // every source: its answers home, in arrival order
    for (uint32_t s = 0; s < W; ++s) {
        auto& R = m->ranks[s];
        HIPCHK(hipSetDevice(R.device));
        if (R.n) {
            { const int r2 = mesh_exchange(m, table, s, true); if (r2) return r2; }
            MxOut O{};
            O.n = R.n; O.M = R.in.M; O.ans = R.ans_recv.p;
            O.status = results[s].status; O.err = results[s].err; O.limit = results[s].limit; O.remaining = results[s].remaining; O.reset_time = results[s].reset_time;
            hipLaunchKernelGGL(k_mx_out, dim3((R.n + FR_TILE - 1u) / FR_TILE), dim3(256), 0, R.st, O);
            if (hipGetLastError() != hipSuccess) return fail(GUBER_E_HIP, "kernel launch");
        }
        HIPCHK(hipEventRecord(R.ev_done, R.st));
        R.done_recorded = true;
    }
    return 0;
}

// gens[r] -> results[r], r = 0 .. n_ranks-1: DEVICE pointers on rank r's device, requests and answers in arrival order.  Asynchronous like
// guber_front_eval_dev: returns when the answers' last hop is enqueued (guber_mesh_synchronize waits).
// rows[r].key_stride != 0: rank r's keys lie in ROWS (gens[r].key_bytes the first row, key_stride bytes apart, key_len[i] bytes of row i
// are the key; gens[r].key_off NULL) — what the device wire decoder leaves; rows NULL or key_stride 0: packed.  Every check comes
// before the first HIP call.
// forwarded: NULL, or the requests THIS call moved to another rank (the counter's step, taken under the mesh's lock)
static int mesh_eval_rows_owner(guber_mesh_t* m, const guber_batch_t* gens, const guber_mesh_rows_t* rows, guber_result_t* results, uint8_t* const* item_owner,
                                uint64_t* forwarded = nullptr) {
    if (!m || !gens || !results) return fail(GUBER_E_INVALID_ARG, "null argument");
    for (uint32_t r = 0; r < m->W; ++r) {
        int rc;
        if (rows && rows[r].key_stride) {
            if (rows[r].key_stride & 7u) return fail(GUBER_E_INVALID_ARG, "key rows are a multiple of 8 bytes apart");
            if (gens[r].key_off) return fail(GUBER_E_INVALID_ARG, "guber_mesh: key rows have no offsets (key_off must be NULL)");
            if ((uint64_t)gens[r].n * rows[r].key_stride > 0xffffffffull) return fail(GUBER_E_BATCH_TOO_LARGE, "guber_mesh: a generation of key rows exceeds 4 GB");
            const guber_batch_t& b = gens[r]; const guber_result_t& q = results[r];
            rc = 0;                                                  // (check_batch_args with key_len in key_off's place)
            if (b.n && (!b.key_bytes || !rows[r].key_len || !b.hits || !b.limit || !b.duration)) rc = fail(GUBER_E_INVALID_ARG, "batch is missing a mandatory array (key rows need key_len)");
            else if (b.n && (!q.status || !q.limit || !q.remaining || !q.reset_time || !q.err)) rc = fail(GUBER_E_INVALID_ARG, "result is missing an array");
        } else rc = check_batch_args(&gens[r], &results[r]);
        if (rc) return rc;
        if (gens[r].n > m->max_n) return fail(GUBER_E_BATCH_TOO_LARGE, "generation larger than the mesh was created for");
        if (gens[r].now_ms != gens[0].now_ms) return fail(GUBER_E_INVALID_ARG, "guber_mesh: the generations of a call carry one now_ms");
        if (gens[r].is_owner) return fail(GUBER_E_INVALID_ARG, "guber_mesh: the ring decides ownership (is_owner must be NULL)");
        if (gens[r].greg_expire || gens[r].greg_duration) return fail(GUBER_E_INVALID_ARG, "a front takes its calendar intervals from the device");
    }
    std::lock_guard<std::mutex> lk(m->mu);
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t fwd0 = m->st.forwarded;
    const int rc = mesh_eval(m, gens, rows, results, item_owner);
    if (forwarded) *forwarded = m->st.forwarded - fwd0;
    m->st.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

extern "C" int guber_mesh_eval_rows_dev(guber_mesh_t* m, const guber_batch_t* gens, const guber_mesh_rows_t* rows, guber_result_t* results) {
    return mesh_eval_rows_owner(m, gens, rows, results, nullptr);
}

extern "C" int guber_mesh_eval_dev(guber_mesh_t* m, const guber_batch_t* gens, guber_result_t* results) {
    return guber_mesh_eval_rows_dev(m, gens, nullptr, results);
}

// ---- the one-launch path: guber_mesh_eval_small (include/guber_gpu.h; the kernel: k_mx_small, guber_kernels_small.h) -------------------------
// A call of at most FT requests over all ranks together, from host memory, synchronous.  The generations are copied into ONE arena of
// pinned host memory — source rank after source rank, arrival order inside each, src_start[W + 1] — that every rank's device sees; every
// rank gets one launch on its routing stream, a workgroup per engine of its front, and the host polls the shares' completion words
// (SmallOut::done, as eval_host_once does, with its 2 s fall-back to a stream synchronisation).
// LOCKS.  Under the mesh's mutex: every front's mutex in rank order, then every engine of every rank in ADDRESS order (the rule of every
// path that holds several engines: EngineLocks).  All fronts come before any engine, as in front_eval, which holds its front's mutex when
// it asks for engines and never the other way round: a thread inside guber_front_eval_dev (or, through it, guber_mesh_eval_dev of another
// mesh) holds one front and waits for engines only, this call holds no engine while it waits for a front — so whoever this call waits
// for can finish — and between holders of several engines the address order decides.
// ARENA.  hipHostMallocPortable | Mapped | Coherent: one allocation, visible to every device of the process.  With every rank a logical
// rank of ONE device — all a one-GPU box has — the kernels of all ranks read it from the device whose context allocated it; a kernel on
// one GPU reading what another rank's caller wrote through it cannot be exercised there.
#ifndef hipHostMallocPortable
#define hipHostMallocPortable 0x1u                                  // (a header without it: the stand-in runtime of the CPU build, which has one kind of memory)
#endif
static size_t mesh_small_carve(guber_mesh* m, uint8_t* base) {
    auto& S = m->sm;
    ColCarver c{(uintptr_t)base};
    const size_t n = FT;
    S.hits = c.take<int64_t>(n); S.limit = c.take<int64_t>(n); S.duration = c.take<int64_t>(n); S.burst = c.take<int64_t>(n); S.created_at = c.take<int64_t>(n);
    S.o_limit = c.take<int64_t>(n); S.o_remaining = c.take<int64_t>(n); S.o_reset = c.take<int64_t>(n);
    S.key_off = c.take<uint32_t>(n + 1); S.behavior = c.take<uint32_t>(n); S.where = c.take<uint32_t>(n);
    S.src_start = c.take<uint32_t>(MULTI_MEM_MAX + 1); S.taken = c.take<uint32_t>((size_t)MULTI_MEM_MAX * MULTI_MEM_MAX);
    S.algorithm = c.take<uint8_t>(n); S.own = c.take<uint8_t>(n); S.o_status = c.take<uint8_t>(n); S.o_err = c.take<uint8_t>(n);
    S.outs = c.take<uint8_t>((size_t)MULTI_MEM_MAX * MULTI_MEM_MAX * 64);            // a SmallOut per (rank, engine), a line each
    S.keys = c.take<uint8_t>(n * S.key_cap + 16);
    return (size_t)(c.at - (uintptr_t)base);
}
// the bytes of the wholesale fall-back's device copy of one rank's generation: the arena's request and answer columns for FT requests
struct MeshSmallGen {
    int64_t *hits, *limit, *duration, *burst, *created_at, *o_limit, *o_remaining, *o_reset; uint32_t *key_off, *behavior; uint8_t *algorithm, *o_status, *o_err, *item_owner, *keys;
};
static size_t mesh_small_gen_carve(const guber_mesh* m, uint8_t* base, MeshSmallGen& G) {
    ColCarver c{(uintptr_t)base};
    const size_t n = FT;
    G.hits = c.take<int64_t>(n); G.limit = c.take<int64_t>(n); G.duration = c.take<int64_t>(n); G.burst = c.take<int64_t>(n); G.created_at = c.take<int64_t>(n);
    G.o_limit = c.take<int64_t>(n); G.o_remaining = c.take<int64_t>(n); G.o_reset = c.take<int64_t>(n);
    G.key_off = c.take<uint32_t>(n + 1); G.behavior = c.take<uint32_t>(n);
    G.algorithm = c.take<uint8_t>(n); G.o_status = c.take<uint8_t>(n); G.o_err = c.take<uint8_t>(n); G.item_owner = c.take<uint8_t>(n);
    G.keys = c.take<uint8_t>(n * m->sm.key_cap + 16);
    return (size_t)(c.at - (uintptr_t)base);
}
static int mesh_small_ensure(guber_mesh* m) {
    auto& S = m->sm;
    if (S.ready) return 0;
    const uint32_t W = m->W;
    uint32_t max_key = 0;
    for (auto& R : m->ranks) max_key = std::max(max_key, R.max_key);
    S.key_cap = max_key + 1u;                                        // (a key above every rank's max_key_bytes travels as max_key + 1 bytes: it only ever earns its item error)
    if (!S.arena) {
        HIPCHK(hipSetDevice(m->ranks[0].device));
        void* p = nullptr;
        if (hipHostMalloc(&p, mesh_small_carve(m, nullptr), hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return fail(GUBER_E_NOMEM, "guber_mesh: the one-launch path's arena");
        S.arena = (uint8_t*)p;
        mesh_small_carve(m, S.arena);
    }
    S.ranks.resize(W);
    std::vector<uint32_t> mk(W);
    for (uint32_t r = 0; r < W; ++r) mk[r] = m->ranks[r].max_key;
    for (uint32_t r = 0; r < W; ++r) {
        auto& R = m->ranks[r]; auto& P = S.ranks[r];
        HIPCHK(hipSetDevice(R.device));
        if (P.src_max.ensure(W) || R.ring_h.ensure(m->npts) || R.ring_o.ensure(m->npts)) return GUBER_E_NOMEM;
        HIPCHK(hipMemcpyAsync(P.src_max.p, mk.data(), (size_t)W * 4, hipMemcpyHostToDevice, R.st));
        if (W == 1) {                                                // (a mesh of one rank keeps no ring on the device: the one-launch kernel searches it all the same)
            HIPCHK(hipMemcpyAsync(R.ring_h.p, m->ring_hh.data(), (size_t)m->npts * 8, hipMemcpyHostToDevice, R.st));
            HIPCHK(hipMemcpyAsync(R.ring_o.p, m->ring_o8.data(), m->npts, hipMemcpyHostToDevice, R.st));
        }
        while (P.ev.size() < R.f->streams.size()) { hipEvent_t ev = nullptr; HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); P.ev.push_back(ev); }
        HIPCHK(hipStreamSynchronize(R.st));
    }
    S.ready = true;
    return 0;
}
// the generations into the arena: source after source, arrival order; -> the call's total
static uint32_t mesh_small_fill(guber_mesh* m, const guber_batch_t* gens) {
    auto& S = m->sm;
    uint32_t t = 0, koff = 0;
    for (uint32_t r = 0; r < m->W; ++r) {
        const guber_batch_t& b = gens[r];
        S.src_start[r] = t;
        for (uint32_t i = 0; i < b.n; ++i, ++t) {
            const uint32_t len = std::min(b.key_off[i + 1] - b.key_off[i], S.key_cap);
            memcpy(S.keys + koff, b.key_bytes + b.key_off[i], len);
            S.key_off[t] = koff; koff += len;
            S.hits[t] = b.hits[i]; S.limit[t] = b.limit[i]; S.duration[t] = b.duration[i];
            S.burst[t] = b.burst ? b.burst[i] : 0;
            S.created_at[t] = b.created_at ? b.created_at[i] : b.now_ms;      // (gubernator.go:218-220, as k_mx_pack: the arrival rank's clock)
            S.behavior[t] = b.behavior ? b.behavior[i] : 0u; S.algorithm[t] = b.algorithm ? b.algorithm[i] : (uint8_t)0;
            S.own[t] = 1; S.where[t] = 0xffffffffu;
        }
    }
    for (uint32_t r = m->W; r <= (uint32_t)MULTI_MEM_MAX; ++r) S.src_start[r] = t;
    S.key_off[t] = koff;
    memset(S.keys + koff, 0, 16);                                    // (keys are read as 8-byte words: the bytes behind the last key are defined)
    return t;
}
// the answers (the arena's result columns) and, where wanted, the ring's owners to the caller's arrays
static void mesh_small_copy_out(guber_mesh* m, const guber_batch_t* gens, guber_result_t* results, uint8_t* const* owner_rank, const uint8_t* owners) {
    auto& S = m->sm;
    for (uint32_t r = 0; r < m->W; ++r) {
        const uint32_t t0 = S.src_start[r], n = gens[r].n;
        if (!n) continue;
        guber_result_t& q = results[r];
        memcpy(q.status, S.o_status + t0, n); memcpy(q.err, S.o_err + t0, n);
        memcpy(q.limit, S.o_limit + t0, (size_t)n * 8); memcpy(q.remaining, S.o_remaining + t0, (size_t)n * 8); memcpy(q.reset_time, S.o_reset + t0, (size_t)n * 8);
        if (owner_rank && owner_rank[r]) memcpy(owner_rank[r], owners + t0, n);
    }
}
// the wholesale fall-back: the arena's generations through mesh_eval on device copies (no lock but the mesh's is held)
static int mesh_small_general(guber_mesh* m, const guber_batch_t* gens, guber_result_t* results, uint8_t* const* owner_rank, int64_t now_ms) {
    auto& S = m->sm;
    const uint32_t W = m->W;
    std::vector<guber_batch_t> db(W); std::vector<guber_result_t> dr(W); std::vector<MeshSmallGen> G(W); std::vector<uint8_t*> io(W, nullptr);
    const bool want_owner = owner_rank != nullptr && W > 1;         // (one rank: the ring has one peer, the host says who)
    for (uint32_t r = 0; r < W; ++r) {
        auto& R = m->ranks[r]; auto& P = S.ranks[r];
        const uint32_t t0 = S.src_start[r], n = gens[r].n;
        db[r] = guber_batch_t{}; dr[r] = guber_result_t{};
        db[r].now_ms = now_ms;
        if (!n) continue;
        HIPCHK(hipSetDevice(R.device));
        MeshSmallGen sz{};
        if (P.gen.ensure(mesh_small_gen_carve(m, nullptr, sz))) return GUBER_E_NOMEM;
        mesh_small_gen_carve(m, P.gen.p, G[r]);
        const MeshSmallGen& g = G[r];
        const uint32_t k0 = S.key_off[t0], k1 = S.key_off[t0 + n];
        // (the offsets stay the arena's: the keys go to the same places of the copy)
        HIPCHK(hipMemcpyAsync(g.keys + k0, S.keys + k0, (size_t)(k1 - k0) + 8, hipMemcpyHostToDevice, R.st));
        HIPCHK(hipMemcpyAsync(g.key_off, S.key_off + t0, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, R.st));
        HIPCHK(hipMemcpyAsync(g.hits, S.hits + t0, (size_t)n * 8, hipMemcpyHostToDevice, R.st));
        HIPCHK(hipMemcpyAsync(g.limit, S.limit + t0, (size_t)n * 8, hipMemcpyHostToDevice, R.st));
        HIPCHK(hipMemcpyAsync(g.duration, S.duration + t0, (size_t)n * 8, hipMemcpyHostToDevice, R.st));
        HIPCHK(hipMemcpyAsync(g.burst, S.burst + t0, (size_t)n * 8, hipMemcpyHostToDevice, R.st));
        HIPCHK(hipMemcpyAsync(g.created_at, S.created_at + t0, (size_t)n * 8, hipMemcpyHostToDevice, R.st));
        HIPCHK(hipMemcpyAsync(g.behavior, S.behavior + t0, (size_t)n * 4, hipMemcpyHostToDevice, R.st));
        HIPCHK(hipMemcpyAsync(g.algorithm, S.algorithm + t0, n, hipMemcpyHostToDevice, R.st));
        HIPCHK(hipStreamSynchronize(R.st));                          // (the front may route on another stream)
        guber_batch_t& b = db[r];
        b.n = n; b.key_bytes = g.keys; b.key_off = g.key_off; b.hits = g.hits; b.limit = g.limit; b.duration = g.duration; b.burst = g.burst; b.created_at = g.created_at;
        b.behavior = g.behavior; b.algorithm = g.algorithm;
        dr[r].status = g.o_status; dr[r].err = g.o_err; dr[r].limit = g.o_limit; dr[r].remaining = g.o_remaining; dr[r].reset_time = g.o_reset;
        if (want_owner) io[r] = g.item_owner;
    }
    { const int rc = mesh_eval(m, db.data(), nullptr, dr.data(), want_owner ? io.data() : nullptr); if (rc) return rc; }
    std::vector<uint8_t> owners(FT, 0);
    for (uint32_t r = 0; r < W; ++r) {
        auto& R = m->ranks[r];
        const uint32_t t0 = S.src_start[r], n = gens[r].n;
        if (!n) continue;
        { const int rc = guber_front_synchronize(R.f); if (rc) return rc; }
        HIPCHK(hipSetDevice(R.device));
        HIPCHK(hipStreamSynchronize(R.st));
        const MeshSmallGen& g = G[r];
        HIPCHK(hipMemcpy(S.o_status + t0, g.o_status, n, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(S.o_err + t0, g.o_err, n, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(S.o_limit + t0, g.o_limit, (size_t)n * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(S.o_remaining + t0, g.o_remaining, (size_t)n * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(S.o_reset + t0, g.o_reset, (size_t)n * 8, hipMemcpyDeviceToHost));
        if (want_owner) HIPCHK(hipMemcpy(owners.data() + t0, g.item_owner, n, hipMemcpyDeviceToHost));
        else for (uint32_t i = 0; i < n; ++i) { const uint32_t len = S.key_off[t0 + i + 1] - S.key_off[t0 + i]; owners[t0 + i] = (len == 0 || len > R.max_key) ? (uint8_t)0xffu : (uint8_t)0; }
    }
    mesh_small_copy_out(m, gens, results, owner_rank, owners.data());
    return 0;
}

static int mesh_eval_small_locked(guber_mesh* m, const guber_batch_t* gens, guber_result_t* results, uint8_t* const* owner_rank, uint32_t total) {
    auto& S = m->sm;
    const uint32_t W = m->W;
    const int64_t now_ms = gens[0].now_ms;
    if (total == 0) { m->st.calls++; return 0; }
    { const int rc = mesh_small_ensure(m); if (rc) return rc; }
    mesh_small_fill(m, gens);
    // every front, then every engine in address order (LOCKS above)
    std::vector<std::unique_lock<std::mutex>> held;
    std::vector<guber_engine*> engs;
    for (auto& R : m->ranks) { held.emplace_back(R.f->mu); for (guber_engine* e : R.f->eng) engs.push_back(e); }
    std::sort(engs.begin(), engs.end());
    for (guber_engine* e : engs) held.emplace_back(e->mu);
    bool small_ok = true;
    for (auto& R : m->ranks) small_ok = small_ok && !R.f->st.probed && !R.f->pre_routed && R.f->eng.size() <= (size_t)MULTI_MEM_MAX;
    for (guber_engine* e : engs) {
        if (e->set_device()) return fail(GUBER_E_HIP, "hipSetDevice");       // (a k_eval3 another call holds back for this table goes first)
        if (e->small_pending) { const int r2 = resolve_small_locked(e->small_pending, true, e); if (r2 < 0) return r2; }
        small_ok = small_ok && !e->no_small && !e->careful && !lru_may_bind(e, total);
    }
    if (!small_ok) {
        S.st.calls++; S.st.wholesale_fallbacks++;
        while (!held.empty()) held.pop_back();                       // (the general path takes the fronts' and the engines' locks where front_eval takes them)
        return mesh_small_general(m, gens, results, owner_rank, now_ms);
    }
    // small_prelude's work per engine, with the call's total as the bound of a share nobody knows yet (batches / small_batches move below,
    // for the engines that got a request)
    BatchView BH{};
    BH.n = total; BH.key_bytes = S.keys; BH.key_off = S.key_off; BH.hits = S.hits; BH.limit = S.limit; BH.duration = S.duration; BH.burst = S.burst; BH.created_at = S.created_at;
    BH.algorithm = S.algorithm; BH.behavior = S.behavior; BH.is_owner = S.own; BH.now_ms = now_ms;
    for (guber_engine* e : engs) {
        if (e->set_device()) return fail(GUBER_E_HIP, "hipSetDevice");
        if (now_ms > e->clock_ms) e->clock_ms = now_ms;
        ArenaHint hint(e, host_arena_bytes(e, S.key_off, total));
        const uint64_t ab = batch_arena_bytes(e, BH);
        const int rc = maintain(e, total, now_ms, false, nullptr, ab);
        if (rc) return rc;                                           // (nothing has been launched)
        note_enqueued(e, total, ab);
        take_stamps(e, total);
    }
    // (from here on the call is taken: nothing above that can fail has moved a statistic)
    m->st.calls++; m->st.requests += total; S.st.calls++;
    if (++S.seq == 0) S.seq = 1;
    // one launch per rank, behind everything enqueued on its engines' streams.  An error part-way: the ranks already launched are waited
    // for before the locks go — their kernels write the arena and the engines' tables
    uint32_t launched = 0;
    auto drain = [&](int rc) { for (uint32_t q = 0; q < launched; ++q) if (hipSetDevice(m->ranks[q].device) == hipSuccess) (void)hipStreamSynchronize(m->ranks[q].st); return rc; };
    for (uint32_t r = 0; r < W; ++r) {
        auto& R = m->ranks[r]; auto& P = S.ranks[r];
        guber_front* f = R.f;
        if (hipSetDevice(R.device) != hipSuccess) return drain(fail(GUBER_E_HIP, "hipSetDevice"));
        for (size_t q = 0; q < f->streams.size(); ++q)
            if (f->streams[q] != R.st && (hipEventRecord(P.ev[q], f->streams[q]) != hipSuccess || hipStreamWaitEvent(R.st, P.ev[q], 0) != hipSuccess))
                return drain(fail(GUBER_E_HIP, "guber_mesh: the engines' streams in front of a small launch"));
        MxSmall A{};
        A.n_total = total; A.self = r; A.world = W; A.n_engines = (uint32_t)f->eng.size(); A.npts = m->npts; A.kind = m->kind; A.front_max_key = f->max_key;
        A.src_start = S.src_start; A.src_max_key = P.src_max.p; A.ring_hash = R.ring_h.p; A.ring_owner = R.ring_o.p;
        A.B = BH; A.R = ResultView{S.o_status, S.o_limit, S.o_remaining, S.o_reset, S.o_err};
        A.where = S.where; A.own = S.own; A.taken = S.taken + (size_t)r * MULTI_MEM_MAX; A.rule = f->rule;
        for (uint32_t j = 0; j < A.n_engines; ++j) {
            guber_engine* e = f->eng[j];
            SmallOut* out = (SmallOut*)(S.outs + ((size_t)r * MULTI_MEM_MAX + j) * 64);
            out->done = 0; A.taken[j] = 0xffffffffu;
            A.sub[j] = MxSmallSub{e->T, out, e->touch, S.seq, 0u};
        }
        hipLaunchKernelGGL(k_mx_small, dim3(A.n_engines), dim3(FT), 0, R.st, A);
        if (hipGetLastError() != hipSuccess) return drain(fail(GUBER_E_HIP, "kernel launch"));
        S.st.launches++; ++launched;
    }
    // wait for every share's word
    for (uint32_t r = 0; r < W; ++r) {
        auto& R = m->ranks[r];
        for (size_t j = 0; j < R.f->eng.size(); ++j) {
            volatile unsigned int* flag = &((SmallOut*)(S.outs + ((size_t)r * MULTI_MEM_MAX + j) * 64))->done;
            const auto t0 = std::chrono::steady_clock::now();
            uint32_t spins = 0;
            while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != S.seq) {
                if ((++spins & 0x3ff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) { HIPCHK(hipSetDevice(R.device)); HIPCHK(hipStreamSynchronize(R.st)); break; }
            }
        }
    }
    // where[] names exactly one taker per request: a valid (rank, engine) each, and as many per taker as it says it took
    uint32_t cnt[MULTI_MEM_MAX][MULTI_MEM_MAX] = {};
    uint64_t forwarded = 0;
    std::vector<uint8_t> owners(FT, 0);
    for (uint32_t t = 0, s = 0; t < total; ++t) {
        while (S.src_start[s + 1] <= t) ++s;
        const uint32_t w = S.where[t], o = w & 0xffu, j = w >> 8 & 0xffu;
        if (w == 0xffffffffu || o >= W || j >= m->ranks[o].f->eng.size()) return fail(GUBER_E_HIP, "guber_mesh: a request of a small call found no taker");
        cnt[o][j]++; owners[t] = (uint8_t)(w >> 16);
        forwarded += o != s;
    }
    for (uint32_t r = 0; r < W; ++r)
        for (size_t j = 0; j < m->ranks[r].f->eng.size(); ++j)
            if (S.taken[(size_t)r * MULTI_MEM_MAX + j] != cnt[r][j]) return fail(GUBER_E_HIP, "guber_mesh: a request of a small call was taken twice");
    m->st.forwarded += forwarded;
    // the shares' counters into their engines; a declined share through the general pipeline, by index list
    guber_batch_t hb{};
    hb.n = total; hb.key_bytes = S.keys; hb.key_off = S.key_off; hb.hits = S.hits; hb.limit = S.limit; hb.duration = S.duration; hb.burst = S.burst; hb.created_at = S.created_at;
    hb.algorithm = S.algorithm; hb.behavior = S.behavior; hb.is_owner = S.own; hb.now_ms = now_ms;
    guber_result_t hr{};
    hr.status = S.o_status; hr.err = S.o_err; hr.limit = S.o_limit; hr.remaining = S.o_remaining; hr.reset_time = S.o_reset;
    for (uint32_t r = 0; r < W; ++r) {
        guber_front* f = m->ranks[r].f;
        for (uint32_t j = 0; j < (uint32_t)f->eng.size(); ++j) {
            guber_engine* e = f->eng[j];
            const SmallOut* out = (const SmallOut*)(S.outs + ((size_t)r * MULTI_MEM_MAX + j) * 64);
            if (!out->fallback) {
                small_fold(e, out);
                if (cnt[r][j]) { e->batches++; e->small_batches++; }
            } else {
                e->small_fallbacks++; S.st.share_fallbacks++;
                std::vector<uint32_t> idx;
                for (uint32_t t = 0; t < total; ++t) if ((S.where[t] & 0xffffu) == (r | j << 8)) idx.push_back(t);
                if (e->set_device()) return fail(GUBER_E_HIP, "hipSetDevice");
                // (two new keys under one 64-bit hash inside the share: the careful rounds, as eval_batch_host_locked runs them)
                for (uint32_t round = 0; round < 64 + 2 * total && !idx.empty(); ++round) {
                    e->careful = round != 0;
                    const int rc = eval_host_once(e, &hb, &hr, idx.data(), (uint32_t)idx.size(), nullptr);
                    e->careful = false;
                    if (rc) return rc;
                    std::vector<uint32_t> again;
                    for (uint32_t t : idx) if (hr.err[t] == GUBER_ITEM_E_RETRY) again.push_back(t);
                    idx.swap(again);
                }
            }
            if (cnt[r][j]) { if (e->set_device()) return fail(GUBER_E_HIP, "hipSetDevice"); const int rc = maintain(e, 0, now_ms); if (rc) return rc; }
        }
    }
    mesh_small_copy_out(m, gens, results, owner_rank, owners.data());
    return 0;
}

// forwarded / fallbacks: NULL, or what THIS call moved to another rank / how many fall-backs of either kind it met (the counters' steps,
// taken under the mesh's lock)
static int mesh_eval_small_counted(guber_mesh_t* m, const guber_batch_t* gens, guber_result_t* results, uint8_t* const* owner_rank, uint64_t* forwarded, uint64_t* fallbacks) {
    if (!m || !gens || !results) return fail(GUBER_E_INVALID_ARG, "null argument");
    uint64_t total = 0;
    for (uint32_t r = 0; r < m->W; ++r) {
        const int rc = check_batch_args(&gens[r], &results[r]);
        if (rc) return rc;
        if (gens[r].n > m->max_n) return fail(GUBER_E_BATCH_TOO_LARGE, "generation larger than the mesh was created for");
        if (gens[r].now_ms != gens[0].now_ms) return fail(GUBER_E_INVALID_ARG, "guber_mesh: the generations of a call carry one now_ms");
        if (gens[r].is_owner) return fail(GUBER_E_INVALID_ARG, "guber_mesh: the ring decides ownership (is_owner must be NULL)");
        if (gens[r].greg_expire || gens[r].greg_duration) return fail(GUBER_E_INVALID_ARG, "a front takes its calendar intervals from the device");
        total += gens[r].n;
    }
    if (total > (uint64_t)FT) return fail(GUBER_E_BATCH_TOO_LARGE, "guber_mesh: a small call holds at most 256 requests over all ranks");
    for (uint32_t r = 0; r < m->W; ++r) clear_aggregates(results[r]);
    std::lock_guard<std::mutex> lk(m->mu);
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t fwd0 = m->st.forwarded, fb0 = m->sm.st.wholesale_fallbacks + m->sm.st.share_fallbacks;
    const int rc = mesh_eval_small_locked(m, gens, results, owner_rank, (uint32_t)total);
    if (forwarded) *forwarded = m->st.forwarded - fwd0;
    if (fallbacks) *fallbacks = m->sm.st.wholesale_fallbacks + m->sm.st.share_fallbacks - fb0;
    m->st.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}
extern "C" int guber_mesh_eval_small(guber_mesh_t* m, const guber_batch_t* gens, guber_result_t* results, uint8_t* const* owner_rank) {
    return mesh_eval_small_counted(m, gens, results, owner_rank, nullptr, nullptr);
}

extern "C" int guber_mesh_small_stats(guber_mesh_t* m, guber_mesh_small_stats_t* out) {
    if (!m || !out) return fail(GUBER_E_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    *out = m->sm.st;
    return GUBER_OK;
}

extern "C" int guber_mesh_synchronize(guber_mesh_t* m) {
    if (!m) return fail(GUBER_E_INVALID_ARG, "null mesh");
    std::lock_guard<std::mutex> lk(m->mu);
    for (auto& R : m->ranks) {
        const int rc = guber_front_synchronize(R.f);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(R.st));                          // (the answers' last hop: the stream the mesh was created on)
    }
    return GUBER_OK;
}

extern "C" int guber_mesh_stats(guber_mesh_t* m, guber_mesh_stats_t* out) {
    if (!m || !out) return fail(GUBER_E_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    *out = m->st;
    return GUBER_OK;
}
