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
