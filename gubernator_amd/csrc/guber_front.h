// guber_front.h — guber_front_*: a generation of requests in ARRIVAL order, resident in HBM -> routed to the GPU's logical shards on
// the device -> evaluated by the fused pipelines -> answered in ARRIVAL order.  Part of guber_engine.hip's translation unit (it uses
// the dispatcher's internals: launch_group, PendSet, the engines' locks).
//
// Reference: WorkerPool.GetRateLimit picks a request's worker from the XXH64 of its HashKey (workers.go:261-289, getWorker :180-184)
// and V1Instance.GetRateLimits answers in request order (gubernator.go:203-300, gubernator.proto:51-54).  guber_eval_batches_routed_dev
// takes batches that somebody has already split by shard and leaves the answers in the shards' order; this is the whole of it.
//
// One generation g (slot = g mod depth):
//   routing stream g mod 2   k_fr_count(g)  k_fr_scan(g)  k_fr_scatter(g)  [event in(g)]
//   engine streams                                             wait in(g) | the shares as batches of the fused pipelines | [event done(g, s)]
//   answers' stream                                                                                              wait done(g, *) | k_fr_out(g) [event out(g)]
// The routing runs ahead of the evaluation (two generations), so the shares' sizes — which the host needs to size the launches and to
// keep the bounded caches' admission exact — are in pinned memory by the time the host asks: it never waits for the GPU in steady state.
#pragma once
#include "guber_kernels_wire.h"    // guber::WireEnc / k_wire_enc: the payload stage's form of the answers' last hop (front_out)

// generations of at most this many requests whose tables share ONE stream go as one pair of launches for all tables (launch_group_mem);
// larger ones keep the owner-partitioned pipeline in groups of four tables, whose advantage grows with the share.
// Measured on the payload stage, eight tables, alternating on one box (profiles/r06_wire_pool.txt): generations of 28 000 requests +16 %,
// of 40 000 +5 ... +10 %, of 57 000 -8 %.
constexpr uint32_t FRONT_ONE_PAIR_MAX = 49152;
struct guber_front {
    // Lock order: fronts' mutexes first (a mesh takes its ranks' in rank order), then engines' in ADDRESS order (EngineLocks; guber_mesh_eval_small
    // takes every front's and then every engine's that way).  guber_front_rebalance holds this mutex over its whole pass and takes engines only
    // through EngineLocks and guber_move_items_by_hash, which takes its two in address order: it fits in.
    std::mutex mu;
    int device = 0;
    std::vector<guber_engine*> eng;
    std::vector<hipStream_t> streams;                 // the engines' distinct streams
    std::vector<int> stream_of;                       // engine -> index into streams
    // ONE stream of the front's own: the routing (k_fr_count, k_fr_scan, k_fr_scatter).  The answers' last hop (k_fr_out) rides on the
    // engines' streams, generation by generation in turn: measured on one box (profiles/r06_front_streams.txt), with it behind the routing
    // on the same stream the routing stream was the pipeline's bottleneck (it also stalled on every generation's evaluation) and the
    // engines' streams idled two fifths of the time: 4.36 -> 5.7 G decisions/s at 8 batches per generation, 5.93 -> 6.2 at 16.  More
    // streams of its own (answers, a second routing stream: GUBER_FRONT_STREAMS=2|3 in the laboratory build) lose 5 - 10 %: the HIP
    // runtime maps streams onto four hardware queues, a fifth stream shares one (and GPU_MAX_HW_QUEUES=8 halves the rate).
    const guber::WireEnc* enc_hook = nullptr;         // set around a front_eval call by the payload stage: k_wire_enc in k_fr_out's place (front_out)
    // fwd[] (arrival position -> place in the shares) has ONE reader, k_wire_enc: k_fr_scatter writes it only for a front whose answers
    // go through the encoder.  The payload stage says so before it routes anything through the front (guber_wire_dev.h); never cleared.
    std::atomic<bool> want_fwd{false};
    hipStream_t rs = nullptr, rs2 = nullptr, os = nullptr, last_os = nullptr; int n_own_streams = 1; bool out_on_eval = false; uint32_t out_delay = 0, one_pair_max = FRONT_ONE_PAIR_MAX; bool rs_borrowed = false;
    uint32_t cap = 0, depth = 0, max_key = 0;
    uint32_t seq = 0;
    DevBuf<uint16_t> rt_table, rt_exs; DevBuf<uint64_t> rt_exh; RouteRule rule{}; bool have_rule = false;
    struct Slot {
        DevBuf<uint8_t> mem; CohBuf<FrontHost> host;
        FrIn in{};
        uint32_t* fwd = nullptr;                        // the mirror's fwd column (FrIn::d_fwd of a generation routed with want_fwd)
        uint8_t *o_status = nullptr, *o_err = nullptr; int64_t *o_limit = nullptr, *o_remaining = nullptr, *o_reset = nullptr;
        hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_a = nullptr; bool out_recorded = false;
        std::vector<std::unique_ptr<EvalHook>> hooks;   // one per engine stream
        CohBuf<uint8_t> h_margs; DevBuf<uint8_t> d_margs; // the argument blocks of a generation that goes as ONE pair of launches (launch_group_mem)
        uint32_t seq = 0, n = 0;
        int64_t gen = -1;                               // the generation the slot holds (-1: free)
        bool dispatched = false;
    };
    std::vector<Slot> slots;
    uint64_t generations = 0, forced_flushes = 0, host_waits = 0; double host_wait_ms = 0;
    bool pre_routed = false;                          // front_route_ahead has routed the next call's first generation already
    // with the first engine's per-kernel timing on (guber_profile_enable): every generation's way through the GPU, first routing kernel's
    // start -> the answers' last hop's end (guber_front_latencies)
    struct GenSpan { hipEvent_t a, b; };
    std::vector<GenSpan> gen_spans;
    // The Store side channel (guber_front_probe_missing_dev / guber_front_eval_store_dev), allocated by the first store call: the election
    // table and the ask list of guber_kernels_front_store.h, the events in the shares' order (what the evaluation kernels write: cap
    // bytes + cap x 64) and in arrival order (what k_fr_out_store leaves for the host).
    struct StoreSide {
        uint32_t cap = 0, cells = 0;
        DevBuf<unsigned long long> tag; DevBuf<uint32_t> first, cell, tile_cnt, index; DevBuf<uint8_t> ask, engine, flags, oflags; DevBuf<Rec> after, oafter;
        DevBuf<FrStoreCtl> ctl; DevBuf<FrStoreTabs> tabs; FrStoreTabs h_tabs{}; FrStoreCtl h_ctl{};
        std::vector<hipEvent_t> ev;                   // one per engine stream: the routing stream reads the tables behind what is enqueued there
        bool probed = false, active = false;          // probed: the next slot holds a probed, unevaluated generation; active: guber_front_eval_store_dev is evaluating it
        uint32_t n = 0, cut_at = 0; const void *key_bytes = nullptr, *key_off = nullptr; int64_t now_ms = 0;
        uint64_t probes = 0, collisions = 0, cuts = 0, asked = 0, evals = 0;
    } st;
    // The observation window (guber_front_observe / guber_front_observation / guber_front_rebalance; guber_kernels_front_observe.h), allocated
    // by the first guber_front_observe(f, every > 0): the candidate table, the slots' words, the striped totals and the compaction's counter in
    // ONE allocation (cleared by one memset at a window's end), and the pinned memory k_fr_observe_top reports into.
    struct Observe {
        uint32_t every = 0, since = 0, n_slots = 0, seq = 0; bool no_agg = false;
        bool ahead_counted = false;                    // the generation routed ahead took its turn in "every k-th" when it was routed
        bool skip_one = false;                         // ... and a pass dropped it: the call that routes it again does not count it again
        DevBuf<uint8_t> mem; size_t mem_bytes = 0; FrObsCell* cell = nullptr; uint32_t* slot_w = nullptr; FrObsTot* tot = nullptr; uint32_t* n_top = nullptr;
        CohBuf<uint8_t> host; CohBuf<FrontHost> word;
        unsigned long long *h_hash = nullptr, *h_tot = nullptr; uint32_t *h_count = nullptr, *h_slot_w = nullptr;
        uint64_t generations = 0;                      // the window's
    } ob;
};

static size_t front_col(size_t bytes) { return (bytes + 63) & ~(size_t)63; }
// An arena of columns, each starting on a 64-byte line: take<T>(n) is the next one.  A carve from 0 gives the arena's size in `at`.
struct ColCarver {
    uintptr_t at;
    template <class T> T* take(size_t n) { T* p = (T*)at; at += front_col(n * sizeof(T)); return p; }
};
// the routing scratch of generations of at most max_n requests (RouteMap, guber_kernels_front.h); `host` is pinned memory of its own
static RouteMap route_carve(ColCarver& c, size_t max_n, FrontHost* host) {
    const size_t tiles = (max_n + FR_TILE - 1) / FR_TILE;
    RouteMap M{};
    M.er = c.take<uint16_t>(max_n);
    M.tile_cnt = c.take<uint32_t>(tiles * MULTI_MEM_MAX); M.tile_base = c.take<uint32_t>(tiles * MULTI_MEM_MAX);
    M.ctl = c.take<FrontCtl>(1); M.host = host;
    return M;
}
// Have all `nwords` words of the routing's report reached host memory?  Every word carries the generation's seq in its upper half
// (FrontHost): the front waits for 17, the sixteen share sizes and the key-width word, the mesh for 16.
static bool route_reported(const FrontHost* h, uint32_t nwords, uint32_t seq) {
    for (uint32_t q = 0; q < nwords; ++q)
        if ((uint32_t)(__atomic_load_n((volatile const unsigned long long*)&h->w[q], __ATOMIC_ACQUIRE) >> 32) != seq) return false;
    return true;
}
// Spins, then yields, until they have; every 1 024 yields it asks whether the routing's stream has run dry without them: `what` is the error
static int route_wait_reported(const FrontHost* h, uint32_t nwords, uint32_t seq, int device, hipStream_t st, const char* what) {
    uint32_t spins = 0;
    while (!route_reported(h, nwords, seq)) {
        if (++spins <= 2000) continue;
        std::this_thread::yield();
        if ((spins & 0x3ffu) != 0) continue;
        if (hipSetDevice(device) != hipSuccess) return fail(GUBER_E_HIP, "hipSetDevice");
        if (hipStreamQuery(st) != hipErrorNotReady && !route_reported(h, nwords, seq)) return fail(GUBER_E_HIP, what);
    }
    return 0;
}
// a generation as the front's internals see it: the caller's guber_batch_t, or columns whose keys are rows (the device wire decoder's output)
struct FrontGen { guber_batch_t b; uint32_t key_stride = 0; const uint32_t* key_len = nullptr; };

extern "C" void guber_front_destroy(guber_front_t* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    for (hipStream_t st : {f->rs, f->rs2, f->os}) if (st) (void)hipStreamSynchronize(st);
    for (auto st : f->streams) (void)hipStreamSynchronize(st);
    for (auto& s : f->slots) {
        s.mem.release(); s.host.release(); s.h_margs.release(); s.d_margs.release();
        if (s.ev_in) (void)hipEventDestroy(s.ev_in);
        if (s.ev_out) (void)hipEventDestroy(s.ev_out);
        for (auto& h : s.hooks) if (h && h->ev) (void)hipEventDestroy(h->ev);
    }
    {
        auto& t = f->st;
        t.tag.release(); t.first.release(); t.cell.release(); t.tile_cnt.release(); t.index.release(); t.ask.release(); t.engine.release();
        t.flags.release(); t.oflags.release(); t.after.release(); t.oafter.release(); t.ctl.release(); t.tabs.release();
        for (auto ev : t.ev) if (ev) (void)hipEventDestroy(ev);
    }
    f->ob.mem.release(); f->ob.host.release(); f->ob.word.release();
    f->rt_table.release(); f->rt_exs.release(); f->rt_exh.release();
    if (f->rs2 && f->rs2 != f->rs) (void)hipStreamDestroy(f->rs2);
    if (f->os && f->os != f->rs) (void)hipStreamDestroy(f->os);
    if (f->rs && !f->rs_borrowed) (void)hipStreamDestroy(f->rs);
    delete f;
}

static int front_set_rule(guber_front* f, const guber_route_rule_t* rule) {
    if (rule->n_shards == 0 || rule->per == 0 || !rule->table || rule->n_shards > 4096 || (rule->ex_cells & (rule->ex_cells - 1)) ||
        (rule->ex_n && (!rule->ex_hash || !rule->ex_shard || rule->ex_n >= rule->ex_cells)))
        return fail(GUBER_E_INVALID_ARG, "malformed route rule");
    const size_t slots = (size_t)rule->n_shards * rule->per, cells = rule->ex_cells ? rule->ex_cells : 1;
    if (f->rt_table.ensure(slots) || f->rt_exh.ensure(cells) || f->rt_exs.ensure(cells)) return GUBER_E_NOMEM;
    hipError_t he = hipStreamSynchronize(f->rs);                     // (launches still reading the previous rule)
    if (he == hipSuccess && f->rs2) he = hipStreamSynchronize(f->rs2);
    if (he == hipSuccess) he = hipMemcpy(f->rt_table.p, rule->table, slots * 2, hipMemcpyHostToDevice);
    if (he == hipSuccess && rule->ex_n) he = hipMemcpy(f->rt_exh.p, rule->ex_hash, cells * 8, hipMemcpyHostToDevice);
    if (he == hipSuccess && rule->ex_n) he = hipMemcpy(f->rt_exs.p, rule->ex_shard, cells * 2, hipMemcpyHostToDevice);
    if (he != hipSuccess) { f->have_rule = false; return fail(GUBER_E_HIP, "guber_front: rule upload", he); }
    f->rule = RouteRule{rule->n_shards, rule->per, rule->ex_cells, rule->ex_n, rule->global_engine, rule->step, rule->inv_step, rule->inv_sub,
                        f->rt_table.p, (const unsigned long long*)f->rt_exh.p, f->rt_exs.p};
    f->have_rule = true;
    return 0;
}

extern "C" int guber_front_create(guber_engine_t* const* engines, uint32_t n_engines, const guber_route_rule_t* rule, uint32_t max_n,
                                  uint32_t depth, guber_front_t** out) {
    if (!engines || !out || !n_engines || n_engines > (uint32_t)MULTI_MEM_MAX) return fail(GUBER_E_INVALID_ARG, "1 .. 16 engines per front");
    if (n_engines > 1 && !rule) return fail(GUBER_E_INVALID_ARG, "a front over several engines needs the placement's rule");
    if (max_n == 0 || max_n > FR_MAX_N) return fail(GUBER_E_BATCH_TOO_LARGE, "a generation holds at most 4 194 304 requests");
    if (depth == 0) depth = 4;
    if (depth < 3 || depth > 16) return fail(GUBER_E_INVALID_ARG, "3 .. 16 generations in flight");
    std::unique_ptr<guber_front, void (*)(guber_front*)> f(new guber_front(), [](guber_front* p) { guber_front_destroy(p); });
    for (uint32_t j = 0; j < n_engines; ++j) {
        guber_engine* e = engines[j];
        if (!e) return fail(GUBER_E_INVALID_ARG, "null engine");
        if (e->device != engines[0]->device) return fail(GUBER_E_INVALID_ARG, "the engines of a front live on one device");
        for (uint32_t q = 0; q < j; ++q) if (engines[q] == e) return fail(GUBER_E_INVALID_ARG, "an engine twice in one front");
        f->eng.push_back(e);
        int si = -1;
        for (size_t q = 0; q < f->streams.size(); ++q) if (f->streams[q] == e->stream) si = (int)q;
        if (si < 0) { si = (int)f->streams.size(); f->streams.push_back(e->stream); }
        f->stream_of.push_back(si);
        f->max_key = j == 0 ? e->max_key : std::min(f->max_key, e->max_key);
    }
    f->device = engines[0]->device; f->cap = max_n; f->depth = depth;
    if (hipSetDevice(f->device) != hipSuccess) return fail(GUBER_E_HIP, "hipSetDevice");
    HIPCHK(hipStreamCreateWithFlags(&f->rs, hipStreamNonBlocking));
    f->n_own_streams = 1;
    if (const char* v = guber_lab_env("GUBER_FRONT_STREAMS")) f->n_own_streams = std::max(1, std::min(3, atoi(v)));
    f->out_on_eval = true;
    if (const char* v = guber_lab_env("GUBER_FRONT_OUT_ON_EVAL")) f->out_on_eval = atoi(v) != 0;
    if (const char* v = guber_lab_env("GUBER_FRONT_OUT_DELAY")) f->out_delay = (uint32_t)std::max(0, std::min(2, atoi(v)));
    if (const char* v = guber_lab_env("GUBER_FRONT_ONE_PAIR_MAX")) f->one_pair_max = (uint32_t)strtoul(v, nullptr, 10);
    f->rs2 = f->os = f->rs;
    if (f->n_own_streams >= 2) HIPCHK(hipStreamCreateWithFlags(&f->os, hipStreamNonBlocking));
    if (f->n_own_streams >= 3) HIPCHK(hipStreamCreateWithFlags(&f->rs2, hipStreamNonBlocking));
    if (rule) { const int rc = front_set_rule(f.get(), rule); if (rc) return rc; }
    else f->rule = RouteRule{1, 1, 0, 0, -1, 0, 0, 0, nullptr, nullptr, nullptr};      // one engine: everything is its share
    f->slots.resize(depth);
    for (auto& s : f->slots) {
        if (s.host.ensure(1)) return GUBER_E_NOMEM;
        const size_t cap = max_n, key_bytes = cap * FR_KEY_COPY_MAX + 64;
        // the mirror: request columns, where each request went, the answers in the shares' order, the keys (<= FR_KEY_COPY_MAX bytes each
        // when they travel), then the routing's scratch
        auto carve = [&](uint8_t* base) {
            ColCarver c{(uintptr_t)base};
            FrIn& A = s.in;
            A.d_key_off = c.take<uint32_t>(cap + 1); A.d_key_len = c.take<uint32_t>(cap + 1); s.fwd = c.take<uint32_t>(cap + 1);
            A.d_hits = c.take<int64_t>(cap); A.d_limit = c.take<int64_t>(cap); A.d_duration = c.take<int64_t>(cap);
            A.d_burst = c.take<int64_t>(cap); A.d_created_at = c.take<int64_t>(cap);
            A.d_behavior = c.take<uint32_t>(cap); A.d_algorithm = c.take<uint8_t>(cap); A.d_is_owner = c.take<uint8_t>(cap);
            s.o_limit = c.take<int64_t>(cap); s.o_remaining = c.take<int64_t>(cap); s.o_reset = c.take<int64_t>(cap);
            s.o_status = c.take<uint8_t>(cap); s.o_err = c.take<uint8_t>(cap);
            A.d_keys = c.take<uint8_t>(key_bytes);
            A.M = route_carve(c, cap, s.host.p);
            return (size_t)(c.at - (uintptr_t)base);
        };
        if (s.mem.ensure(carve(nullptr))) return GUBER_E_NOMEM;
        carve(s.mem.p);
        if (f->streams.size() == 1 && n_engines > 1 && (s.h_margs.ensure(sizeof(MultiArgsMem)) || s.d_margs.ensure(sizeof(MultiArgsMem)))) return GUBER_E_NOMEM;
        memset((void*)s.host.p, 0, sizeof(FrontHost));
        HIPCHK(hipMemsetAsync(s.in.M.ctl, 0, sizeof(FrontCtl), f->rs));
        HIPCHK(hipMemsetAsync(s.in.d_keys, 0, front_col(key_bytes), f->rs));   // (the kernels read keys as 8-byte words: the bytes behind the last key are defined)
        HIPCHK(hipEventCreateWithFlags(&s.ev_in, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&s.ev_out, hipEventDisableTiming));
        for (size_t q = 0; q < f->streams.size(); ++q) {
            s.hooks.emplace_back(new EvalHook());
            HIPCHK(hipEventCreateWithFlags(&s.hooks.back()->ev, hipEventDisableTiming));
            s.hooks.back()->st = f->streams[q];
        }
    }
    HIPCHK(hipStreamSynchronize(f->rs));
    *out = f.release();
    return GUBER_OK;
}

// The routing on a stream of the caller's choice — the engines' own, when they share one — instead of the front's (before the front's first
// generation).  For a caller that needs the hardware queue the routing stream would take: the runtime has four that run at full speed
// (profiles/r06_wire_pool_hw_queues.txt: a fifth quarters the payload stage's rate), and a payload stage wants two for its decodes.
static int front_route_on(guber_front* f, hipStream_t st) {
    std::lock_guard<std::mutex> lk(f->mu);
    if (f->generations || f->pre_routed || f->n_own_streams != 1) return fail(GUBER_E_INVALID_ARG, "guber_front: the routing stream is chosen before the first generation");
    if (hipSetDevice(f->device) != hipSuccess) return fail(GUBER_E_HIP, "hipSetDevice");
    HIPCHK(hipStreamSynchronize(f->rs));
    HIPCHK(hipStreamDestroy(f->rs));
    f->rs = f->rs2 = f->os = st; f->rs_borrowed = true;
    return 0;
}

extern "C" int guber_front_set_rule(guber_front_t* f, const guber_route_rule_t* rule) {
    if (!f || !rule) return fail(GUBER_E_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(f->mu);
    if (f->ob.every && (uint64_t)rule->n_shards * rule->per != f->ob.n_slots) return fail(GUBER_E_INVALID_ARG, "guber_front: the rule's slots are counted by the observation window; guber_front_observe(f, 0) first");
    if (hipSetDevice(f->device) != hipSuccess) return fail(GUBER_E_HIP, "hipSetDevice");
    return front_set_rule(f, rule);
}

// k_fr_count, k_fr_scan and k_fr_scatter of generation g on its routing stream; observe: the generation counts for guber_front_observe's
// "every k-th" (a store generation does not, nor does an empty one), and the k-th is counted behind its routing (k_fr_observe)
static int front_route(guber_front* f, guber_front::Slot& s, const FrontGen* fg, int64_t gen, bool observe = true) {
    const guber_batch_t* b = &fg->b;
    hipStream_t rs = (gen & 1) ? f->rs2 : f->rs;
    if (observe && f->ob.skip_one) { f->ob.skip_one = false; observe = false; }   // (routed ahead, counted then, dropped by a pass: see Observe)
    // the slot's previous generation has left it: its answers' way home read what this routing writes
    if (s.out_recorded) { HIPCHK(hipStreamWaitEvent(rs, s.ev_out, 0)); s.out_recorded = false; }
    s.gen = gen; s.n = b->n; s.dispatched = false;
    s.seq = ++f->seq ? f->seq : ++f->seq;
    for (auto& h : s.hooks) { h->outstanding.store(1); h->recorded.store(false); }      // (1: the dispatcher's own hold until the generation's groups are out)
    if (b->n == 0) return 0;
    FrIn& A = s.in;
    A.n = b->n; A.n_engines = (uint32_t)f->eng.size(); A.max_key = f->max_key; A.seq = s.seq;
    A.key_bytes = b->key_bytes; A.key_off = b->key_off; A.key_stride = fg->key_stride; A.key_len = fg->key_len; A.hits = b->hits; A.limit = b->limit; A.duration = b->duration;
    A.burst = b->burst; A.created_at = b->created_at; A.behavior = b->behavior; A.algorithm = b->algorithm; A.is_owner = b->is_owner;
    A.R = f->rule;
    A.d_fwd = f->want_fwd.load(std::memory_order_relaxed) ? s.fwd : nullptr;
    const uint32_t tiles = (b->n + FR_TILE - 1u) / FR_TILE;
    guber_engine* e0 = f->eng[0];
    std::unique_lock<std::mutex> pl(e0->mu, std::defer_lock);       // (the per-kernel timing's spans and events belong to the first engine)
    if (e0->profiling || s.ev_a) pl.lock();
    if (s.ev_a) e0->event_pool.push_back(s.ev_a);                    // (the slot held a probed generation that was dropped: its span never ended)
    s.ev_a = nullptr;
    if (e0->profiling) { s.ev_a = e0->get_event(); (void)hipEventRecord(s.ev_a, rs); }
    e0->span_begin(KT_FR_COUNT, b->n, rs);
    hipLaunchKernelGGL(k_fr_count, dim3(tiles), dim3(FR_TILE), 0, rs, A);
    e0->span_end();
    e0->span_begin(KT_FR_SCAN, b->n, rs);
    hipLaunchKernelGGL(k_fr_scan, dim3(MULTI_MEM_MAX / 4), dim3(FR_SCAN_T), 0, rs, A, tiles, (tiles + FR_SCAN_T - 1) / FR_SCAN_T);
    e0->span_end();
    e0->span_begin(KT_FR_SCATTER, b->n, rs);
    hipLaunchKernelGGL(k_fr_scatter, dim3(tiles), dim3(256), 0, rs, A);
    e0->span_end();
    if (hipGetLastError() != hipSuccess) return fail(GUBER_E_HIP, "kernel launch");
    HIPCHK(hipEventRecord(s.ev_in, rs));
    if (observe && f->ob.every && ++f->ob.since >= f->ob.every) {
        // (behind the event: the generation's evaluation does not wait for it; the caller's arrays stay valid until guber_front_synchronize)
        f->ob.since = 0; f->ob.generations++;
        FrObs O{};
        O.n = A.n; O.max_key = A.max_key; O.key_stride = A.key_stride; O.cmask = FO_CELLS - 1u; O.no_agg = f->ob.no_agg ? 1u : 0u;
        O.key_bytes = A.key_bytes; O.key_off = A.key_off; O.key_len = A.key_len; O.behavior = A.behavior;
        O.slot_w = f->ob.slot_w; O.cell = f->ob.cell; O.tot = f->ob.tot; O.R = A.R;
        e0->span_begin(KT_FR_OBSERVE, b->n, rs);
        hipLaunchKernelGGL(k_fr_observe, dim3(tiles), dim3(FR_TILE), 0, rs, O);
        e0->span_end();
        if (hipGetLastError() != hipSuccess) return fail(GUBER_E_HIP, "kernel launch");
    }
    return 0;
}

// the answers of the slot's generation home, in arrival order (every evaluation of the generation has been launched)
static int front_out(guber_front* f, guber_front::Slot& s, guber_result_t* r) {
    if (s.n == 0) return 0;
    // (out_on_eval: the answers' last hop rides on one of the engines' streams, generation by generation in turn — those are idle two fifths
    //  of the time, the routing stream is the pipeline's bottleneck)
    hipStream_t os = f->out_on_eval ? f->streams[(size_t)s.gen % f->streams.size()] : f->os;
    f->last_os = os;
    for (auto& h : s.hooks) if (h->st != os) HIPCHK(hipStreamWaitEvent(os, h->ev, 0));
    FrOut O{};
    O.n = s.n; O.M = s.in.M;                                         // (the slot's routing scratch: routed into again only behind ev_out)
    O.d_status = s.o_status; O.d_err = s.o_err; O.d_limit = s.o_limit; O.d_remaining = s.o_remaining; O.d_reset_time = s.o_reset;
    O.status = r->status; O.err = r->err; O.limit = r->limit; O.remaining = r->remaining; O.reset_time = r->reset_time;
    guber_engine* e0 = f->eng[0];
    std::unique_lock<std::mutex> pl(e0->mu, std::defer_lock);
    if (e0->profiling) pl.lock();
    e0->span_begin(f->st.active ? KT_FR_OUT_STORE : KT_FR_OUT, s.n, os);
    if (f->st.active) {
        // a store generation: the events travel home with the answers
        FrOutStore S{O, FrOutSide{f->st.flags.p, f->st.after.p, f->st.oflags.p, f->st.oafter.p}};
        hipLaunchKernelGGL(k_fr_out_store, dim3((s.n + FR_TILE - 1u) / FR_TILE), dim3(256), 0, os, S);
    } else if (f->enc_hook) {
        // the payload stage (guber_wire_pool.h): the answers' last hop is the encoder — every RPC's GetRateLimitsResp bytes from the shares, through fwd
        if (!s.in.d_fwd) return fail(GUBER_E_INVALID_ARG, "guber_front: the generation was routed without fwd (want_fwd is set before the routing)");
        guber::WireEnc E = *f->enc_hook;
        E.fwd = s.in.d_fwd; E.d_status = O.d_status; E.d_err = O.d_err; E.d_limit = O.d_limit; E.d_remaining = O.d_remaining; E.d_reset = O.d_reset_time;
        hipLaunchKernelGGL(guber::k_wire_enc, dim3(E.nrpc), dim3(guber::WE_T), 0, os, E);
    } else
    hipLaunchKernelGGL(k_fr_out, dim3((s.n + FR_TILE - 1u) / FR_TILE), dim3(256), 0, os, O);
    e0->span_end();
    if (s.ev_a) { hipEvent_t evb = e0->get_event(); (void)hipEventRecord(evb, os); f->gen_spans.push_back({s.ev_a, evb}); s.ev_a = nullptr; }
    if (hipGetLastError() != hipSuccess) return fail(GUBER_E_HIP, "kernel launch");
    if (os != f->rs) { HIPCHK(hipEventRecord(s.ev_out, os)); s.out_recorded = true; }
    return 0;
}

static bool front_evals_launched(const guber_front::Slot& s) {
    for (auto& h : s.hooks) if (!h->recorded.load(std::memory_order_acquire)) return false;
    return true;
}

// gens[k] -> results[k], k = 0 .. count-1: every pointer inside is a DEVICE pointer, requests in arrival order, answers in arrival
// order.  Asynchronous: returns when everything is enqueued (guber_front_synchronize waits).  The caller's arrays must stay valid and
// their contents ready (produced before the call, on any stream the caller has synchronised with) until then.
static int front_eval(guber_front* f, const FrontGen* gens, guber_result_t* results, uint32_t count, uint32_t* done, hipEvent_t after = nullptr);
extern "C" int guber_front_eval_dev(guber_front_t* f, const guber_batch_t* gens, guber_result_t* results, uint32_t count, uint32_t* done) {
    if (done) *done = 0;
    if (!f || (count && (!gens || !results))) return fail(GUBER_E_INVALID_ARG, "null argument");
    std::vector<FrontGen> g(count);
    for (uint32_t k = 0; k < count; ++k) {
        const int rc = check_batch_args(&gens[k], &results[k]);
        if (rc) return rc;
        g[k].b = gens[k];
    }
    return front_eval(f, g.data(), results, count, done);
}
// `after`: recorded behind the last generation's answers (on the stream their last hop ran on: the answers of a call leave in order)
static int front_eval_locked(guber_front* f, const FrontGen* gens, guber_result_t* results, uint32_t count, uint32_t* done, hipEvent_t after);
static int front_eval(guber_front* f, const FrontGen* gens, guber_result_t* results, uint32_t count, uint32_t* done, hipEvent_t after) {
    if (done) *done = 0;
    for (uint32_t k = 0; k < count; ++k) {
        if (gens[k].b.n > f->cap) return fail(GUBER_E_BATCH_TOO_LARGE, "generation larger than the front was created for");
        if (gens[k].b.greg_expire || gens[k].b.greg_duration) return fail(GUBER_E_INVALID_ARG, "a front takes its calendar intervals from the device");
        if (gens[k].key_stride & 7u) return fail(GUBER_E_INVALID_ARG, "key rows are a multiple of 8 bytes apart");
        clear_aggregates(results[k]);
    }
    std::lock_guard<std::mutex> lk(f->mu);
    if (hipSetDevice(f->device) != hipSuccess) return fail(GUBER_E_HIP, "hipSetDevice");
    return front_eval_locked(f, gens, results, count, done, after);
}
// (f->mu held, the device set, the generations checked; st.active: the one generation is the probed one — guber_front_eval_store_dev)
static int front_eval_locked(guber_front* f, const FrontGen* gens, guber_result_t* results, uint32_t count, uint32_t* done, hipEvent_t after) {
    if (f->st.probed && !f->st.active) { f->st.probed = false; f->pre_routed = false; }   // (a probed generation nobody evaluated: dropped, this call routes afresh)
    const uint32_t ne = (uint32_t)f->eng.size(), D = f->depth, ahead = D - 2;
    PendSet pendset;
    bool any_ep = false;
    for (auto* e : f->eng) any_ep = any_ep || e->fuse_ep;
    PendSet* const ps = any_ep ? &pendset : nullptr;
    struct Dispatching { bool on; Dispatching(bool o) : on(o) { if (on) ++tl_ep_dispatcher; } ~Dispatching() { if (on) --tl_ep_dispatcher; } } dispatching(any_ep);
    uint32_t next_route = 0, next_out = 0, enq = 0;
    int rc = 0;
    uint64_t fp[4] = {0, 0, 0, 0};                                  // GUBER_DISPATCH_PROFILE: ns spent enqueueing the routing, waiting for the shares' sizes, dispatching, on the answers
    struct FpSpan { uint64_t* a; uint64_t t0; explicit FpSpan(uint64_t* x) : a(x), t0(dp_now()) {} ~FpSpan() { if (g_dprof) *a += dp_now() - t0; } };
    // (the slots go round across calls: a caller that hands over one generation per call — the payload stage — gets the routing of its next
    //  generation beside the evaluation of the last one, as a caller that hands over sixteen at once does)
    const uint64_t g0 = f->generations;
    auto slot_of = [&](uint32_t k) -> guber_front::Slot& { return f->slots[(g0 + k) % D]; };
    // the answers of every generation whose evaluations have all been launched go home, oldest first
    auto drain_outs = [&](uint32_t upto, bool force) -> int {
        while (next_out < upto) {
            guber_front::Slot& s = slot_of(next_out);
            if (!s.dispatched) break;
            if (s.n && !front_evals_launched(s)) {
                if (!force) break;
                f->forced_flushes++;
                const int r2 = pendset.flush_all();
                if (r2) return r2;
                if (!front_evals_launched(s)) return fail(GUBER_E_HIP, "guber_front: an evaluation was not launched");
            }
            const int r3 = front_out(f, s, &results[next_out]);
            if (r3) return r3;
            ++next_out;
            if (done) *done = next_out;
        }
        return 0;
    };
    std::vector<std::vector<GroupItem>> fifo(ne);
    std::vector<EvalHook*> hook_of(ne, nullptr);
    for (uint32_t k = 0; k < count && !rc; ++k) {
        // the routing runs ahead; a slot is routed into again only after its previous generation's answers have left it
        while (next_route < count && next_route <= k + ahead && !rc) {
            if (next_route >= D) { rc = drain_outs(next_route - D + 1, true); if (rc) break; }
            if (next_route == 0 && f->pre_routed) f->pre_routed = false;          // (front_route_ahead did it: same slot, same generation number)
            else { FpSpan sp(&fp[0]); rc = front_route(f, slot_of(next_route), &gens[next_route], (int64_t)f->generations + next_route); }
            ++next_route;
        }
        if (rc) break;
        guber_front::Slot& s = slot_of(k);
        const guber_batch_t* b = &gens[k].b;
        if (s.n) {
            // the shares' sizes (in pinned memory since k_fr_scan: normally long there)
            if (!route_reported(s.host.p, MULTI_MEM_MAX + 1, s.seq)) {
                FpSpan sp(&fp[1]);
                const auto t0 = std::chrono::steady_clock::now();
                f->host_waits++;
                rc = route_wait_reported(s.host.p, MULTI_MEM_MAX + 1, s.seq, f->device, (s.gen & 1) ? f->rs2 : f->rs, "guber_front: the routing of a generation did not report");
                f->host_wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                if (rc) break;
            }
            uint32_t counts[MULTI_MEM_MAX];
            for (int q = 0; q < MULTI_MEM_MAX; ++q) counts[q] = (uint32_t)s.host.p->w[q];
            const bool packed = !((uint32_t)s.host.p->w[MULTI_MEM_MAX] >> 8 & 1u);
            const uint32_t width = (uint32_t)s.host.p->w[MULTI_MEM_MAX] & 0xffu;      // (packed: 1 .. FR_KEY_COPY_MAX, k_fr_count has seen to it)
            if (packed && (width == 0 || width > FR_KEY_COPY_MAX)) { rc = fail(GUBER_E_HIP, "guber_front: a packed generation without a key width"); break; }
            for (auto st : f->streams) { if (hipStreamWaitEvent(st, s.ev_in, 0) != hipSuccess) { rc = fail(GUBER_E_HIP, "hipStreamWaitEvent"); break; } }
            if (rc) break;
            uint32_t base = 0, total = 0;
            for (uint32_t j = 0; j < ne; ++j) {
                fifo[j].clear();
                hook_of[j] = s.hooks[f->stream_of[j]].get();
                const uint32_t nj = counts[j];
                total += nj;
                guber_engine* e = f->eng[j];
                // a share larger than the engine's pipelines take goes in pieces of EQUAL size (whole tiles): the rounds of a generation then
                // carry the same load (65 536 + a rest would make the second round a third of the first)
                const uint32_t cap_e = std::max<uint32_t>(1u, std::min<uint32_t>(e->fast_cap ? e->fast_cap : e->max_batch, e->max_batch));
                const uint32_t np = (nj + cap_e - 1) / cap_e;
                uint32_t piece = np > 1 ? ((nj + np - 1) / np + 255u) & ~255u : cap_e;
                if (piece > cap_e) piece = cap_e;
                for (uint32_t pos = 0; pos < nj; pos += piece) {
                    const uint32_t len = std::min(piece, nj - pos), d0 = base + pos;
                    const FrIn& A = s.in;
                    // (a packed generation's pieces say where their keys are with key_width: k_fr_scatter wrote no offsets for them)
                    BatchView B{len, 0, packed ? A.d_keys + (size_t)d0 * width : b->key_bytes, packed ? nullptr : A.d_key_off + d0, A.d_hits + d0, A.d_limit + d0, A.d_duration + d0,
                                b->burst ? A.d_burst + d0 : nullptr, b->created_at ? A.d_created_at + d0 : nullptr,
                                A.d_algorithm + d0, A.d_behavior + d0, b->is_owner ? A.d_is_owner + d0 : nullptr, nullptr, nullptr, b->now_ms,
                                0, packed ? width : 0u, packed ? nullptr : A.d_key_len + d0};
                    fifo[j].push_back(GroupItem{B, ResultView{s.o_status + d0, s.o_limit + d0, s.o_remaining + d0, s.o_reset + d0, s.o_err + d0},
                                                f->st.active ? f->st.flags.p + d0 : nullptr, f->st.active ? f->st.after.p + d0 : nullptr});
                }
                base += nj;
            }
            if (total != s.n) { rc = fail(GUBER_E_HIP, "guber_front: the shares do not add up to the generation"); break; }
            // a generation of small shares on ONE stream (the payload stage's): all its tables in one pair of launches
            bool one_pair = f->streams.size() == 1 && ne > 1 && s.h_margs.p && s.n <= f->one_pair_max;
            guber_engine* og[MULTI_MEM_MAX]; GroupItem oi[MULTI_MEM_MAX]; int on = 0;
            for (uint32_t j = 0; j < ne && one_pair; ++j) {
                if (fifo[j].empty()) continue;
                one_pair = fifo[j].size() == 1 && can_fuse(f->eng[j], fifo[j][0].B.n);
                og[on] = f->eng[j]; oi[on] = fifo[j][0]; ++on;
            }
            if (one_pair && on > 1) {
                FpSpan sp(&fp[2]);
                rc = pendset.flush_all();                                   // (what an earlier generation of this call holds back on these tables goes first)
                int r1 = rc ? rc : launch_group_mem(og, oi, on, &enq, (MultiArgsMem*)s.h_margs.p, (MultiArgsMem*)s.d_margs.p);
                if (r1 == 1) r1 = dispatch_rounds(f->eng.data(), ne, fifo, ps, &enq, hook_of.data());   // (a table turned out tight: the ordinary way)
                rc = r1;
            } else { FpSpan sp(&fp[2]); rc = dispatch_rounds(f->eng.data(), ne, fifo, ps, &enq, hook_of.data()); }
        }
        s.dispatched = true;
        for (auto& h : s.hooks) h->launched();                      // the dispatcher's hold: the event is recorded once nothing of the generation is held back
        if (rc) break;
        { FpSpan sp(&fp[3]); rc = drain_outs(k + 1 > f->out_delay ? k + 1 - f->out_delay : 0, false); }
    }
    // (what was routed or enqueued is completed, also after an error: its evaluations go now, its answers go home)
    {
        for (uint32_t k = 0; k < next_route; ++k) {
            guber_front::Slot& s = slot_of(k);
            if (k >= next_out && !s.dispatched) { s.dispatched = true; s.n = 0; for (auto& h : s.hooks) h->launched(); }   // (routed, never evaluated: an error above)
        }
        const int rcf = pendset.flush_all();
        if (!rc) rc = rcf;
        const int rco = drain_outs(next_route, true);
        if (!rc) rc = rco;
    }
    f->generations += next_out;
    if (after && !rc && hipEventRecord(after, f->last_os ? f->last_os : f->rs) != hipSuccess) rc = fail(GUBER_E_HIP, "hipEventRecord");
    if (g_dprof && next_out) {
        fprintf(stderr, "[front] %u generations; per generation: routing enqueue %.2f us, waiting for the shares' sizes %.2f, dispatch %.2f, answers %.2f\n", next_out,
                fp[0] / 1e3 / next_out, fp[1] / 1e3 / next_out, fp[2] / 1e3 / next_out, fp[3] / 1e3 / next_out);
        if (tl_dp[6]) fprintf(stderr, "[front dispatch] %llu batches in %llu groups; per batch: wait-for-progress %.2f us, locks %.2f, preludes+plans %.2f, argument blocks %.2f, launches %.2f\n",
                (unsigned long long)tl_dp[6], (unsigned long long)tl_dp[5], tl_dp[0] / 1e3 / tl_dp[6], tl_dp[1] / 1e3 / tl_dp[6], tl_dp[2] / 1e3 / tl_dp[6],
                tl_dp[3] / 1e3 / tl_dp[6], tl_dp[4] / 1e3 / tl_dp[6]);
        for (auto& v : tl_dp) v = 0;
    }
    return rc;
}

// The routing of the NEXT call's first generation, enqueued now (the payload stage: its flusher never waits for the GPU, so it routes as
// soon as a stage is decoded and comes back for the evaluation when the shares' sizes are in host memory).  The next front_eval call must
// hand over the same generation first.
static int front_route_ahead(guber_front* f, const FrontGen* g) {
    if (g->b.n > f->cap) return fail(GUBER_E_BATCH_TOO_LARGE, "generation larger than the front was created for");
    if (g->key_stride & 7u) return fail(GUBER_E_INVALID_ARG, "key rows are a multiple of 8 bytes apart");
    std::lock_guard<std::mutex> lk(f->mu);
    if (f->st.probed) { f->st.probed = false; f->pre_routed = false; }   // (a probed generation nobody evaluated: dropped)
    if (f->pre_routed) return fail(GUBER_E_INVALID_ARG, "guber_front: a generation is routed ahead already");
    if (hipSetDevice(f->device) != hipSuccess) return fail(GUBER_E_HIP, "hipSetDevice");
    const int rc = front_route(f, f->slots[f->generations % f->depth], g, (int64_t)f->generations);
    if (!rc) { f->pre_routed = true; f->ob.ahead_counted = f->ob.every != 0 && g->b.n != 0; }
    return rc;
}
// have the shares' sizes of the generation routed ahead reached host memory?
static bool front_routed_ahead_ready(guber_front* f) {
    std::lock_guard<std::mutex> lk(f->mu);
    if (!f->pre_routed) return true;
    guber_front::Slot& s = f->slots[f->generations % f->depth];
    return s.n == 0 || route_reported(s.host.p, MULTI_MEM_MAX + 1, s.seq);
}

// ---- the Store side channel of a generation routed on the device (include/guber_gpu.h, Config.Store) -------------------------------
// guber_front_probe_missing_dev routes the generation into the next slot, the way front_route_ahead leaves one, and runs k_fr_elect /
// k_fr_missing / k_fr_ask (guber_kernels_front_store.h) behind the routing on its stream; guber_front_eval_store_dev evaluates that
// generation with the side channel in every share's Work and brings the events home with k_fr_out_store.  Both are synchronous.
static int front_store_ensure(guber_front* f) {
    auto& t = f->st;
    if (t.cap) return 0;
    const uint32_t cap = std::min<uint32_t>(f->cap, FR_STORE_MAX_N);
    uint32_t cells = 1024; while (cells < 2 * (uint64_t)cap) cells <<= 1;
    const size_t tiles = ((size_t)cap + FR_TILE - 1) / FR_TILE;
    if (t.tag.ensure(cells) || t.first.ensure(2 * (size_t)cells) || t.cell.ensure(cap) || t.tile_cnt.ensure(tiles) || t.index.ensure(cap) || t.ask.ensure(cap) ||
        t.engine.ensure(cap) || t.flags.ensure(cap) || t.oflags.ensure(cap) || t.after.ensure(cap) || t.oafter.ensure(cap) || t.ctl.ensure(1) || t.tabs.ensure(1)) return GUBER_E_NOMEM;
    for (size_t q = 0; q < f->streams.size(); ++q) { hipEvent_t ev = nullptr; HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); t.ev.push_back(ev); }
    t.cells = cells; t.cap = cap;
    return 0;
}
// collision != 0 (two identities in one election cell): cut_at and the ask list from a host copy of the generation's keys and a residency
// read of every request (k_fr_missing, all = 1).  The engines' locks are the caller's; rs has been synchronised.
static int front_store_on_host(guber_front* f, guber_front::Slot& s, const FrontGen* g, FrStore E, hipStream_t rs, std::vector<uint32_t>& index, std::vector<uint8_t>& engine, uint32_t* cut_at) {
    const guber_batch_t& b = g->b;
    const uint32_t n = b.n;
    std::vector<uint16_t> er(n); std::vector<uint32_t> off(n + 1, 0), len(n), beh(n, 0); std::vector<uint8_t> miss(n), keys;
    E.all = 1u;
    hipLaunchKernelGGL(k_fr_missing, dim3((n + 255u) / 256u), dim3(256), 0, rs, s.in, E);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(miss.data(), E.ask, n, hipMemcpyDeviceToHost, rs));
    HIPCHK(hipMemcpyAsync(er.data(), s.in.M.er, (size_t)n * 2, hipMemcpyDeviceToHost, rs));
    if (b.behavior) HIPCHK(hipMemcpyAsync(beh.data(), b.behavior, (size_t)n * 4, hipMemcpyDeviceToHost, rs));
    if (g->key_stride) HIPCHK(hipMemcpyAsync(len.data(), g->key_len, (size_t)n * 4, hipMemcpyDeviceToHost, rs));
    else HIPCHK(hipMemcpyAsync(off.data(), b.key_off, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, rs));
    HIPCHK(hipStreamSynchronize(rs));
    size_t base = 0;
    if (g->key_stride) {
        keys.resize((size_t)n * g->key_stride);
        for (uint32_t i = 0; i < n; ++i) off[i] = i * g->key_stride;
    } else {
        base = off[0];
        keys.resize((size_t)off[n] - base);
        for (uint32_t i = 0; i < n; ++i) len[i] = off[i + 1] - off[i];
    }
    if (!keys.empty()) HIPCHK(hipMemcpy(keys.data(), b.key_bytes + base, keys.size(), hipMemcpyDeviceToHost));
    struct Seen { bool reset; };
    std::unordered_map<std::string, Seen> seen;
    seen.reserve(n);
    uint32_t cut = n;
    index.clear(); engine.clear();
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t e = (uint8_t)(er[i] >> FR_RANK_BITS);
        std::string id(1, (char)e);
        id.append((const char*)keys.data() + (off[i] - base), len[i]);
        auto ins = seen.emplace(std::move(id), Seen{false});
        if (!ins.second && ins.first->second.reset) { cut = i; break; }
        if (ins.second && len[i] != 0 && miss[i]) { index.push_back(i); engine.push_back(e); }
        if (beh[i] & 8u) ins.first->second.reset = true;
    }
    *cut_at = cut;
    return 0;
}
static int front_probe_missing(guber_front* f, const FrontGen* g, guber_front_ask_t* ask) {
    const guber_batch_t& b = g->b;
    const uint32_t n = b.n;
    ask->n = 0; ask->cut_at = n;
    if (n > FR_STORE_MAX_N) return fail(GUBER_E_BATCH_TOO_LARGE, "a store generation holds at most 1 048 576 requests");
    if (n > f->cap) return fail(GUBER_E_BATCH_TOO_LARGE, "generation larger than the front was created for");
    if (b.greg_expire || b.greg_duration) return fail(GUBER_E_INVALID_ARG, "a front takes its calendar intervals from the device");
    if (g->key_stride & 7u) return fail(GUBER_E_INVALID_ARG, "key rows are a multiple of 8 bytes apart");
    if (n && (!b.key_bytes || (!g->key_stride && !b.key_off) || !b.hits || !b.limit || !b.duration)) return fail(GUBER_E_INVALID_ARG, "batch is missing a mandatory array");
    if (ask->cap && (!ask->index || !ask->engine)) return fail(GUBER_E_INVALID_ARG, "null ask arrays");
    std::lock_guard<std::mutex> lk(f->mu);
    auto& t = f->st;
    if (f->pre_routed && !t.probed) return fail(GUBER_E_INVALID_ARG, "guber_front: a generation is routed ahead already");
    if (hipSetDevice(f->device) != hipSuccess) return fail(GUBER_E_HIP, "hipSetDevice");
    { const int rc = front_store_ensure(f); if (rc) return rc; }
    guber_front::Slot& s = f->slots[f->generations % f->depth];
    guber_engine* e0 = f->eng[0];
    t.probed = false; f->pre_routed = false;
    { const int rc = front_route(f, s, g, (int64_t)f->generations, false); if (rc) return rc; }
    t.probes++;
    t.n = n; t.cut_at = n; t.key_bytes = b.key_bytes; t.key_off = g->key_stride ? (const void*)g->key_len : (const void*)b.key_off; t.now_ms = b.now_ms;
    if (n == 0) { t.probed = true; f->pre_routed = true; return GUBER_OK; }
    hipStream_t rs = (s.gen & 1) ? f->rs2 : f->rs;
    uint32_t cells = 1024; while (cells < 2 * (uint64_t)n) cells <<= 1;
    const uint32_t tiles = (n + FR_TILE - 1u) / FR_TILE;
    FrStore E{};
    E.tag = t.tag.p; E.first = t.first.p; E.first_reset = t.first.p + cells; E.cmask = cells - 1u; E.hash_mask = e0->T.hash_mask; E.cell = t.cell.p;
    E.tabs = t.tabs.p; E.now = b.now_ms; E.ask = t.ask.p; E.ctl = t.ctl.p; E.tile_cnt = t.tile_cnt.p; E.index = t.index.p; E.engine = t.engine.p; E.cap = t.cap; E.all = 0u;
    std::vector<uint32_t> h_index; std::vector<uint8_t> h_engine;
    uint32_t n_ask = 0, cut = n;
    {
        // the engines' tables as they are now, behind everything enqueued on their streams (evaluations, guber_add_items): read under the
        // engines' locks, which are kept until the probe has run
        const int ne = (int)f->eng.size();
        EngineLocks locks(ne, [&](int i) { return f->eng[i]; });
        locks.launch_held_by_others();
        for (int j = 0; j < ne; ++j) t.h_tabs.t[j] = f->eng[j]->T;
        for (size_t q = 0; q < f->streams.size(); ++q) if (f->streams[q] != rs) { HIPCHK(hipEventRecord(t.ev[q], f->streams[q])); HIPCHK(hipStreamWaitEvent(rs, t.ev[q], 0)); }
        t.h_ctl = FrStoreCtl{n, 0u, 0u, 0u};
        HIPCHK(hipMemcpyAsync(t.tabs.p, &t.h_tabs, sizeof(FrStoreTabs), hipMemcpyHostToDevice, rs));
        HIPCHK(hipMemcpyAsync(t.ctl.p, &t.h_ctl, sizeof(FrStoreCtl), hipMemcpyHostToDevice, rs));
        HIPCHK(hipMemsetAsync(t.tag.p, 0, (size_t)cells * 8, rs));
        HIPCHK(hipMemsetAsync(t.first.p, 0xff, (size_t)cells * 8, rs));                 // (first and first_reset)
        HIPCHK(hipMemsetAsync(t.flags.p, 0, n, rs));                                    // (the side channel's flags: a request answered with an error writes none)
        e0->span_begin(KT_FR_ELECT, n, rs);
        hipLaunchKernelGGL(k_fr_elect, dim3((n + 255u) / 256u), dim3(256), 0, rs, s.in, E);
        e0->span_end();
        e0->span_begin(KT_FR_MISSING, n, rs);
        hipLaunchKernelGGL(k_fr_missing, dim3((n + 255u) / 256u), dim3(256), 0, rs, s.in, E);
        e0->span_end();
        for (uint32_t w = 0; w < 2; ++w) {
            e0->span_begin(KT_FR_ASK, n, rs);
            hipLaunchKernelGGL(k_fr_ask, dim3(tiles), dim3(FR_TILE), 0, rs, E, (const uint16_t*)s.in.M.er, n, w);
            e0->span_end();
        }
        if (hipGetLastError() != hipSuccess) return fail(GUBER_E_HIP, "kernel launch");
        HIPCHK(hipMemcpyAsync(&t.h_ctl, t.ctl.p, sizeof(FrStoreCtl), hipMemcpyDeviceToHost, rs));
        HIPCHK(hipStreamSynchronize(rs));
        if (t.h_ctl.collision) {
            t.collisions++;
            int rc;
            try { rc = front_store_on_host(f, s, g, E, rs, h_index, h_engine, &cut); }
            catch (const std::bad_alloc&) { rc = fail(GUBER_E_NOMEM, "guber_front: the host copy of the generation's keys"); }   // (the locks go with the scope)
            if (rc) return rc;
            n_ask = (uint32_t)h_index.size();
        } else { n_ask = t.h_ctl.n_ask; cut = t.h_ctl.cut_at; }
    }
    if (cut > n || n_ask > n) return fail(GUBER_E_HIP, "guber_front: the probe left no verdict");
    ask->n = n_ask; ask->cut_at = cut;
    t.cut_at = cut;
    // (cut_at < n: nothing stays routed — the caller comes back with the pieces; otherwise the generation waits in its slot)
    t.probed = f->pre_routed = cut == n;
    if (cut < n) t.cuts++;
    if (n_ask > ask->cap) return fail(GUBER_E_NOMEM, "guber_front: the ask arrays are too small");
    if (n_ask) {
        if (t.h_ctl.collision) { memcpy(ask->index, h_index.data(), (size_t)n_ask * 4); memcpy(ask->engine, h_engine.data(), n_ask); }
        else {
            HIPCHK(hipMemcpy(ask->index, t.index.p, (size_t)n_ask * 4, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(ask->engine, t.engine.p, n_ask, hipMemcpyDeviceToHost));
        }
    }
    t.asked += n_ask;
    return GUBER_OK;
}
static int front_eval_store(guber_front* f, const FrontGen* g, guber_result_t* result, guber_store_events_t* ev) {
    const guber_batch_t& b = g->b;
    const uint32_t n = b.n;
    if (n && (!ev->flags || !ev->items)) return fail(GUBER_E_INVALID_ARG, "null store event arrays");
    clear_aggregates(*result);
    std::lock_guard<std::mutex> lk(f->mu);
    auto& t = f->st;
    if (!t.probed || !f->pre_routed || t.cut_at != t.n) return fail(GUBER_E_INVALID_ARG, "guber_front: no probed generation to evaluate (guber_front_probe_missing_dev first; a cut generation goes in pieces)");
    if (n != t.n || b.key_bytes != t.key_bytes || (g->key_stride ? (const void*)g->key_len : (const void*)b.key_off) != t.key_off || b.now_ms != t.now_ms)
        return fail(GUBER_E_INVALID_ARG, "guber_front: not the generation the last probe routed");
    {   // the optional columns the routing scattered are the ones the shares are evaluated with
        const FrIn& A = f->slots[f->generations % f->depth].in;
        if (n && ((b.burst != nullptr) != (A.burst != nullptr) || (b.created_at != nullptr) != (A.created_at != nullptr) || (b.is_owner != nullptr) != (A.is_owner != nullptr)))
            return fail(GUBER_E_INVALID_ARG, "guber_front: burst / created_at / is_owner are not present as they were at the probe");
    }
    if (hipSetDevice(f->device) != hipSuccess) return fail(GUBER_E_HIP, "hipSetDevice");
    t.active = true;
    uint32_t done = 0;
    int rc = front_eval_locked(f, g, result, 1, &done, nullptr);
    t.active = false; t.probed = false;
    if (rc) return rc;
    t.evals++;
    if (n == 0) return GUBER_OK;
    // the answers and the events are complete on return: every stream the generation ran on
    for (auto st : f->streams) HIPCHK(hipStreamSynchronize(st));
    for (hipStream_t st : {f->rs, f->rs2, f->os}) HIPCHK(hipStreamSynchronize(st));
    std::vector<Rec> after;
    std::vector<uint32_t> off;
    try { after.resize(n); off.resize((size_t)n + 1); } catch (...) { return GUBER_E_NOMEM; }
    HIPCHK(hipMemcpy(ev->flags, t.oflags.p, n, hipMemcpyDeviceToHost));
    bool any = false;
    for (uint32_t i = 0; i < n && !any; ++i) any = (ev->flags[i] & GUBER_STORE_ONCHANGE) != 0;
    if (!any) return GUBER_OK;
    HIPCHK(hipMemcpy(after.data(), t.oafter.p, (size_t)n * sizeof(Rec), hipMemcpyDeviceToHost));
    if (g->key_stride) HIPCHK(hipMemcpy(off.data(), g->key_len, (size_t)n * 4, hipMemcpyDeviceToHost));
    else HIPCHK(hipMemcpy(off.data(), b.key_off, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i) {
        if (!(ev->flags[i] & GUBER_STORE_ONCHANGE)) continue;
        item_from_rec(after[i], &ev->items[i]);
        ev->items[i].key = nullptr;                                   // (the caller owns the key bytes)
        ev->items[i].key_len = g->key_stride ? off[i] : off[i + 1] - off[i];
    }
    return GUBER_OK;
}
extern "C" int guber_front_probe_missing_dev(guber_front_t* f, const guber_batch_t* gen, guber_front_ask_t* ask) {
    if (!f || !gen || !ask) return fail(GUBER_E_INVALID_ARG, "null argument");
    FrontGen g; g.b = *gen;
    return front_probe_missing(f, &g, ask);
}
extern "C" int guber_front_eval_store_dev(guber_front_t* f, const guber_batch_t* gen, guber_result_t* result, guber_store_events_t* ev) {
    if (!f || !ev) return fail(GUBER_E_INVALID_ARG, "null argument");
    const int rc = check_batch_args(gen, result);
    if (rc) return rc;
    FrontGen g; g.b = *gen;
    return front_eval_store(f, &g, result, ev);
}
extern "C" int guber_front_store_stats(guber_front_t* f, guber_front_store_stats_t* out) {
    if (!f || !out) return fail(GUBER_E_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(f->mu);
    out->probes = f->st.probes; out->collisions = f->st.collisions; out->cuts = f->st.cuts; out->asked = f->st.asked; out->evaluations = f->st.evals;
    return GUBER_OK;
}

extern "C" int guber_front_synchronize(guber_front_t* f) {
    if (!f) return fail(GUBER_E_INVALID_ARG, "null front");
    std::lock_guard<std::mutex> lk(f->mu);
    if (hipSetDevice(f->device) != hipSuccess) return fail(GUBER_E_HIP, "hipSetDevice");
    for (auto st : f->streams) HIPCHK(hipStreamSynchronize(st));
    for (hipStream_t st : {f->rs, f->rs2, f->os}) HIPCHK(hipStreamSynchronize(st));
    return GUBER_OK;
}

// microseconds per generation since the last call (needs guber_profile_enable on the front's FIRST engine while the generations ran);
// waits for the routing stream
extern "C" int guber_front_latencies(guber_front_t* f, float* us, uint32_t cap, uint32_t* n_out) {
    if (!f || !n_out) return fail(GUBER_E_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(f->mu);
    if (hipSetDevice(f->device) != hipSuccess) return fail(GUBER_E_HIP, "hipSetDevice");
    HIPCHK(hipStreamSynchronize(f->os));
    uint32_t n = 0;
    guber_engine* e0 = f->eng[0];
    std::lock_guard<std::mutex> lk2(e0->mu);
    for (auto& g : f->gen_spans) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, g.a, g.b) == hipSuccess && us && n < cap) us[n] = ms * 1e3f;
        ++n;
        e0->event_pool.push_back(g.a); e0->event_pool.push_back(g.b);
    }
    f->gen_spans.clear();
    *n_out = n;
    return GUBER_OK;
}

extern "C" void* guber_front_stream(guber_front_t* f) { return f ? (void*)f->os : nullptr; }

extern "C" int guber_front_stats(guber_front_t* f, guber_front_stats_t* out) {
    if (!f || !out) return fail(GUBER_E_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(f->mu);
    out->generations = f->generations; out->forced_flushes = f->forced_flushes; out->host_waits = f->host_waits;
    out->host_wait_us = (uint64_t)(f->host_wait_ms * 1e3);
    return GUBER_OK;
}

// ---- online placement: the front observes its own traffic and runs placement passes (include/guber_gpu.h) ------------------------------
// guber_front_observe turns the sampling on (front_route launches k_fr_observe behind every k-th generation's routing); a window ends in
// guber_front_observation (tests, tools) or guber_front_rebalance, which drives the placement as GPUWorkerPool's passes do
// (worker_pool.cpp: plan, migrate, cancel what could not be migrated, commit).
static int front_observe_ensure(guber_front* f) {
    auto& o = f->ob;
    const uint32_t n_slots = f->rule.n_shards * f->rule.per;
    if (o.mem.p && o.n_slots == n_slots) return 0;
    for (hipStream_t st : {f->rs, f->rs2}) HIPCHK(hipStreamSynchronize(st));      // (a window counted under a rule of another size: nobody reads it any more)
    auto carve = [&](uint8_t* base) {
        ColCarver c{(uintptr_t)base};
        o.cell = c.take<FrObsCell>(FO_CELLS); o.slot_w = c.take<uint32_t>(n_slots); o.tot = c.take<FrObsTot>(FO_STRIPES); o.n_top = c.take<uint32_t>(1);
        return (size_t)(c.at - (uintptr_t)base);
    };
    auto carve_host = [&](uint8_t* base) {
        ColCarver c{(uintptr_t)base};
        o.h_hash = c.take<unsigned long long>(FO_TOP_MAX); o.h_tot = c.take<unsigned long long>(4); o.h_count = c.take<uint32_t>(FO_TOP_MAX); o.h_slot_w = c.take<uint32_t>(n_slots);
        return (size_t)(c.at - (uintptr_t)base);
    };
    o.mem_bytes = carve(nullptr);
    if (o.mem.ensure(o.mem_bytes) || o.host.ensure(carve_host(nullptr)) || o.word.ensure(1)) return GUBER_E_NOMEM;
    carve(o.mem.p); carve_host(o.host.p);
    memset((void*)o.word.p, 0, sizeof(FrontHost));
    HIPCHK(hipMemsetAsync(o.mem.p, 0, o.mem_bytes, f->rs));
    HIPCHK(hipStreamSynchronize(f->rs));
    o.n_slots = n_slots; o.generations = 0; o.since = 0;
    return 0;
}
extern "C" int guber_front_observe(guber_front_t* f, uint32_t every) {
    if (!f) return fail(GUBER_E_INVALID_ARG, "null front");
    std::lock_guard<std::mutex> lk(f->mu);
    if (every == 0) { f->ob.every = 0; f->ob.since = 0; f->ob.skip_one = false; return GUBER_OK; }
    if (f->eng.size() < 2 || !f->have_rule || f->rule.n_shards < 2) return fail(GUBER_E_INVALID_ARG, "guber_front_observe: a front of several engines with a placement's rule");
    if (hipSetDevice(f->device) != hipSuccess) return fail(GUBER_E_HIP, "hipSetDevice");
    const int rc = front_observe_ensure(f);
    if (rc) return rc;
    f->ob.no_agg = guber_lab_env("GUBER_FRONT_OBSERVE_NO_AGG") != nullptr;   // (the laboratory build's measure of the per-tile aggregation)
    f->ob.every = every; f->ob.since = 0;
    return GUBER_OK;
}
// (f->mu held, the device set, the window allocated) k_fr_observe_top behind everything the window's generations left on the routing
// stream; on return its report is in f->ob's pinned memory, *n_top candidates of it, and the window's memory is being cleared on the stream
static int front_observe_end(guber_front* f, uint32_t* n_top, uint32_t* threshold, uint64_t* generations) {
    auto& o = f->ob;
    hipStream_t rs = f->rs;
    if (f->rs2 != rs) HIPCHK(hipStreamSynchronize(f->rs2));
    // the bar needs the window's total: one small copy (the pass is synchronous anyway)
    static_assert(sizeof(FrObsTot) == 32, "four words per stripe");
    std::vector<FrObsTot> tot(FO_STRIPES);
    HIPCHK(hipMemcpyAsync(tot.data(), o.tot, sizeof(FrObsTot) * FO_STRIPES, hipMemcpyDeviceToHost, rs));
    HIPCHK(hipStreamSynchronize(rs));
    uint64_t observed = 0;
    for (auto& t : tot) observed += t.w[FO_OBSERVED];
    // one eighth of the planner's default bar.  Fewer than 2 x engines x 64 keys can stand at or above it (FO_TOP_MAX's note): all are reported
    static_assert(FO_TOP_MAX >= 2u * MULTI_MEM_MAX * 64u, "every key at the bar has a place in the report");
    const uint64_t bar = std::max<uint64_t>(1, observed / ((uint64_t)f->eng.size() * 64u));
    const uint32_t seq = ++o.seq ? o.seq : ++o.seq;
    FrObsTop T{FO_CELLS, o.n_slots, (uint32_t)std::min<uint64_t>(bar, 0xffffffffu), seq, 0u, o.cell, o.slot_w, o.tot, o.n_top,
               o.h_hash, o.h_count, o.h_slot_w, o.h_tot, &o.word.p->w[0]};
    {
        guber_engine* e0 = f->eng[0];
        std::unique_lock<std::mutex> pl(e0->mu, std::defer_lock);
        if (e0->profiling) pl.lock();
        e0->span_begin(KT_FR_OBSERVE_TOP, FO_CELLS, rs);
        hipLaunchKernelGGL(k_fr_observe_top, dim3(64), dim3(256), 0, rs, T);
        e0->span_end();
        T.phase = 1u;
        e0->span_begin(KT_FR_OBSERVE_TOP, 0, rs);
        hipLaunchKernelGGL(k_fr_observe_top, dim3(1), dim3(256), 0, rs, T);
        e0->span_end();
    }
    if (hipGetLastError() != hipSuccess) return fail(GUBER_E_HIP, "kernel launch");
    const int rc = route_wait_reported(o.word.p, 1, seq, f->device, rs, "guber_front: the observation window did not report");
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(o.mem.p, 0, o.mem_bytes, rs));             // the next window starts from zero
    if (f->rs2 != rs) HIPCHK(hipStreamSynchronize(rs));              // (... also for an odd generation's k_fr_observe on a second routing stream)
    *n_top = (uint32_t)o.word.p->w[0]; *threshold = T.threshold; *generations = o.generations;
    o.generations = 0;
    return 0;
}
extern "C" int guber_front_observation(guber_front_t* f, guber_front_observation_t* out) {
    if (!f || !out) return fail(GUBER_E_INVALID_ARG, "null argument");
    if ((out->slot_cap && !out->slot_w) || (out->cap && (!out->hash || !out->count))) return fail(GUBER_E_INVALID_ARG, "null observation arrays");
    std::lock_guard<std::mutex> lk(f->mu);
    auto& o = f->ob;
    if (!o.mem.p) return fail(GUBER_E_INVALID_ARG, "guber_front_observation: guber_front_observe has never been turned on");
    if (hipSetDevice(f->device) != hipSuccess) return fail(GUBER_E_HIP, "hipSetDevice");
    uint32_t n_top = 0;
    const int rc = front_observe_end(f, &n_top, &out->threshold, &out->generations);
    if (rc) return rc;
    out->observed = o.h_tot[0]; out->skipped = o.h_tot[1]; out->dropped = o.h_tot[2];
    out->n_slots = o.n_slots; out->n = n_top;
    if (out->slot_cap) memcpy(out->slot_w, o.h_slot_w, (size_t)std::min(out->slot_cap, o.n_slots) * 4);
    if (out->cap) { memcpy(out->hash, o.h_hash, (size_t)std::min(out->cap, n_top) * 8); memcpy(out->count, o.h_count, (size_t)std::min(out->cap, n_top) * 4); }
    return GUBER_OK;
}
extern "C" int guber_front_rebalance(guber_front_t* f, guber_placement_t* placement, double heavy_fraction, guber_front_rebalance_stats_t* out) {
    if (out) *out = guber_front_rebalance_stats_t{};
    if (!f || !placement || !out) return fail(GUBER_E_INVALID_ARG, "null argument");
    uint32_t p_shards = 0, p_slots = 0, n_hot = 0;
    if (guber_placement_info(placement, &p_shards, &p_slots, &n_hot)) return fail(GUBER_E_INVALID_ARG, "guber_front_rebalance: no placement");
    std::lock_guard<std::mutex> lk(f->mu);
    auto& o = f->ob;
    if (f->eng.size() < 2 || !f->have_rule) return fail(GUBER_E_INVALID_ARG, "guber_front_rebalance: a front of several engines with a placement's rule");
    if (p_shards != f->rule.n_shards || p_shards > f->eng.size() || p_slots != f->rule.n_shards * f->rule.per)
        return fail(GUBER_E_INVALID_ARG, "guber_front_rebalance: not the placement the front's rule came from (shards, slots)");
    if (!o.mem.p) return fail(GUBER_E_INVALID_ARG, "guber_front_rebalance: guber_front_observe has never been turned on");
    if (hipSetDevice(f->device) != hipSuccess) return fail(GUBER_E_HIP, "hipSetDevice");
    // a generation that was probed or routed ahead followed the rule that is about to change: whoever evaluates it routes it afresh
    // (a probed one was never counted; one routed ahead while observation was on was: the call that routes it again must not count it twice)
    if (f->pre_routed && !f->st.probed && o.ahead_counted) o.skip_one = true;
    f->st.probed = false; f->pre_routed = false; o.ahead_counted = false;
    {
        // every generation in flight, on every slot: what another call holds back for these tables goes first, then the streams run dry
        const int ne = (int)f->eng.size();
        EngineLocks locks(ne, [&](int i) { return f->eng[i]; });
        locks.launch_held_by_others();
        for (auto st : f->streams) HIPCHK(hipStreamSynchronize(st));
        for (hipStream_t st : {f->rs, f->rs2, f->os}) HIPCHK(hipStreamSynchronize(st));
    }
    uint32_t n_top = 0, threshold = 0; uint64_t generations = 0;
    int rc = front_observe_end(f, &n_top, &threshold, &generations);
    if (rc) return rc;
    out->observed = o.h_tot[0]; out->dropped = o.h_tot[2];
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the candidates' hashes as the placement takes them");
    if (guber_placement_observe_aggregate(placement, o.h_slot_w, o.n_slots, (const uint64_t*)o.h_hash, o.h_count, n_top))
        return fail(GUBER_E_INVALID_ARG, "guber_front_rebalance: the placement did not take the window");
    guber_placement_move_t moves[64];
    uint32_t nm = 0;
    rc = guber_placement_plan(placement, heavy_fraction, moves, 64, &nm);
    if (rc) return fail(rc, "guber_front_rebalance: guber_placement_plan");
    nm = std::min(nm, 64u);
    out->moves_planned = nm;
    for (uint32_t q = 0; q < nm; ++q) {
        // (guber_move_items_by_hash takes its two engines in address order: the order next to the front's mutex)
        uint32_t moved = 0;
        int mrc = GUBER_E_INVALID_ARG;
        if (moves[q].from < f->eng.size() && moves[q].to < f->eng.size())
            mrc = guber_move_items_by_hash(f->eng[moves[q].from], f->eng[moves[q].to], &moves[q].key_hash, 1, &moved);
        if (mrc) { (void)guber_placement_cancel(placement, moves[q].key_hash); out->cancelled++; }   // (what was not taken is back in its table)
        else out->buckets_moved++;
    }
    rc = guber_placement_commit(placement);
    guber_route_rule_t rule;
    if (!rc) rc = guber_placement_export(placement, &rule);
    if (rc) return fail(rc, "guber_front_rebalance: commit / export");
    rule.global_engine = f->rule.global_engine;
    rc = front_set_rule(f, &rule);
    if (rc) return rc;
    (void)guber_placement_info(placement, nullptr, nullptr, &n_hot);
    out->n_hot = n_hot;
    return GUBER_OK;
}
