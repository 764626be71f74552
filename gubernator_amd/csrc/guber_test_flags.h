// guber_test_flags.h — bits of guber_config_t.flags that exist for the TEST SUITE (tests/: gubernator_amd.FLAG_TEST_*): each forces a code
// path that production traffic reaches only by size or by accident, so that the parity tests can drive it with small inputs.  Not part
// of the public header (include/guber_gpu.h reserves the bits); a binding never sets them.
#pragma once
#define GUBER_FLAG_TEST_WEAK_HASH 1u    /* keep 6 bits of the key hash so distinct keys collide and the exact-key verification / retry path is exercised */
#define GUBER_FLAG_TEST_FORCE_RADIX 2u  /* evaluate small batches with the large-batch (global radix sort) kernel sequence as well */
#define GUBER_FLAG_TEST_CAREFUL 4u      /* never claim speculatively (the retry-round code path) */
#define GUBER_FLAG_DIR_CLAIMS 16u       /* accepted and ignored (round-1 tuning knob: per-batch claims in the directory entries) */
#define GUBER_FLAG_TEST_NO_SMALL 32u    /* batches of <= 256 requests take the two-launch pipeline too (not the one-launch small path) */
#define GUBER_FLAG_TEST_FORCE_PART 64u  /* every batch (also <= 256 requests, also host-resident ones) takes the owner-partitioned three-launch pipeline */
#define GUBER_FLAG_TEST_LATE_COUNTERS 256u /* the engine's counters start where production is after seconds to days (the values below): nothing else changes */
#define GUBER_FLAG_TEST_FIXED_ARENA 512u /* the long-key arena keeps its first size: no bound asks for a rebuild, no rebuild grows it — so that a full arena and its per-item refusal can be reached */
#define GUBER_FLAG_TEST_LAST_STAMPS 1024u /* the engine's next recency stamp starts 4 096 below the END of the 53 bits (the value below): nothing else changes.  With
                                             GUBER_FLAG_TEST_LATE_COUNTERS (the epochs) this flag's stamp start wins */
// Where an engine created with GUBER_FLAG_TEST_LAST_STAMPS starts: the call that would hand out a stamp above REC_STAMP_MASK renumbers the live
// items' stamps 1..live first (engine_batch.inl stamps_ensure; tests/stamp_end_cases.py positions that call by arithmetic of its own).
#define GUBER_TEST_LAST_SEQ_NEXT ((1ull << 53) - 4096ull) /* guber_engine::seq_next */
// Where an engine created with GUBER_FLAG_TEST_LATE_COUNTERS starts (guber_engine_create; tests/late_counters.py mirrors the four values and
// tests/test_late_counters_cpu.py holds the mirror to this file).  The next 4 096 recency stamps have Rec::pad near 0xffffffff and the twenty
// lower high bits set; stamp 2^52 clears pad, flips every one of those bits and sets bit 52 (Rec::meta bit 31).  A batch takes one epoch and,
// through the two-launch pipeline, one claim epoch; every counter snapshot takes one ring sequence number.
#define GUBER_TEST_LATE_SEQ_NEXT ((1ull << 52) - 4096ull) /* guber_engine::seq_next */
#define GUBER_TEST_LATE_EPOCH (0x7fffffffu - 12u)         /* guber_engine::epoch: the directory's 31-bit epoch (batch_prelude wraps it) */
#define GUBER_TEST_LATE_EPOCH16 (0xffffu - 12u)           /* guber_engine::fast_epoch16: the claim table's 16-bit epoch (plan_fast wraps it) */
#define GUBER_TEST_LATE_RB_SEQ (0xffffffffu - 8u)         /* guber_engine::rb_seq: the snapshot ring's sequence (skips 0) */
