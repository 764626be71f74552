/* guber_wire.h — wire-format front end of the batched rate-limit path (C ABI, host code).
 *
 * What it replaces in the reference: the protobuf unmarshalling of `GetRateLimitsReq` /
 * `GetPeerRateLimitsReq` into one heap-allocated `*RateLimitReq` per item (generated code of
 * gubernator.proto:137-182 / peers.proto:36-44) followed by the per-item validation of
 * `V1Instance.GetRateLimits` (gubernator.go:189-220), and the marshalling of `GetRateLimitsResp` /
 * `GetPeerRateLimitsResp` (gubernator.proto:189-203, peers.proto:46-49).  Here the serialized RPC payload
 * is transcoded straight into the SoA batch `guber_eval_batch` consumes (include/guber_gpu.h) — no per-item
 * allocation — and the SoA results straight back into the serialized response.  Several RPC payloads can
 * be appended to ONE device batch, which lifts the reference's 1000-items-per-RPC cap (gubernator.go:40,189)
 * and 1 MiB receive limit (daemon.go:122) from the device batch size.
 *
 * Wire facts relied upon (proto3): both request messages are `repeated RateLimitReq = 1`, both response
 * messages are `repeated RateLimitResp = 1`, so one decoder / encoder serves the client and the peer RPC.
 *   RateLimitReq : name 1 (LEN), unique_key 2 (LEN), hits 3, limit 4, duration 5 (int64 varint),
 *                  algorithm 6, behavior 7 (enum varint), burst 8 (int64 varint),
 *                  metadata 9 (map entry, skipped: tracing propagation only), created_at 10 (optional int64)
 *   RateLimitResp: status 1 (enum), limit 2, remaining 3, reset_time 4 (int64), error 5 (string),
 *                  metadata 6 (one entry, "owner" -> the owning peer's address, on the answers that were not evaluated as the
 *                  arrival instance's own: guber_wire_encode_responses_owner, guber_wire_dev_eval_mesh_enc; no other entry is ever set)
 * Unknown fields are skipped by wire type, the last occurrence of a singular field wins, zero-valued
 * response fields are omitted and fields are written in field-number order — the bytes equal what the
 * protobuf runtimes produce for the same message.
 *
 * Conventions: as guber_gpu.h (0 or negative code, never throws, caller-owned buffers, no pointer kept).
 */
#ifndef GUBER_WIRE_H
#define GUBER_WIRE_H

#include <stddef.h>
#include <stdint.h>

#include "guber_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GUBER_E_WIRE_MALFORMED (-20)   /* truncated / invalid protobuf; nothing was appended */
#define GUBER_E_WIRE_TOO_LARGE (-21)   /* more than max_per_rpc items: gubernator.go:189-193 (codes.OutOfRange) */
#define GUBER_E_WIRE_FULL (-22)        /* the batch has no room for this payload; nothing was appended: flush, reset, retry */
#define GUBER_E_WIRE_CLOSED (-23)      /* guber_wire_pool: the pool is being destroyed */
#define GUBER_PENDING 1                /* guber_wire_dev_*_collect(wait = 0): the GPU is still at it */

#define GUBER_WIRE_PINNED 1u           /* allocate the SoA with guber_alloc_pinned (needs a HIP device) */

/* per-item validation outcome of gubernator.go:207-217, kept next to the SoA */
#define GUBER_WIRE_PRE_OK 0
#define GUBER_WIRE_PRE_EMPTY_UNIQUE_KEY 1   /* "field 'unique_key' cannot be empty" */
#define GUBER_WIRE_PRE_EMPTY_NAME 2         /* "field 'namespace' cannot be empty" */

/* what a request message is, one byte per RPC: the per-RPC byte of the device decoder (guber_wire_dev_decode*'s is_owner[]) and of the
 * payload stage.  Bit 0: RateLimitReqState.IsOwner of its items.  Bit 1: the message is a GetPeerRateLimitsReq and is served as
 * V1Instance.GetPeerRateLimits serves it (gubernator.go:462-539) — no per-item validation (an item with an empty name or unique_key is
 * evaluated on the key name + "_" + unique_key, client.go:39), Behavior_DRAIN_OVER_LIMIT ORed into every item that carries Behavior_GLOBAL
 * (:506-512: peers accumulate hits and may ask for more than remains), items evaluated as the owner (:486: the peer bit implies the owner
 * bit).  0 and 1 mean what they always meant. */
#define GUBER_WIRE_RPC_OWNER 1u
#define GUBER_WIRE_RPC_PEER 2u

typedef struct guber_wire_batch guber_wire_batch_t;

/* A growable-up-to-capacity SoA batch plus the result arrays of its evaluation. */
int guber_wire_batch_create(uint32_t max_items, uint32_t max_key_bytes, uint32_t flags, guber_wire_batch_t** out);
void guber_wire_batch_destroy(guber_wire_batch_t* b);
/* Empty the batch and set the clock of the next evaluation: MillisecondNow() for expiry (lrucache.go:106)
 * and the CreatedAt default of items that carry none (gubernator.go:218-220). */
void guber_wire_batch_reset(guber_wire_batch_t* b, int64_t now_ms);
uint32_t guber_wire_batch_size(const guber_wire_batch_t* b);

/* Append every RateLimitReq of one serialized GetRateLimitsReq / GetPeerRateLimitsReq.
 *   max_per_rpc  0 = no cap; the reference passes 1000 (gubernator.go:40) -> GUBER_E_WIRE_TOO_LARGE
 *   is_owner     RateLimitReqState.IsOwner of these items (gubernator.go:246, 489)
 *   *first,*count  the slice [first, first+count) of the batch this payload occupies (responses are
 *                  positionally aligned, gubernator.proto:51-54)
 * Items failing the reference's validation keep their position with an empty key; they are answered with
 * the reference's error text by guber_wire_encode_responses and never reach a bucket. */
int guber_wire_decode_requests(guber_wire_batch_t* b, const uint8_t* msg, size_t len, uint32_t max_per_rpc,
                               uint8_t is_owner, uint32_t* first, uint32_t* count);

/* The same for one GetPeerRateLimitsReq served as the reference's peer RPC serves it (GUBER_WIRE_RPC_PEER above): every item gets its key
 * ("name_", "_ukey" or "_" when a half is empty) and no validation code, GLOBAL items get DRAIN_OVER_LIMIT, is_owner = 1; the CreatedAt
 * default (gubernator.go:514-518) and max_per_rpc are as above — GUBER_E_WIRE_TOO_LARGE is the same code, the caller picks the text
 * ("'PeerRequest.rate_limits' list too large; max size is '1000'", gubernator.go:465). */
int guber_wire_decode_peer_requests(guber_wire_batch_t* b, const uint8_t* msg, size_t len, uint32_t max_per_rpc,
                                    uint32_t* first, uint32_t* count);

/* The SoA view to hand to guber_eval_batch (valid until the next reset / decode), the result arrays an
 * evaluation fills, and the per-item validation codes. */
const guber_batch_t* guber_wire_batch_view(guber_wire_batch_t* b);
guber_result_t* guber_wire_batch_result(guber_wire_batch_t* b);
const uint8_t* guber_wire_batch_pre_errors(const guber_wire_batch_t* b);

/* guber_eval_batch(e, view, result) on the batch's own arrays. */
int guber_wire_eval(guber_engine_t* e, guber_wire_batch_t* b);

/* Serialize the responses of the slice [first, first+count) as GetRateLimitsResp (= GetPeerRateLimitsResp).
 *   wrap_errors  1 = local path: errors of the evaluation are wrapped as
 *                "Error while apply rate limit for '<key>': <text>" (gubernator.go:250-255); 0 = peer path
 * Returns GUBER_E_NOMEM when cap is too small; *len then holds the size needed. */
size_t guber_wire_encode_bound(const guber_wire_batch_t* b, uint32_t first, uint32_t count);
int guber_wire_encode_responses(const guber_wire_batch_t* b, uint32_t first, uint32_t count, int wrap_errors,
                                uint8_t* out, size_t cap, size_t* len);

/* The same as GetPeerRateLimitsResp with the peer RPC's error texts: an item's error is wrapped as "Error in getLocalRateLimit: "
 * (gubernator.go:523) around "during workerPool.GetRateLimit: " (:600) around the worker's text; the two Gregorian errors, which come out
 * of an algorithm, carry "Error in tokenBucket: " / "Error in leakyBucket: " (workers.go:302-313) in front of theirs.  The engine's own
 * errors (table full, key too long), which the reference does not have, get the two outer wrappers.  guber_wire_encode_bound covers it. */
int guber_wire_encode_peer_responses(const guber_wire_batch_t* b, uint32_t first, uint32_t count, uint8_t* out, size_t cap, size_t* len);

/* Responses with the OWNER'S ADDRESS: guber_wire_encode_responses for an instance of a cluster.  The reference puts
 * metadata{"owner": <owner's GRPCAddress>} on every answer that was not evaluated as the arrival instance's own: forwarded items
 * (gubernator.go:379-381) and Behavior_GLOBAL items answered from a non-owner's replica (:267-268).
 *   owner_rank[k]  the ring's owner of item first + k (a peer index below n_ranks; 0xFF = none: a key the ring cannot place) — what
 *                  guber_ring_route or guber_wire_dev_eval_mesh_enc's owner_rank gives
 *   self_rank      the instance the payload arrived at;  owner_addr[p]: the name peer p was given in guber_ring_create
 * Per item, in this order:
 *   1  pre-rejected (empty unique_key / name), a dead slot, or owner_rank 0xFF   error text as guber_wire_encode_responses, no metadata
 *   2  owner_rank == self_rank                                                   as guber_wire_encode_responses (wrap_errors honoured), no metadata
 *   3  a plain item of another owner (forwarded)        error text exactly guber_wire_encode_peer_responses' (gubernator.go:523 around :600:
 *                                                       the owner's GetPeerRateLimits produced it, asyncRequest hands it on), metadata
 *   4  Behavior_GLOBAL, another owner                   "Error in getGlobalRateLimit: during in getLocalRateLimit: " + what the peer text has
 *                                                       behind "Error in getLocalRateLimit: " (gubernator.go:261, :416, :600), metadata
 * An answer with an error carries the error (field 5) and the metadata (field 6) and no other field.  Field 6 is one map entry,
 *   32 <varint entry_len> 0a 05 "owner" 12 <varint addr_len> <addr>
 * behind field 5.  An address has 1 .. GUBER_WIRE_OWNER_ADDR_MAX bytes (a 253-byte host name, ':', five digits, rounded up to 8): entry_len and
 * addr_len take two bytes from 128 on, a suffix is at most 277 bytes, a body without an error at most 35 + 277 = 312 — its length prefix two
 * bytes from 128 on — and such an item at most 315.  GUBER_E_INVALID_ARG: a NULL, empty or over-long address, self_rank or an owner_rank
 * outside the ranks.  guber_wire_encode_bound_owner = guber_wire_encode_bound + the longest suffix per item (0: refused arguments). */
#define GUBER_WIRE_OWNER_ADDR_MAX 264
size_t guber_wire_encode_bound_owner(const guber_wire_batch_t* b, uint32_t first, uint32_t count, const char* const* owner_addr, uint32_t n_ranks);
int guber_wire_encode_responses_owner(const guber_wire_batch_t* b, uint32_t first, uint32_t count, int wrap_errors,
                                      const uint8_t* owner_rank /* [count], 0xFF = none */, uint32_t self_rank,
                                      const char* const* owner_addr, uint32_t n_ranks,
                                      uint8_t* out, size_t cap, size_t* len);

/* ---- UpdatePeerGlobals (peers.proto:51-63; sender global.go:234-283 broadcastPeers, receiver gubernator.go:425-459) ----
 * The third payload kind that touches the path: the owner of GLOBAL keys broadcasts their state, every other peer
 * installs it in its cache.
 *   UpdatePeerGlobalsReq: globals 1 (repeated UpdatePeerGlobal)
 *   UpdatePeerGlobal    : key 1 (string), status 2 (RateLimitResp), algorithm 3 (enum), duration 4, created_at 5 (int64)
 *
 * guber_wire_encode_globals  the sender side: one UpdatePeerGlobal per update row (key, algorithm, duration, created_at
 *     of the queued request — what guber_global_take role 2 returns) with `status` = the owner's hits = 0 read of the
 *     bucket; rows whose status read failed (status->err[i] != 0) are skipped (global.go:246-249).
 *     GUBER_E_NOMEM + *len = size needed when cap is too small.
 * guber_wire_decode_globals  the receiver side: the CacheItem of every global exactly as UpdatePeerGlobals builds it
 *     (ExpireAt = status.reset_time; leaky: Remaining = float64(status.remaining), Burst = Limit = status.limit,
 *     UpdatedAt = now; token: Status, Limit, Remaining from status, CreatedAt = now; Duration = the message's; any other
 *     algorithm: an item without a value), as a guber_item_t array ready for guber_add_items.  The array and the key
 *     bytes it points to belong to `items` and stay valid until the next decode into it or its destruction. */
typedef struct guber_wire_items guber_wire_items_t;
int guber_wire_items_create(uint32_t max_items, uint32_t max_key_bytes, guber_wire_items_t** out);
void guber_wire_items_destroy(guber_wire_items_t* items);
int guber_wire_decode_globals(guber_wire_items_t* items, const uint8_t* msg, size_t len, int64_t now_ms,
                              const guber_item_t** out, uint32_t* count);
int guber_wire_encode_globals(const uint8_t* key_bytes, const uint32_t* key_off, const uint8_t* algorithm,
                              const int64_t* duration, const int64_t* created_at, const guber_result_t* status, uint32_t n,
                              uint8_t* out, size_t cap, size_t* len);

/* ---- the same decode ON THE DEVICE (gubernator_amd/csrc/guber_kernels_wire.h): the serialized payloads of many RPCs -> one batch in
 *      HBM, evaluated where it is.  The reference unmarshals every RateLimitReq into a heap object on the CPU (generated code of
 *      gubernator.proto:137-182) and validates it there (gubernator.go:189-220); here a workgroup per 8 KB window of a payload finds its part of
 *      the record chain (a wave per payload walks it where it holds anything but plain records), a thread per item parses its record (the same source as guber_wire_decode_requests) and the items land in the structure of
 *      arrays the engine's kernels read.
 *   guber_wire_dev_create   a decoder bound to an engine: at most max_items items, max_payload_bytes payload bytes and max_rpcs
 *                           payloads per decode (max_items <= the engine's max_batch; an RPC holds at most min(max_items, 4096) items)
 *   guber_wire_dev_decode   nrpc payloads (msgs[r], lens[r]; is_owner[r] = RateLimitReqState.IsOwner of its items, NULL = all owner —
 *                           the byte is the flag byte above: GUBER_WIRE_RPC_OWNER | GUBER_WIRE_RPC_PEER decodes payload r as the peer RPC
 *                           does, in k_wire_fill, from the byte it loads anyway; guber_wire_dev_decode_staged[_async] alike;
 *                           max_per_rpc as guber_wire_decode_requests) -> per RPC: status[r] (GUBER_OK, GUBER_E_WIRE_MALFORMED,
 *                           GUBER_E_WIRE_TOO_LARGE), first[r], count[r] = the slice of the batch its items occupy (responses are
 *                           positionally aligned); *n_items = the batch size.  Items of a rejected RPC that were already placed stay
 *                           as dead slots (pre_err GUBER_WIRE_PRE_DEAD, empty key): they never reach a bucket.
 *   guber_wire_dev_buffer / guber_wire_dev_decode_staged   the decoder's own pinned staging buffer, and the decode of payloads that
 *                           already lie in it (offs[r] 16-byte aligned, ascending, not overlapping, 16 bytes of room behind the
 *                           last): a receive path that reads its sockets straight into the buffer skips guber_wire_dev_decode's copy
 *   guber_wire_dev_eval     the batch through the engine (as guber_eval_batch_dev), results to host arrays of n_items entries
 *   guber_wire_dev_eval_front  the batch through a front over several engines: decode, routing, evaluation and the answers' order in HBM
 *   guber_wire_dev_eval_mesh   the last decodes of one decoder per rank through a mesh of fronts (include/guber_gpu.h guber_mesh_*): every
 *                           item is evaluated on the rank the ring names and answered where its payload arrived — the decision WHERE a
 *                           payload's items go (gubernator.go:236-283), taken on the device
 *   guber_wire_dev_eval_mesh_enc  the same, answered as serialized GetRateLimitsResp bytes with the owner's address on every answer another
 *                           rank owns (metadata "owner"): encoded on the device, RPC by RPC
 *   guber_wire_dev_columns  the decoded columns copied to host memory (keys as rows of key_stride bytes + key_len): what
 *                           guber_wire_encode_responses-style code and the tests read */
#define GUBER_WIRE_PRE_DEAD 255
typedef struct guber_wire_dev guber_wire_dev_t;
typedef struct {
    uint32_t n, key_stride;
    const uint8_t* key_rows; const uint32_t* key_len;
    const int64_t *hits, *limit, *duration, *burst, *created_at;
    const uint32_t* behavior; const int32_t* algo_raw;
    const uint8_t *algorithm, *is_owner, *pre_err;
} guber_wire_columns_t;
int guber_wire_dev_create(guber_engine_t* e, uint32_t max_items, uint32_t max_payload_bytes, uint32_t max_rpcs, guber_wire_dev_t** out);
void guber_wire_dev_destroy(guber_wire_dev_t* d);
int guber_wire_dev_decode(guber_wire_dev_t* d, const uint8_t* const* msgs, const uint32_t* lens, uint32_t nrpc, const uint8_t* is_owner,
                          uint32_t max_per_rpc, int64_t now_ms, int32_t* status, uint32_t* first, uint32_t* count, uint32_t* n_items);
int guber_wire_dev_buffer(guber_wire_dev_t* d, uint8_t** buf, size_t* cap);
int guber_wire_dev_decode_staged(guber_wire_dev_t* d, const uint32_t* offs, const uint32_t* lens, uint32_t nrpc, const uint8_t* is_owner,
                                 uint32_t max_per_rpc, int64_t now_ms, int32_t* status, uint32_t* first, uint32_t* count, uint32_t* n_items);
int guber_wire_dev_eval(guber_wire_dev_t* d, guber_result_t* r);
/* the decoded batch through a front (include/guber_gpu.h guber_front_*) instead: routed to the front's engines on the device, evaluated there,
 * answered in the order of the RPCs' items; results to host arrays of n_items entries (n_items <= the front's max_n) */
int guber_wire_dev_eval_front(guber_wire_dev_t* d, guber_front_t* f, guber_result_t* r);
/* the decoded batches of decs[r] — the payloads that ARRIVED at rank r; NULL, or nothing decoded: nothing arrived there — through a mesh of
 * fronts: each decoder's last decode is its rank's generation (its key rows, its columns, the decode's now_ms) for guber_mesh_eval_rows_dev;
 * synchronous: results[r] are HOST arrays of decs[r]'s n_items entries, answered in the order of the RPCs' items, aggregate counters zero.
 * The ring decides ownership, so the decoder's per-item is_owner is not handed on: a decode that carried a GUBER_WIRE_RPC_PEER payload is
 * refused (a peer RPC's items are evaluated where they arrive, gubernator.go:486: guber_wire_dev_eval_front).  Pre-rejected items and the
 * dead slots of a rejected RPC have empty keys: they stay on their arrival rank, keep their place and earn the front's item error.
 * GUBER_E_INVALID_ARG before anything is enqueued: a NULL argument, a decoder with an uncollected asynchronous call, the same decoder at
 * two ranks, a decoder whose engine is on another device than its rank's front, two non-empty decoders with different now_ms, a missing
 * result array where n_items > 0; GUBER_E_BATCH_TOO_LARGE: n_items above the mesh's max_n. */
int guber_wire_dev_eval_mesh(guber_wire_dev_t* const* decs /* [n_ranks] */, guber_mesh_t* m, guber_result_t* results /* [n_ranks] */);
/* The same with SERIALIZED RESPONSES: what V1Instance.GetRateLimits hands its gRPC layer in a cluster, with nothing per item on the host.  After
 * the mesh's last hop every rank's answers are encoded on its device (k_wire_enc_owner: one workgroup per RPC, the peers' metadata suffixes
 * copied from a table in LDS; the ring's owner per item is k_mx_count's optional output) into pinned memory of the decoder, and every RPC's
 * GetRateLimitsResp — guber_wire_encode_responses_owner's bytes, with rank r as self_rank — is copied to out[r].buf, back to back:
 *   out[r].off[q], out[r].len[q]   RPC q of decs[r]'s last decode (len 0: the decode turned it away, or it holds no item)
 *   out[r].owner_rank              optional: [n_items] the ring's owner per item, 0xFF = none
 * An RPC with an item error is re-decoded from the decoder's staging buffer by the host transcoder and written by
 * guber_wire_encode_responses_owner (the texts need the item's key).  owner_addr[p] is the name peer p was given in guber_ring_create.
 * out[r].cap >= guber_wire_dev_mesh_enc_bound(decs[r], owner_addr, n_ranks): the worst case INCLUDING error texts for the decoder's last
 * decode (0: nothing to answer, or refused addresses) — the call never finds a buffer too small after decisions have been applied, and the
 * host transcoder's batch is allocated before anything is enqueued.  (What can still fail afterwards is a HIP error, or the device's and the
 * host's decoders disagreeing about a payload, GUBER_E_HIP: a defect, not a condition of the input.)
 * Synchronous; refuses what guber_wire_dev_eval_mesh refuses and, as GUBER_E_INVALID_ARG, a NULL, empty or over-long address or a missing
 * out array; a cap below the bound is GUBER_E_NOMEM.  Every refusal comes before anything is enqueued: no engine is touched. */
typedef struct guber_wire_mesh_resp {
    uint8_t* buf; size_t cap;          /* caller's host memory for rank r's responses */
    uint32_t *off, *len;               /* [RPCs of decs[r]'s last decode]: RPC q's GetRateLimitsResp = buf + off[q], len[q] bytes */
    uint8_t* owner_rank;               /* optional, [n_items]: the ring's owner per item, 0xFF = none */
} guber_wire_mesh_resp_t;
size_t guber_wire_dev_mesh_enc_bound(const guber_wire_dev_t* d, const char* const* owner_addr, uint32_t n_ranks);
/* DIAGNOSTIC, not part of the serving interface (tests and measurements read them):
 *   guber_wire_dev_mesh_enc_host_rpcs  how many RPCs of d's last guber_wire_dev_eval_mesh_enc the host transcoder wrote (they held an item
 *                                      error); the device wrote the others
 *   guber_wire_dev_mesh_enc_piece      the items k_wire_enc_owner encodes per piece: RPCs around it are the encoder's edge cases */
uint32_t guber_wire_dev_mesh_enc_piece(void);
uint32_t guber_wire_dev_mesh_enc_host_rpcs(const guber_wire_dev_t* d);
int guber_wire_dev_eval_mesh_enc(guber_wire_dev_t* const* decs, guber_mesh_t* m, const char* const* owner_addr /* [n_ranks] */,
                                 int wrap_errors, guber_wire_mesh_resp_t* out /* [n_ranks] */);
int guber_wire_dev_columns(guber_wire_dev_t* d, guber_wire_columns_t* c);
/* The same in two halves each, for a caller that keeps several decoders busy and never blocks on the GPU (the payload stage below):
 *   guber_wire_dev_set_stream           the decode's copies and kernels go to `stream` (hipStream_t) instead of the engine's stream
 *   guber_wire_dev_decode_staged_async  guber_wire_dev_decode_staged up to its last enqueue (is_owner stays valid until collected)
 *   guber_wire_dev_decode_collect       wait = 0: GUBER_PENDING while the GPU is at it; GUBER_OK: the verdicts, as guber_wire_dev_decode_staged
 *   guber_wire_dev_eval_front_async     guber_wire_dev_eval_front, enqueued only; r's arrays are DEVICE-VISIBLE (HBM, or pinned host memory the
 *                                       answers' last hop writes in place over PCIe): no copy follows
 *   guber_wire_dev_eval_collect         wait = 0: GUBER_PENDING while the answers are on their way
 *   guber_wire_dev_route_front_async    optional, before guber_wire_dev_eval_front_async: only the front's routing of the decoded batch, enqueued;
 *   guber_wire_dev_route_ready          GUBER_PENDING until the shares' sizes are in host memory (the evaluation's enqueue then waits for nothing).
 *                                       Nothing else may go through the front between the two calls. */
int guber_wire_dev_set_stream(guber_wire_dev_t* d, void* stream);
int guber_wire_dev_decode_staged_async(guber_wire_dev_t* d, const uint32_t* offs, const uint32_t* lens, uint32_t nrpc, const uint8_t* is_owner,
                                       uint32_t max_per_rpc, int64_t now_ms);
int guber_wire_dev_decode_collect(guber_wire_dev_t* d, int wait, int32_t* status, uint32_t* first, uint32_t* count, uint32_t* n_items);
int guber_wire_dev_eval_front_async(guber_wire_dev_t* d, guber_front_t* f, guber_result_t* r);
int guber_wire_dev_eval_collect(guber_wire_dev_t* d, int wait);
int guber_wire_dev_route_front_async(guber_wire_dev_t* d, guber_front_t* f);
int guber_wire_dev_route_ready(guber_wire_dev_t* d, guber_front_t* f);

/* ---- the payload stage: V1Instance.GetRateLimits / GetPeerRateLimits on the SERIALIZED messages (gubernator.go:183-306, :470-520; the batching
 *      shape is peer_client.go:284-337's: a queue that leaves when it is full or BatchWait after its first entry — here RPCs are the entries).
 *      Caller threads (the gRPC handlers: a codec that hands the handler the raw bytes) call guber_wire_pool_get_rate_limits concurrently; per RPC the
 *      host does one compare-and-swap (a place in the open stage) and two memcpys (the payload into pinned memory, the response out of it).
 *      Unmarshalling, validation, the CreatedAt default, HashKey, the worker's choice by XXH64 (workers.go:180-184), the evaluation, the
 *      answers' order and the marshalling of GetRateLimitsResp (gubernator.proto:184-203) all happen on the device: k_wire_* -> guber_front ->
 *      k_wire_enc, which writes every RPC's response bytes in place into host memory.  (An RPC with an item error is marshalled by the host
 *      transcoder from the raw answers: the error's text needs the item's key.)  An RPC of at most FOUR requests that finds at most eight calls inside the
 *      pool skips the stages: its caller evaluates it through the engine's one-launch path (host transcoder, the placement's rule on the host,
 *      guber_eval_batch) — 12 us instead of a stage's 90; same bytes.
 *   guber_wire_pool_create            over the engines of ONE device and the placement's rule (as guber_front_create; rule NULL with one engine);
 *                                     cfg NULL or zero fields = defaults.  Two threads per pool (intake, front); neither ever blocks on the GPU.
 *   guber_wire_pool_get_rate_limits   req/len: one serialized GetRateLimitsReq (= GetPeerRateLimitsReq); is_owner: RateLimitReqState.IsOwner of its
 *                                     items; wrap_errors as guber_wire_encode_responses.  Blocks until the stage the payload joined has been
 *                                     through the GPU.  resp/cap: at least guber_wire_pool_response_bound(req, len) bytes — a smaller buffer is
 *                                     refused before anything is evaluated when it cannot even hold error-free answers; when it turns out too small
 *                                     for the error texts the call returns GUBER_E_NOMEM AFTER the decisions have been applied.
 *                                     GUBER_E_WIRE_MALFORMED / GUBER_E_WIRE_TOO_LARGE: the message is turned away whole (nothing of it evaluated),
 *                                     as the protobuf runtime / gubernator.go:189-193 do.  The bytes equal guber_wire_encode_responses' (and the
 *                                     protobuf runtimes').
 *   guber_wire_pool_get_peer_rate_limits  req/len: one serialized GetPeerRateLimitsReq, answered as V1Instance.GetPeerRateLimits answers it
 *                                     (gubernator.go:462-539; GUBER_WIRE_RPC_PEER above: no validation, DRAIN_OVER_LIMIT on GLOBAL items, the peer
 *                                     RPC's error texts).  Everything else — stages, the caller's own evaluation of a small RPC, routing of GLOBAL items
 *                                     to the GLOBAL engine and its update queue, buffers, codes — as guber_wire_pool_get_rate_limits; for
 *                                     GUBER_E_WIRE_TOO_LARGE the caller answers "'PeerRequest.rate_limits' list too large; max size is '1000'" (:465).
 *   guber_wire_pool_update_peer_globals   msg/len: one serialized UpdatePeerGlobalsReq (gubernator.go:425-459).  Decoded by guber_wire_decode_globals at
 *                                     the pool's clock; every item goes to the engine the pool's rule keeps GLOBAL state in — the GLOBAL engine when
 *                                     the rule has one, else the table XXH64 of the key picks, as for a GLOBAL request — and is installed there by ONE
 *                                     guber_add_items per engine touched (LRUCache.Add, item by item in the message's order).  Safe beside stages in
 *                                     flight and callers evaluating their own RPCs: guber_add_items takes the engine's lock, as every evaluation
 *                                     does.  *installed (may be NULL) = the items installed.  A malformed message (GUBER_E_WIRE_MALFORMED), or one with
 *                                     an item no table can hold (an empty key: GUBER_E_INVALID_ARG; a key longer than max_key_bytes:
 *                                     GUBER_E_KEY_TOO_LONG), is turned away whole: nothing is installed.  The decode stays on the HOST on purpose: a
 *                                     broadcast holds at most 1000 items per sync interval (global.go:234-283, GlobalBatchLimit), microseconds of work.
 *   guber_wire_pool_set_clock         0 = the wall clock (clock.Now(): a stage's items share the instant it was sealed); otherwise a frozen clock
 *                                     in ms, as the reference's tests use clock.Freeze
 *   What this surface does NOT do: the Store's write-through callbacks (store.go:49-65: guber_pool_set_store / guber_eval_batch_store — a daemon
 *   with conf.Store keeps the per-request pool) (the front below it has it: guber_front_eval_store_dev), metadata propagation (RateLimitReq.metadata is skipped), and the decision WHERE a payload goes
 *   (forwarding to the owning peer, gubernator.go:236-283: this pool evaluates only what its instance owns, the Go front end hands
 *   over just that; the payload stage that takes the decision on the devices is guber_wire_mesh_pool_* below).  Behavior_GLOBAL items
 *   are evaluated on their table and queued for the GLOBAL exchange by the engine as on every other entry point (guber_global_take / _sync);
 *   a rule whose global_engine is set sends them to the device's GLOBAL engine. */
typedef struct guber_wire_pool guber_wire_pool_t;
typedef struct guber_wire_pool_config {
    uint32_t stages;             /* payload stages in rotation (one fills while the others are on the GPU); 0 = 12, 2 .. 12 */
    uint32_t max_items;          /* items a stage holds; 0 = 49 152 — what the front evaluates as one pair of launches for all tables (<= 1 048 575) */
    uint32_t max_payload_bytes;  /* payload bytes a stage holds; 0 = 8 MiB (<= 16 MiB) */
    uint32_t max_rpcs;           /* RPCs a stage holds; 0 = 1024 (<= 4095) */
    uint32_t batch_wait_us;      /* a stage leaves at the latest this long after its first payload; 0 = 500 (BatchWait, config.go:131) */
    uint32_t max_per_rpc;        /* 0 = 1000 (gubernator.go:40); 0xffffffff = no cap */
    uint32_t spin_us;            /* how long a waiting caller looks before it sleeps — when there are CPUs to look with: callers beyond half of them sleep at once; 0 = 150 */
    uint32_t decodes_queued;     /* a stage leaves early — before it is full or BatchWait is over — while fewer than this many stages are waiting for or
                                  * in their decode: 1 = one decode at a time (smallest latency under light load), 0 = 2 (the decoder's stream never idles) */
} guber_wire_pool_config_t;
typedef struct guber_wire_pool_stats {
    uint64_t rpcs, items, stages;                       /* answered so far */
    uint64_t sealed_full, sealed_wait, sealed_idle;     /* why stages left: full / BatchWait / the decoder was idle */
    uint64_t open_waits;                                /* callers that slept because every stage was on the GPU */
    uint64_t fill_us_sum, decode_us_sum, eval_us_sum;   /* per stage: first payload -> sealed; sealed -> decoded; decoded -> answers in host memory */
    uint64_t host_decode_ns, host_route_ns, host_eval_ns; /* the pool's threads' own time inside the three enqueueing calls */
} guber_wire_pool_stats_t;
int guber_wire_pool_create(guber_engine_t* const* engines, uint32_t n_engines, const struct guber_route_rule* rule, const guber_wire_pool_config_t* cfg,
                           guber_wire_pool_t** out);
void guber_wire_pool_destroy(guber_wire_pool_t* p);     /* no call may be in flight or arrive any more */
int guber_wire_pool_get_rate_limits(guber_wire_pool_t* p, const uint8_t* req, size_t len, int is_owner, int wrap_errors, uint8_t* resp, size_t cap,
                                    size_t* resp_len);
int guber_wire_pool_get_peer_rate_limits(guber_wire_pool_t* p, const uint8_t* req, size_t len, uint8_t* resp, size_t cap, size_t* resp_len);
int guber_wire_pool_update_peer_globals(guber_wire_pool_t* p, const uint8_t* msg, size_t len, uint32_t* installed);
size_t guber_wire_pool_response_bound(const uint8_t* req, size_t len);
int guber_wire_pool_set_clock(guber_wire_pool_t* p, int64_t now_ms);
int guber_wire_pool_stats(guber_wire_pool_t* p, guber_wire_pool_stats_t* out);

/* ---- the payload stage over a MESH: RPC bytes in at any rank, response bytes out.  guber_wire_pool above serves the engines of one device;
 *      this one lies over a guber_mesh_t (include/guber_gpu.h: one front per rank, the ring's peers), so that on a node with several GPUs the
 *      handler threads hand the bytes of their GetRateLimitsReq to ANY rank and get GetRateLimitsResp bytes back, with metadata{"owner": <address>}
 *      on every answer another rank owns — exactly guber_wire_dev_eval_mesh_enc's bytes with self_rank = the rank the RPC arrived at.  Decode, the
 *      ring's owner decision (gubernator.go:236-283), the evaluation on the owner, the answers' order and the marshalling stay on the devices
 *      (k_wire_* -> k_mx_count / k_mx_scan / k_mx_pack -> the owners' fronts -> k_mx_apack / k_mx_out -> k_wire_enc_owner).
 *   guber_wire_mesh_pool_create            over a mesh the caller keeps (the pool owns neither the mesh nor its fronts nor their engines, and is
 *                                          destroyed before them); owner_addr[r]: the name peer r has in the ring.  sets x n_ranks decoders, each
 *                                          bound to the first engine of its rank's front; the owners' suffix table is uploaded once.  One
 *                                          dispatcher thread; it may block on the GPU.  GUBER_E_INVALID_ARG: a NULL argument, a NULL, empty or
 *                                          over-long address, a field outside its range, max_items above the mesh's max_n or above the
 *                                          max_batch of a rank's decoder engine.
 *   guber_wire_mesh_pool_get_rate_limits   rank: where the RPC arrived (the handler picks it, round robin for instance); req/len: one serialized
 *                                          GetRateLimitsReq.  Blocks until the stage set the payload joined has been through the GPUs.  A stage
 *                                          set is one stage per rank; it leaves when a rank's stage cannot take the RPC that asks, batch_wait_us
 *                                          after its first payload, or at once while no set is on the GPUs.  The clock is read once per set, when
 *                                          it is sealed.  Within a rank's stage items keep the order the places were taken; between ranks the
 *                                          mesh's rule holds (owner o takes source 0, 1, ... W-1); sets are evaluated in the order they were
 *                                          sealed: a call that has returned was evaluated before any call that starts later.
 *                                          cap >= guber_wire_mesh_pool_response_bound(p, req, len), or GUBER_E_NOMEM (*resp_len = the bound) BEFORE
 *                                          the RPC joins a set: nothing is ever found too small after decisions have been applied.  Turned away
 *                                          whole, the set's other RPCs unaffected: GUBER_E_WIRE_MALFORMED; GUBER_E_WIRE_TOO_LARGE (more than
 *                                          min(max_items, 4096, max_per_rpc) items); GUBER_E_WIRE_FULL (a payload no empty stage can hold, at the
 *                                          door).  len == 0: an empty response, no set.  GUBER_E_INVALID_ARG: a NULL argument, rank >= n_ranks.
 *                                          GUBER_E_WIRE_CLOSED: destroy has begun, or a set failed on the devices — that set's callers get the
 *                                          HIP error, and the pool closes.  An RPC with an item error is marshalled by its CALLER from its own req
 *                                          bytes through the host transcoder (the texts need the keys); the dispatcher does nothing per item.
 *   guber_wire_mesh_pool_response_bound    items (walked, or the cap for long payloads) x (an answer with an error text + the longest owner
 *                                          suffix) + len: everything guber_wire_dev_mesh_enc_bound counts, for one RPC
 *   guber_wire_mesh_pool_set_clock         0 = the wall clock; otherwise a frozen clock in ms, as clock.Freeze
 *   Other threads may keep calling guber_mesh_eval*, guber_add_items and guber_global_sync on the same objects: the mesh's and the engines' locks
 *   serialise them, as beside guber_wire_pool.
 *   What this surface does NOT do: GetPeerRateLimits / UpdatePeerGlobals (every peer of the mesh's ring is a local rank, nobody outside sends
 *   them; guber_wire_pool serves them per device), the Store callbacks, non-blocking dispatch (the dispatcher waits for the GPUs phase by phase), an RCCL transport and one rank per
 *   process (guber_mesh_create_local's ranks live in this process). */
typedef struct guber_wire_mesh_pool guber_wire_mesh_pool_t;
typedef struct guber_wire_mesh_pool_config {
    uint32_t sets;               /* stage sets in rotation (one fills while another is on the GPUs); 0 = 3, 2 .. 8 */
    uint32_t max_items;          /* items one rank's stage holds; 0 = min(49 152, the mesh's max_n, the rank's decoder engine's max_batch) */
    uint32_t max_payload_bytes;  /* per rank and stage; 0 = 8 MiB (<= 16 MiB) */
    uint32_t max_rpcs;           /* per rank and stage; 0 = 1024 (<= 4095) */
    uint32_t batch_wait_us;      /* a set leaves at the latest this long after its first payload; 0 = 500 (BatchWait, config.go:131) */
    uint32_t max_per_rpc;        /* 0 = 1000 (gubernator.go:40); 0xffffffff = no cap */
    uint32_t wrap_errors;        /* as guber_wire_encode_responses_owner, for every RPC of the pool */
} guber_wire_mesh_pool_config_t;
typedef struct guber_wire_mesh_pool_stats {
    uint64_t rpcs, items, sets;                      /* answered so far (an RPC turned away whole counts as an RPC, not as items) */
    uint64_t sealed_full, sealed_wait, sealed_idle;  /* why sets left */
    uint64_t forwarded;                              /* items evaluated on another rank than they arrived at */
    uint64_t host_rpcs;                              /* RPCs with an item error: marshalled by their CALLER through the host transcoder */
    uint64_t open_waits;                             /* callers that had to wait for a set to open */
    uint64_t fill_us_sum, gpu_us_sum;                /* per set: first payload -> sealed; sealed -> answers in host memory */
} guber_wire_mesh_pool_stats_t;
int    guber_wire_mesh_pool_create(guber_mesh_t* m, const char* const* owner_addr /* [n_ranks], the ring's peer names */,
                                   const guber_wire_mesh_pool_config_t* cfg /* NULL = defaults */, guber_wire_mesh_pool_t** out);
void   guber_wire_mesh_pool_destroy(guber_wire_mesh_pool_t* p);   /* no call may be in flight or arrive any more */
int    guber_wire_mesh_pool_get_rate_limits(guber_wire_mesh_pool_t* p, uint32_t rank, const uint8_t* req, size_t len,
                                            uint8_t* resp, size_t cap, size_t* resp_len);
size_t guber_wire_mesh_pool_response_bound(const guber_wire_mesh_pool_t* p, const uint8_t* req, size_t len);
int    guber_wire_mesh_pool_set_clock(guber_wire_mesh_pool_t* p, int64_t now_ms);   /* 0 = wall clock; else frozen, as clock.Freeze */
int    guber_wire_mesh_pool_stats(guber_wire_mesh_pool_t* p, guber_wire_mesh_pool_stats_t* out);
/* Lone small RPCs evaluated by their CALLER (opt-in; off by default, and with it off the pool behaves exactly as without it).  A stage set
 * costs a lone one-item RPC a decode, the mesh's general call, an encoder and the dispatcher's waits.  With max_items != 0 an RPC whose item
 * bound is at most max_items (<= 256), arriving while at most max_calls calls (0 = 8) are inside the pool and the pool is open, joins no set:
 * its caller decodes it with the host transcoder at the pool's clock, evaluates it with guber_mesh_eval_small (include/guber_gpu.h: one
 * launch per rank; the ring's and the fronts' decisions are taken on the devices, as in a set) and writes the bytes
 * guber_wire_encode_responses_owner writes — error texts and metadata{"owner"} included.  Everything a set checks at the door applies
 * unchanged (malformed and too large messages, a cap below the bound, len == 0), with the same codes.  The call is synchronous under the
 * mesh's mutex: a call that has returned was evaluated before any call that starts later, on either path.  max_items = 0 switches the path
 * off again.  May be called while callers are inside.
 * guber_wire_mesh_pool_direct_stats: direct_rpcs = RPCs served this way (they count in stats.rpcs / items / forwarded, in no set);
 * fallback_rpcs = those of them whose small call met a fall-back of either kind (guber_mesh_small_stats). */
typedef struct guber_wire_mesh_pool_direct_stats { uint64_t direct_rpcs, fallback_rpcs; } guber_wire_mesh_pool_direct_stats_t;
int    guber_wire_mesh_pool_set_direct(guber_wire_mesh_pool_t* p, uint32_t max_items /* 0 = off */, uint32_t max_calls /* 0 = 8 */);
int    guber_wire_mesh_pool_direct_stats(guber_wire_mesh_pool_t* p, guber_wire_mesh_pool_direct_stats_t* out);

#ifdef __cplusplus
}
#endif
#endif
