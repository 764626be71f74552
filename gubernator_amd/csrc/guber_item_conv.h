// guber_item_conv.h — guber_item_t (include/guber_gpu.h: CacheItem + its Value) <-> the bucket record guber::Rec.  One spelling for the
// engine (engine_items.inl, engine_host.inl) and for the kernel source on the CPU (tests/hostsim/devsim.cpp).
#pragma once
#include <string.h>

#include "../../include/guber_gpu.h"
#include "guber_algo.h"

static inline guber::Rec rec_from_item(const guber_item_t& in) {
    using namespace guber;
    Rec s; rec_clear(s);
    s.limit = in.limit; s.duration = in.duration; s.stamp = in.stamp; s.burst = in.burst;
    s.expire_at = in.expire_at; s.invalid_at = in.invalid_at;
    if (in.algorithm == GUBER_ALGO_TOKEN_BUCKET) { s.remaining = in.remaining; s.burst = 0; s.meta = make_meta(K_TOKEN, in.status, ALGO_TOKEN); }
    else if (in.algorithm == GUBER_ALGO_LEAKY_BUCKET) { s.remaining = f2bits(in.remaining_f); s.meta = make_meta(K_LEAKY, 0, ALGO_LEAKY); }
    else s.meta = make_meta(K_NIL, 0, in.algorithm);   // gubernator.go:435-455: no Value for other algorithms
    return s;
}
static inline void item_from_rec(const guber::Rec& s, guber_item_t* out) {
    using namespace guber;
    memset(out, 0, sizeof(*out));
    out->limit = s.limit; out->duration = s.duration; out->stamp = s.stamp; out->burst = s.burst;
    out->expire_at = s.expire_at; out->invalid_at = s.invalid_at;
    if (rec_kind(s) == K_TOKEN) { out->algorithm = GUBER_ALGO_TOKEN_BUCKET; out->status = (uint8_t)rec_status(s); out->remaining = s.remaining; out->burst = 0; }
    else if (rec_kind(s) == K_LEAKY) { out->algorithm = GUBER_ALGO_LEAKY_BUCKET; out->remaining_f = bits2f(s.remaining); }
    else {   // CacheItem without a Value: only the CacheItem fields exist
        out->algorithm = (uint8_t)rec_algo(s);
        out->limit = out->duration = out->stamp = out->burst = 0;
    }
}
