// gsx_ops.h — device functions shared by the kernels: the scorer's arithmetic
// (score.go), its tracer updates, and the canonical RNG.  Header-only so every
// kernel file inlines them.  gfx950 only.
#pragma once

#include "gsx_device.h"

namespace gsx {

// ---- score() pieces (score.go:258-381) --------------------------------------

// P6, ipColocationFactor (score.go:337-381) from the per-(observer, IP) count
// of present pairs (the size of ps.peerIPs[ip]).
__device__ __forceinline__ double ip_colocation(const DevState& s, const DevPeerParams& pp, uint64_t p) {
    const uint2 g = reinterpret_cast<const uint2*>(s.ipg)[p];
    double result = 0.0;
    const uint32_t gs[2] = {g.x, g.y};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint32_t id = gs[k];
        if (id == IPG_NONE || (id & IPG_WL)) continue;  // no IP / whitelisted (:346-367)
        const int64_t peers_in_ip = (int64_t)s.ipcount[id];
        if (peers_in_ip > pp.thr6) {
            const double surpluss = (double)(peers_in_ip - pp.thr6);
            result += surpluss * surpluss;
        }
    }
    return result;
}

// The per-pair tail of score(): topic cap, P5, P6, P7 (score.go:315-332).
// From p5 and p6 as given (p6 is not read when w6 == 0): the refresh pass passes
// the constant +0.0 for what the pair zero map says is zero, and every product
// is still executed.
// score_tail_parts is the same with every piece handed to `part` as it is
// formed (index: gsx_device.h SP_*; SP_TOPICS is the capped topic sum, a term
// that score() does not add is not handed over): gsx_score_parts reports the
// very values score() adds.  score_tail_vals is its instance that looks at none.
template <class F>
__device__ __forceinline__ double score_tail_parts(const DevPeerParams& pp, double score, double p5, double p6,
                                                   double bp, F&& part) {
    if (pp.topic_score_cap > 0 && score > pp.topic_score_cap) score = pp.topic_score_cap;
    part(SP_TOPICS, score);
    const double t5 = p5 * pp.w5;
    part(SP_P5, t5);
    score += t5;
    // With w6 == 0 the term is +-0 and score (never -0) is unchanged.
    if (pp.w6 != 0.0) {
        const double t6 = p6 * pp.w6;
        part(SP_P6, t6);
        score += t6;
    }
    if (bp > pp.thr7) {
        const double excess = bp - pp.thr7;
        const double p7 = excess * excess;
        const double t7 = p7 * pp.w7;
        part(SP_P7, t7);
        score += t7;
    }
    return score;
}
__device__ __forceinline__ double score_tail_vals(const DevPeerParams& pp, double score, double p5, double p6,
                                                  double bp) {
    return score_tail_parts(pp, score, p5, p6, bp, [](uint32_t, double) {});
}
__device__ __forceinline__ double score_tail(const DevState& s, const DevPeerParams& pp, uint64_t p, double score,
                                             double bp) {
    const double p5 = s.app[p];
    // With w6 == 0 the term is not added: skip the gather.
    const double p6 = pp.w6 != 0.0 ? ip_colocation(s, pp, p) : 0.0;
    return score_tail_vals(pp, score, p5, p6, bp);
}

// ---- P1's Duration division (score.go:280) ------------------------------------
// mesh_time / q1 as Go's int64 division (truncating), without the compiler's
// 64-bit software divide on the device.  The host stores inv = q1_inverse(q1)
// (gsx_device.h) beside q1 (DevTopicParams); inv == 0 (q1 < 0, which only a
// topic with TimeInMeshWeight == 0 can have) always takes the plain division.
//
// For q1 > 0 and |mt| < 2^50 (13 days in ns), with x = mt / q1 the real quotient
// and u = 2^-53:
//   (double)mt is exact; (double)q1 = q1 (1 + d1), inv = (1 + d2) / (double)q1,
//   est = mt * inv * (1 + d3), |d_i| <= u, so |est - x| <= |x| ((1 + u)^2 / (1 - u) - 1)
//   < |x| * 3.0001 u < 2^50 * 3.0001 * 2^-53 < 0.3751;
//   est + 1.5 * 2^52 rounds est to an integer n (|est| < 2^51, ties to even):
//   |n - est| <= 0.5, and n is the sum's low 52 mantissa bits less 2^51.
// So |n - x| < 0.8751 < 1: n is within 1 of trunc(x), and one exact integer
// remainder r = mt - n * q1 says which way: trunc(x) leaves a remainder of mt's
// sign with |r| < q1.  n * q1 does not overflow: n != 0 needs |x| > 0.1249, hence
// q1 < 2^53 and |n * q1| <= |mt| + 0.8751 * q1 < 2^54.
// Outside the bound the branch to the plain division is taken by the lanes that
// need it (a wave without such a lane skips it).  With inv == 0 every lane that
// divides takes it: such a topic runs at the software divide's speed, as it
// did before, and only for its in-mesh records (topic_score).
constexpr int64_t DIV_Q1_BOUND = 1ll << 50;

__host__ __device__ __forceinline__ int64_t div_q1(int64_t mt, int64_t q1, double inv) {
    // |mt| < 2^50 as one unsigned compare: mt + 2^50 in [1, 2^51)
    if (inv != 0.0 && (uint64_t)mt + (uint64_t)DIV_Q1_BOUND - 1u < 2u * (uint64_t)DIV_Q1_BOUND - 1u) {
        const double est = (double)mt * inv;
        const double sum = est + 6755399441055744.0;  // 1.5 * 2^52
#if defined(__HIP_DEVICE_COMPILE__)
        const uint64_t bits = (uint64_t)__double_as_longlong(sum);
#else
        uint64_t bits;
        __builtin_memcpy(&bits, &sum, sizeof bits);
#endif
        int64_t n = (int64_t)(bits & ((1ull << 52) - 1)) - (1ll << 51);
        const int64_t r = (int64_t)((uint64_t)mt - (uint64_t)n * (uint64_t)q1);
        const bool neg = mt < 0;
        const bool up = neg ? r > 0 : r >= q1;     // n is one below trunc(x)
        const bool down = neg ? r <= -q1 : r < 0;  // n is one above
        n += (int64_t)up - (int64_t)down;
        return n;
    }
    return mt / q1;
}

// One topic's contribution, score.go:276-311.  P1 and P3 are computed only for
// the records that have them (in the mesh; active and under the threshold), as
// the reference does: a record outside the mesh never reaches the division.
// topic_score_parts hands every weighted term to `part` as it is added (index:
// gsx_device.h SP_P1 .. SP_P4, before the topic weight; a term the record does
// not have is not handed over): gsx_score_parts reports the very products
// score() adds.  topic_score is its instance that looks at none.
template <class F>
__device__ __forceinline__ double topic_score_parts(const DevTopicParams& tp, uint8_t fl, int64_t mesh_time,
                                                    double fmd, double mmd, double mfp, double imd, F&& part) {
    double ts = 0.0;
    if (fl & REC_IN_MESH) {  // P1, integer Duration division (:280)
        double p1 = (double)div_q1(mesh_time, tp.q1, tp.inv_q1);
        if (p1 > tp.cap1) p1 = tp.cap1;
        const double t1 = p1 * tp.w1;
        part(SP_P1, t1);
        ts += t1;
    }
    const double p2 = fmd;  // P2
    const double t2 = p2 * tp.w2;
    part(SP_P2, t2);
    ts += t2;
    if (fl & REC_ACTIVE) {  // P3
        if (mmd < tp.thr3) {
            const double deficit = tp.thr3 - mmd;
            const double p3 = deficit * deficit;
            const double t3 = p3 * tp.w3;
            part(SP_P3, t3);
            ts += t3;
        }
    }
    const double p3b = mfp;  // P3b
    const double t3b = p3b * tp.w3b;
    part(SP_P3B, t3b);
    ts += t3b;
    const double p4 = (imd * imd);  // P4
    const double t4 = p4 * tp.w4;
    part(SP_P4, t4);
    ts += t4;
    return ts * tp.topic_weight;
}
__device__ __forceinline__ double topic_score(const DevTopicParams& tp, uint8_t fl, int64_t mesh_time, double fmd,
                                              double mmd, double mfp, double imd) {
    return topic_score_parts(tp, fl, mesh_time, fmd, mmd, mfp, imd, [](uint32_t, double) {});
}

// meshTime of a stored record: FRESH (grafted, not refreshed since) -> 0,
// else the value the last refresh computed (score.go:544-546).
__device__ __forceinline__ int64_t mesh_time_of(const DevState& s, uint8_t fl, uint64_t p, uint32_t t) {
    if (!(fl & REC_IN_MESH) || (fl & REC_FRESH)) return 0;
    const int64_t graft = reinterpret_cast<const int64_t*>(s.rec)[rec_index(p, t, s.n_topics, GRAFT)];
    return s.last_refresh - graft;
}
// The same from a graftTime loaded beforehand (with the record's other fields).
__device__ __forceinline__ int64_t mesh_time_from(const DevState& s, uint8_t fl, int64_t graft) {
    return (!(fl & REC_IN_MESH) || (fl & REC_FRESH)) ? 0 : s.last_refresh - graft;
}

// x *= decay; x = 0 if x < DecayToZero   (score.go:527-542, 553-556)
__device__ __forceinline__ double decay(double x, double d, double dtz) {
    x *= d;
    return x < dtz ? 0.0 : x;
}

// Every store to a record's MFP / IMD of a value that may be non-zero goes with
// this mark (the zero map's invariant, gsx_device.h).  A plain byte store of
// the constant: lanes racing on one tile's byte all write the same value.
__device__ __forceinline__ void zmap_mark(const DevState& s, uint64_t p, uint32_t t, int field) {
    s.zmap[zmap_index(p, t, s.n_topics, field)] = ZM_MAYBE;
}

// x is the same in every lane of the wave: says so to the compiler, which then
// keeps it (and what is loaded through it) in scalar registers.
__device__ __forceinline__ uint64_t wave_uniform(uint64_t x) {
    return (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)x) |
           (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(x >> 32)) << 32;
}

// The zero-map bytes of one (tile, topic) at the even byte offset o, MFP's in
// bits 0-7 and IMD's in bits 8-15, read through their aligned 32-bit word (a
// scalar load: the offset is wave-uniform).
constexpr uint32_t ZM_MFP_BITS = 0x00FFu, ZM_IMD_BITS = 0xFF00u;
__device__ __forceinline__ uint32_t zmap_pair(const uint8_t* zmap, uint64_t o) {
    const uint32_t w = reinterpret_cast<const uint32_t*>(zmap)[o >> 2];
    return __builtin_amdgcn_readfirstlane((w >> ((uint32_t)(o & 2) * 8)) & 0xFFFFu);
}

// The pair zero map's marks (gsx_device.h), as plain: one tile's entry, and
// PZ_P6 of every tile the pairs [lo, hi) of one observer's row overlap (an
// (observer, IP) group's pairs all lie in that row, in any of its tiles).
__device__ __forceinline__ void pzmap_mark(const DevState& s, uint64_t p, int which) {
    s.pzmap[(p / TILE) * PZ_ENTRY + which] = ZM_MAYBE;
}
__device__ __forceinline__ void pzmap_mark_row(const DevState& s, uint64_t lo, uint64_t hi) {
    if (hi > s.n_pairs) hi = s.n_pairs;
    if (lo >= hi) return;
    for (uint64_t tile = lo / TILE; tile <= (hi - 1) / TILE; ++tile) s.pzmap[tile * PZ_ENTRY + PZ_P6] = ZM_MAYBE;
}

// ---- deferred write-back of the decayed counters (REC_EPOCH, gsx_device.h) ----
// The refresh pass stores the decayed counters only every wb_period-th
// refresh; in between, a record's stored counters lag by rec_pend() decays.
// rec_decay(k) of the stored value is, bit for bit, what k refreshes with a
// store after each would have left.  Outside the refresh pass
// every access to a counter goes through rec_read (a reader) or
// rec_materialize (before any read-modify-write).
struct RecVals {
    double fmd, mmd, mfp, imd;
};

// decays the stored counters of record (pair flags st, record flags fl) lag by
__device__ __forceinline__ uint32_t rec_pend(const DevState& s, uint8_t st, uint8_t fl, const DevTopicParams& tp) {
    return ((st & PAIR_CONNECTED) && tp.scored) ? ((s.phase - ((uint32_t)fl >> REC_EPOCH_SHIFT)) & EPOCH_MASK) : 0u;
}

// ---- the decay chain ------------------------------------------------------------
// k pending decays as k multiplies and ONE zero test: for 0 < d < 1 and
// 0 < dtz, x = fl(x * d) taken k >= 1 times and then x < dtz ? 0 : x gives, bit
// for bit, what decay() applied k times gives.  Both forms run the same
// multiplies on the same values until the stepwise one zeroes x, so they can
// differ only in when that happens:
//   - x >= 0: x * d <= x exactly, and x is representable, so the rounded
//     product is <= x too (subnormals included).  A value under dtz after
//     step j is therefore still under it after step k: the last test zeroes
//     what an earlier one would have, and +0.0 decays to +0.0 in between.  A
//     value never under dtz on the way is not under it at the end, by the
//     same monotony, and neither form touches it.
//   - x < 0 (or -0.0): every product stays <= -0.0 < dtz: the first test and
//     the last alike give +0.0.
//   - NaN and +inf fail every test and pass through the same multiplies; -inf
//     is zeroed like any negative value.
// k == 0 runs no test: a stored value under dtz that no decay has touched
// stands (an import may hold one).
// The preconditions are the host's parameter validation
// (gsx_validate_peer_params: 0 < DecayToZero < 1; gsx_validate_topic_params
// and the peer parameters: 0 < decay < 1), but a decay is validated only where
// its weight is not zero, and an engine without peer parameters has
// DecayToZero == 0.  With d > 1 a value can climb back over dtz, with d < 0 it
// changes sign, with dtz <= 0 a -0.0 survives the one test: where
// DevTopicParams::chain (all four decays of the topic), decay_chain_ok(d7) or
// dtz > 0 does not hold, the pending decays keep the stepwise form.
__device__ __forceinline__ double decay_chain(double x, double d, double dtz, uint32_t k) {
    for (uint32_t i = 0; i < k; ++i) x *= d;
    return (k && x < dtz) ? 0.0 : x;
}

__device__ __forceinline__ void rec_decay(RecVals& v, const DevTopicParams& tp, double dtz, uint32_t k) {
    if (tp.chain && dtz > 0.0) {
        for (uint32_t i = 0; i < k; ++i) {
            v.fmd *= tp.d2;
            v.mmd *= tp.d3;
            v.mfp *= tp.d3b;
            v.imd *= tp.d4;
        }
        if (k) {
            v.fmd = v.fmd < dtz ? 0.0 : v.fmd;
            v.mmd = v.mmd < dtz ? 0.0 : v.mmd;
            v.mfp = v.mfp < dtz ? 0.0 : v.mfp;
            v.imd = v.imd < dtz ? 0.0 : v.imd;
        }
        return;
    }
    for (uint32_t i = 0; i < k; ++i) {  // a decay outside (0, 1): test after every multiply
        v.fmd = decay(v.fmd, tp.d2, dtz);
        v.mmd = decay(v.mmd, tp.d3, dtz);
        v.mfp = decay(v.mfp, tp.d3b, dtz);
        v.imd = decay(v.imd, tp.d4, dtz);
    }
}

// The record's counters as of the last refresh; stores nothing.
__device__ __forceinline__ RecVals rec_read(const DevState& s, uint64_t p, uint32_t t, uint8_t st, uint8_t fl) {
    const size_t b = rec_index(p, t, s.n_topics, FMD);
    RecVals v = {s.rec[b + FMD * TILE], s.rec[b + MMD * TILE], s.rec[b + MFP * TILE], s.rec[b + IMD * TILE]};
    rec_decay(v, s.tp[t], s.decay_to_zero, rec_pend(s, st, fl, s.tp[t]));
    return v;
}
__device__ __forceinline__ RecVals rec_read(const DevState& s, uint64_t p, uint32_t t) {
    return rec_read(s, p, t, s.pflags[p], s.rflags[flag_index(p, t, s.n_topics)]);
}

// k decays applied to the stored counters of a record, the changed ones stored.
__device__ __forceinline__ void rec_store_decayed(const DevState& s, uint64_t p, uint32_t t, uint32_t k) {
    const size_t b = rec_index(p, t, s.n_topics, FMD);
    const RecVals o = {s.rec[b + FMD * TILE], s.rec[b + MMD * TILE], s.rec[b + MFP * TILE], s.rec[b + IMD * TILE]};
    RecVals v = o;
    rec_decay(v, s.tp[t], s.decay_to_zero, k);
    if (__double_as_longlong(v.fmd) != __double_as_longlong(o.fmd)) s.rec[b + FMD * TILE] = v.fmd;
    if (__double_as_longlong(v.mmd) != __double_as_longlong(o.mmd)) s.rec[b + MMD * TILE] = v.mmd;
    if (__double_as_longlong(v.mfp) != __double_as_longlong(o.mfp)) {
        if (__double_as_longlong(v.mfp) != 0) zmap_mark(s, p, t, MFP);
        s.rec[b + MFP * TILE] = v.mfp;
    }
    if (__double_as_longlong(v.imd) != __double_as_longlong(o.imd)) {
        if (__double_as_longlong(v.imd) != 0) zmap_mark(s, p, t, IMD);
        s.rec[b + IMD * TILE] = v.imd;
    }
}

// Brings the stored record up to date: applies its pending decays to all four
// counters, stores the ones that changed and sets its epoch to the current
// phase (the epoch is per record, hence the whole record).  -> the flag byte
// as stored.  st: the pair's flags as the decays were skipped under (a pair
// being disconnected passes its old, connected flags).
__device__ __forceinline__ uint8_t rec_materialize(const DevState& s, uint64_t p, uint32_t t, uint8_t st) {
    const size_t fi = flag_index(p, t, s.n_topics);
    const uint8_t fl = s.rflags[fi];
    const uint32_t k = rec_pend(s, st, fl, s.tp[t]);
    if (k) rec_store_decayed(s, p, t, k);
    const uint8_t nf = (uint8_t)((fl & ~REC_EPOCH) | ((s.phase & EPOCH_MASK) << REC_EPOCH_SHIFT));
    if (nf != fl) s.rflags[fi] = nf;
    return nf;
}
__device__ __forceinline__ uint8_t rec_materialize(const DevState& s, uint64_t p, uint32_t t) {
    return rec_materialize(s, p, t, s.pflags[p]);
}

// ---- the behaviour penalty under the same write-back (PAIR_EPOCH, gsx_device.h) ----
// decays of d7 the stored bp of a pair with flags st lags by
__device__ __forceinline__ uint32_t bp_pend(const DevState& s, uint8_t st) {
    return (st & PAIR_CONNECTED) ? ((s.phase - ((uint32_t)st >> PAIR_EPOCH_SHIFT)) & EPOCH_MASK) : 0u;
}

// (the decay chain above; BehaviourPenaltyDecay is validated only with a
// non-zero BehaviourPenaltyWeight, so any other value keeps the stepwise form)
__device__ __forceinline__ double bp_decay(double bp, double d7, double dtz, uint32_t k) {
    if (decay_chain_ok(d7) && dtz > 0.0) return decay_chain(bp, d7, dtz, k);
    for (uint32_t i = 0; i < k; ++i) bp = decay(bp, d7, dtz);
    return bp;
}

// The pair's behaviour penalty as of the last refresh; stores nothing.
__device__ __forceinline__ double bp_read(const DevState& s, uint64_t p, uint8_t st) {
    return bp_decay(s.bp[p], s.d7, s.decay_to_zero, bp_pend(s, st));
}

// Brings the stored bp of a connected pair up to date and its epoch to the
// current phase (before any read-modify-write of bp, and before the pair stops
// being decayed).  -> the flag byte as stored.
__device__ __forceinline__ uint8_t bp_materialize(const DevState& s, uint64_t p, uint8_t st) {
    if (!(st & PAIR_CONNECTED)) return st;
    const uint32_t k = bp_pend(s, st);
    if (k) {
        const double o = s.bp[p], v = bp_decay(o, s.d7, s.decay_to_zero, k);
        if (__double_as_longlong(v) != __double_as_longlong(o)) s.bp[p] = v;
    }
    const uint8_t nf = (uint8_t)((st & ~PAIR_EPOCH) | ((s.phase & EPOCH_MASK) << PAIR_EPOCH_SHIFT));
    if (nf != st) s.pflags[p] = nf;
    return nf;
}

// score(p) from the stored state, no refresh (RemovePeer, score.go:615).
__device__ __forceinline__ double eval_pair(const DevState& s, const DevPeerParams& pp, uint64_t p) {
    const uint8_t st = s.pflags[p];
    if (!(st & PAIR_PRESENT)) return 0.0;
    double score = 0.0;
    for (uint32_t t = 0; t < s.n_topics; ++t) {
        const DevTopicParams& tp = s.tp[t];
        if (!tp.scored) continue;
        const uint8_t fl = s.rflags[flag_index(p, t, s.n_topics)];
        const RecVals v = rec_read(s, p, t, st, fl);
        score += topic_score(tp, fl, mesh_time_of(s, fl, p, t), v.fmd, v.mmd, v.mfp, v.imd);
    }
    return score_tail(s, pp, p, score, bp_read(s, p, st));
}

// k steps of "x = x + 1; if x > cap { x = cap }" (score.go:925-938, 970-973),
// bit for bit, in O(log k): x only ever grows until it is capped, and it
// stays capped, so the result is min(cap, k sequential +1s); within one
// binade [2^e, 2^(e+1)) with 0 <= e <= 52 adding an integer is exact, so only
// the step that crosses into the next binade rounds.  Below 1 (and in the
// never-reached range >= 2^52) the steps are taken one by one.
__device__ __forceinline__ double add_ones_capped(double x, uint32_t k, double cap) {
    while (k && !(x >= 1.0 && x < 4503599627370496.0)) {  // [1, 2^52)
        x = x + 1;
        --k;
        if (x > cap) return cap;
    }
    while (k) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
        const double top = __longlong_as_double((long long)((((bits >> 52) & 0x7FF) + 1) << 52));  // 2^(e+1)
        const double gap = top - x;  // exact (Sterbenz)
        const double s = ceil(gap) - 1;  // steps that stay below top
        if (s >= (double)k) {
            x = x + (double)k;
            k = 0;
        } else {
            x = x + s;
            k -= (uint32_t)s;
            x = x + 1;  // the crossing step rounds
            --k;
        }
        if (x > cap) return cap;
        if (!(x < 4503599627370496.0))
            while (k) {
                x = x + 1;
                --k;
                if (x > cap) return cap;
            }
    }
    return x > cap ? cap : x;
}

// ---- tracer updates (score.go:588-974) -----------------------------------------

__device__ __forceinline__ void ipcount_add(const DevState& s, uint64_t p, int delta) {
    const uint2 g = reinterpret_cast<const uint2*>(s.ipg)[p];
    if (g.x != IPG_NONE) s.ipcount[g.x & ~IPG_WL] += (uint32_t)delta;
    if (g.y != IPG_NONE && g.y != g.x) s.ipcount[g.y & ~IPG_WL] += (uint32_t)delta;
}

__device__ __forceinline__ bool scored_topic(const DevState& s, uint64_t p, uint32_t topic) {
    return (s.pflags[p] & PAIR_PRESENT) && topic < s.n_topics && s.tp[topic].scored;
}

// [row_lo, row_hi): the pairs of p's observer (the host's row bounds).
__device__ inline void ev_add_peer(const DevState& s, const DevPeerParams& pp, uint64_t p, uint64_t row_lo,
                                   uint64_t row_hi) {  // AddPeer :588-602
    const uint8_t st = s.pflags[p];
    const uint8_t ep = (uint8_t)((s.phase & EPOCH_MASK) << REC_EPOCH_SHIFT);  // the records are current as of this phase
    if (!(st & PAIR_PRESENT)) {  // new peerStats{topics: {}}
        for (uint32_t t = 0; t < s.n_topics; ++t) {
            const size_t b = rec_index(p, t, s.n_topics, FMD);
            for (int f = 0; f < NFIELD; ++f) s.rec[b + f * TILE] = 0.0;
            s.rflags[flag_index(p, t, s.n_topics)] = ep;
        }
        s.bp[p] = 0.0;
        s.expire[p] = 0;
        ipcount_add(s, p, +1);  // setIPs
        // A group that is now above the threshold gives every pair carrying it a
        // P6, this one included: PZ_P6 of the whole row.  At or below it nothing
        // changes (ordinary churn leaves the map alone); a whitelisted group
        // never counts.
        const uint2 g = reinterpret_cast<const uint2*>(s.ipg)[p];
        const bool over_x = g.x != IPG_NONE && !(g.x & IPG_WL) && (int64_t)s.ipcount[g.x] > pp.thr6;
        const bool over_y = g.y != IPG_NONE && !(g.y & IPG_WL) && (int64_t)s.ipcount[g.y] > pp.thr6;
        if (over_x || over_y) {
            pzmap_mark(s, p, PZ_P6);
            pzmap_mark_row(s, row_lo, row_hi);
        }
    } else if (!(st & PAIR_CONNECTED)) {  // a retained pair reconnects: it was not decayed meanwhile
        for (uint32_t t = 0; t < s.n_topics; ++t) {
            const size_t fi = flag_index(p, t, s.n_topics);
            const uint8_t fl = s.rflags[fi];
            if ((fl & REC_EPOCH) != ep) s.rflags[fi] = (uint8_t)((fl & ~REC_EPOCH) | ep);
        }
    }
    // a new or reconnecting pair's bp is current as of this phase; a connected
    // pair keeps its epoch
    if (!(st & PAIR_PRESENT) || !(st & PAIR_CONNECTED))
        s.pflags[p] = (uint8_t)(PAIR_PRESENT | PAIR_CONNECTED | ((s.phase & EPOCH_MASK) << PAIR_EPOCH_SHIFT));
}

__device__ inline void ev_remove_peer(const DevState& s, const DevPeerParams& pp, uint64_t p, int64_t now) {  // :604-637
    const uint8_t st = s.pflags[p];
    if (!(st & PAIR_PRESENT)) return;
    if (eval_pair(s, pp, p) > 0) {  // positive score: forget the peer
        ipcount_add(s, p, -1);
        bp_materialize(s, p, st);  // (an absent pair's bp is exported as stored)
        s.pflags[p] = 0;
        return;
    }
    // a retained pair is not decayed (and its epochs are not read) until it
    // reconnects: every record is brought up to date now
    for (uint32_t t = 0; t < s.n_topics; ++t) {
        const DevTopicParams& tp = s.tp[t];
        if (!tp.scored) continue;
        const size_t b = rec_index(p, t, s.n_topics, FMD);
        const size_t fi = flag_index(p, t, s.n_topics);
        const uint8_t fl = rec_materialize(s, p, t, st);
        s.rec[b + FMD * TILE] = 0.0;
        const double threshold = tp.thr3;
        const double mmd = s.rec[b + MMD * TILE];
        if ((fl & REC_IN_MESH) && (fl & REC_ACTIVE) && mmd < threshold) {
            const double deficit = threshold - mmd;
            zmap_mark(s, p, t, MFP);
            s.rec[b + MFP * TILE] = s.rec[b + MFP * TILE] + deficit * deficit;
        }
        s.rflags[fi] = fl & ~(REC_IN_MESH | REC_FRESH);
    }
    bp_materialize(s, p, st);  // (and bp, before the pair stops being decayed)
    s.pflags[p] = PAIR_PRESENT;
    s.expire[p] = now + pp.retain_ns;
}

__device__ inline void ev_graft(const DevState& s, uint64_t p, uint32_t topic, int64_t now) {  // :642-660
    if (!scored_topic(s, p, topic)) return;
    reinterpret_cast<int64_t*>(s.rec)[rec_index(p, topic, s.n_topics, GRAFT)] = now;
    const size_t fi = flag_index(p, topic, s.n_topics);  // meshTime = 0, not active; the counters' epoch stays
    s.rflags[fi] = (uint8_t)((s.rflags[fi] & REC_EPOCH) | REC_IN_MESH | REC_FRESH);
}

__device__ inline void ev_prune(const DevState& s, uint64_t p, uint32_t topic) {  // :662-684
    if (!scored_topic(s, p, topic)) return;
    const size_t b = rec_index(p, topic, s.n_topics, FMD);
    const size_t fi = flag_index(p, topic, s.n_topics);
    const uint8_t fl = rec_materialize(s, p, topic);
    const double threshold = s.tp[topic].thr3;
    const double mmd = s.rec[b + MMD * TILE];
    if ((fl & REC_ACTIVE) && mmd < threshold) {
        const double deficit = threshold - mmd;
        zmap_mark(s, p, topic, MFP);
        s.rec[b + MFP * TILE] = s.rec[b + MFP * TILE] + deficit * deficit;
    }
    s.rflags[fi] = fl & ~(REC_IN_MESH | REC_FRESH);
}

__device__ inline void ev_first(const DevState& s, uint64_t p, uint32_t topic) {  // :912-939
    if (!scored_topic(s, p, topic)) return;
    const DevTopicParams& tp = s.tp[topic];
    const size_t b = rec_index(p, topic, s.n_topics, FMD);
    const uint8_t fl = rec_materialize(s, p, topic);
    double f = s.rec[b + FMD * TILE] + 1;
    if (f > tp.cap2) f = tp.cap2;
    s.rec[b + FMD * TILE] = f;
    if (!(fl & REC_IN_MESH)) return;
    double m = s.rec[b + MMD * TILE] + 1;
    if (m > tp.cap3) m = tp.cap3;
    s.rec[b + MMD * TILE] = m;
}

__device__ inline void ev_mesh(const DevState& s, uint64_t p, uint32_t topic) {  // :944-974 (window checked by caller)
    if (!scored_topic(s, p, topic)) return;
    if (!(s.rflags[flag_index(p, topic, s.n_topics)] & REC_IN_MESH)) return;
    rec_materialize(s, p, topic);
    const size_t b = rec_index(p, topic, s.n_topics, MMD);
    double m = s.rec[b] + 1;
    if (m > s.tp[topic].cap3) m = s.tp[topic].cap3;
    s.rec[b] = m;
}

__device__ inline void ev_invalid(const DevState& s, uint64_t p, uint32_t topic) {  // :894-907
    if (!scored_topic(s, p, topic)) return;
    const size_t b = rec_index(p, topic, s.n_topics, IMD);
    rec_materialize(s, p, topic);
    zmap_mark(s, p, topic, IMD);
    s.rec[b] = s.rec[b] + 1;
}

__device__ inline void ev_penalty(const DevState& s, uint64_t p, int64_t count) {  // AddPenalty :384-398
    const uint8_t st = s.pflags[p];
    if (!(st & PAIR_PRESENT)) return;
    bp_materialize(s, p, st);
    s.bp[p] = s.bp[p] + (double)count;
}

// ---- counters --------------------------------------------------------------------
// Sums NV per-thread counters over a 256-thread block (wave shuffles, then
// LDS across the four waves) and adds each non-zero total to its global
// counter with ONE atomic per block.  Same-address atomics serialise at the
// memory side, so kernels that own counters run grid-stride over a bounded
// grid (COUNTER_GRID blocks) and reach this once per block, every thread.
constexpr unsigned COUNTER_GRID = 2048;

template <int NV>
__device__ __forceinline__ void block_count(unsigned long long (&v)[NV], unsigned long long* stats,
                                            const uint32_t (&slot)[NV]) {
    __shared__ unsigned long long part[NV][4];
#pragma unroll
    for (int i = 0; i < NV; ++i)
        for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_down(v[i], off, 64);
    const unsigned wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) part[i][wave] = v[i];
    __syncthreads();
    if (threadIdx.x < NV) {
        const unsigned i = threadIdx.x;
        const unsigned long long t = part[i][0] + part[i][1] + part[i][2] + part[i][3];
        if (t) atomicAdd(&stats[slot[i]], t);
    }
}

// Appends to a shared list with ONE atomic per wave: the active lanes with
// `take` get consecutive slots in lane order (-> the lane's slot; callable in
// divergent code: the ballot and the broadcast see the active lanes only).  A
// per-lane atomicAdd on one counter serialises every append of the grid at
// one L2 channel.
__device__ __forceinline__ uint32_t wave_append(uint32_t* ctr, bool take) {
    const uint64_t b = __ballot(take);
    if (b == 0) return 0;
    const uint32_t lane = __lane_id();
    const int leader = __ffsll((long long)b) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(ctr, (uint32_t)__popcll(b));
    base = (uint32_t)__shfl((int)base, leader, 64);
    return base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
}

// ---- canonical RNG ---------------------------------------------
__host__ __device__ __forceinline__ uint64_t smix(uint64_t z) {  // SplitMix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t h4(uint64_t seed, uint64_t tag, uint64_t a, uint64_t b) {
    return smix(seed + 0x9E3779B97F4A7C15ull * (1ull + smix(tag ^ smix(a ^ smix(b)))));
}
// math/rand's Int31n over Int31 draws h(seed, tag, vertex, base | k), standing
// in for the router's global rand source (gossipsub.go:1890-1895).
struct Rng {
    uint64_t seed, tag, vertex, base;
    uint32_t k;
    __host__ __device__ int32_t int31() { return (int32_t)(h4(seed, tag, vertex, base | k++) >> 33); }
    __host__ __device__ int32_t int31n(int32_t n) {
        if ((n & (n - 1)) == 0) return int31() & (n - 1);
        const int32_t max = (int32_t)((1u << 31) - 1 - (1u << 31) % (uint32_t)n);
        int32_t v = int31();
        while (v > max) v = int31();
        return v % n;
    }
    // shufflePeers: for i, j = Intn(i+1), swap
    template <typename T>
    __device__ void shuffle(T* a, int n) {
        for (int i = 0; i < n; ++i) {
            const int j = int31n(i + 1);
            const T x = a[i];
            a[i] = a[j];
            a[j] = x;
        }
    }
};

}  // namespace gsx
