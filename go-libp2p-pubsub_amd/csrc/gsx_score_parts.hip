// gsx_score_parts.hip — what each score is made of (gsx_score_parts), reduced
// on the device: per pair the weighted P1 .. P7 that score() (score.go:258-335)
// adds up, the capped topic sum and the score; the part that is lowest and
// negative (the pair's cause), the topic whose weighted score is (its worst
// topic); and the selected pairs counted per (score bin, cause), per (score
// bin, worst topic), per (observer row, cause) and per (peer, cause), without
// a record leaving HBM.
//
// One streaming pass over the tiled records, shaped like k_refresh_score's
// score-only path: lane l of a wave owns pair 64 w + l, every field load is the
// tile's contiguous 512-B line, the zero maps (gsx_device.h) are read first and
// a counter whose entry says zero is the constant +0.0 without a load, topic
// parameters come from the kernel-argument segment up to KARG_TOPICS topics.
// The pending decays of the deferred write-back are applied in registers
// (rec_pend / rec_decay, bp_read); nothing is stored to the engine's state.
// The arithmetic is gsx_ops.h's: topic_score and score_tail_vals are
// topic_score_parts and score_tail_parts with nobody looking, so SCORE is bit
// for bit the score the refresh pass stores, and the parts are the very
// products it added.
//
// A wave per 64-pair tile, grid-stride over a bounded grid, because of how the
// pass accumulates (all integer adds: bit-identical from run to run, whatever
// the grid):
//   * cause_hist / topic_hist: a per-block LDS table (ds_add, no return), then
//     ONE no-return global atomic per block and non-zero counter;
//   * obs_cause: k_score_stats's segmented runs.  A row's pairs are contiguous,
//     so the lanes of a wave that share pair_obs form a run; per cause one
//     ballot masked to the run, popcount taken by the run's first lane.  A run
//     that neither began in the wave before nor goes on in the wave after is
//     the whole row: a plain store (the output starts zeroed); only rows cut by
//     a wave's edge add with an atomic, at most two runs per wave, so a hub row
//     of thousands of pairs costs one atomic per cause and wave;
//   * peer_cause: the targets col[p] are scattered: one no-return u32 atomic
//     per selected pair.
#include "gsx_ops.h"

#include <algorithm>

namespace gsx {

namespace {

constexpr uint32_t SP_THREADS = 256, SP_WAVES = SP_THREADS / 64;
constexpr uint32_t SP_LC = SS_MAX_BINS * SP_CAUSES, SP_LT = SS_MAX_BINS * (SP_MAX_TOPICS + 1);

template <int TT>
__global__ __launch_bounds__(SP_THREADS) void k_score_parts(DevState s, KernParams kp, ScorePartsArgs a) {
    __shared__ uint32_t lc[SP_LC];  // [bin][cause]
    __shared__ uint32_t lt[SP_LT];  // [bin][topic | none]
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int T = TT > 0 ? TT : (int)s.n_topics;
    const uint32_t nb = a.n_edges + 1, ntc = (uint32_t)T + 1;
    const DevPeerParams& pp = kp.pp;
    const bool obs_view = a.obs_cause != nullptr;
    for (uint32_t i = threadIdx.x; i < SP_LC; i += SP_THREADS) lc[i] = 0;
    for (uint32_t i = threadIdx.x; i < SP_LT; i += SP_THREADS) lt[i] = 0;
    __syncthreads();

    // (base is wave-uniform: a wave's lanes stay in the loop together)
    for (uint64_t base = ((uint64_t)blockIdx.x * SP_WAVES + wave) * 64; base < s.n_pairs;
         base += (uint64_t)gridDim.x * SP_THREADS) {
        const uint64_t p = base + lane;
        const bool valid = p < s.n_pairs;
        const uint64_t wtile = wave_uniform(base / TILE);
        const uint64_t zoff = wtile * (uint64_t)T * 2;
        // the wave's zero-map entries, before the record loads (k_refresh_score)
        uint32_t zm[TT > 0 ? TT : 1];
        if constexpr (TT > 0) {
#pragma unroll
            for (int t = 0; t < TT; ++t) zm[t] = zmap_pair(s.zmap, zoff + 2 * t);
        }
        const uint32_t pz = __builtin_amdgcn_readfirstlane(reinterpret_cast<const uint32_t*>(s.pzmap)[wtile]);
        const bool app_maybe = (pz >> (8 * PZ_APP)) & 0xFFu;
        const uint8_t st = valid ? s.pflags[p] : (uint8_t)0;
        const bool present = (st & PAIR_PRESENT) != 0;

        // an absent pair has no peerStats: every part +0.0, no cause, no topic
        double part[SP_PARTS];
#pragma unroll
        for (uint32_t j = 0; j < SP_PARTS; ++j) part[j] = 0.0;
        uint32_t cause = SP_CAUSE_NONE, worst = SP_TOPIC_NONE;
        const uint8_t* const ftile = s.rflags + wtile * (uint64_t)T * TILE + lane;
        if (present) {
            const double* const tile = s.rec + wtile * (uint64_t)T * (NFIELD * TILE) + lane;
            double p5 = 0.0;
            if (app_maybe) p5 = s.app[p];  // early, with the record loads
            double score = 0.0, low = 0.0;
            // One topic's terms from its loaded record: the pending decays, the
            // products topic_score adds, each into its part, and their sum.
            auto topic_step = [&](int t, const DevTopicParams& tp, double fmd, double mmd, double mfp, double imd,
                                  int64_t graft, uint8_t fl) {
                RecVals v = {fmd, mmd, mfp, imd};
                rec_decay(v, tp, s.decay_to_zero, rec_pend(s, st, fl, tp));
                const double ts = topic_score_parts(tp, fl, mesh_time_from(s, fl, graft), v.fmd, v.mmd, v.mfp, v.imd,
                                                    [&](uint32_t j, double x) { part[j] += x * tp.topic_weight; });
                score += ts;
                if (ts < low) {  // the lowest t among the lowest negative: a NaN is below nothing
                    low = ts;
                    worst = (uint32_t)t;
                }
            };
            if constexpr (TT > 0) {
                // every scored topic's record in flight before any is used
                double fmd[TT], mmd[TT], mfp[TT], imd[TT];
                int64_t gr[TT];
                uint8_t fl[TT];
#pragma unroll
                for (int t = 0; t < TT; ++t) {
                    if (!kp.tp[t].scored) continue;
                    const double* const r = tile + (uint64_t)t * (NFIELD * TILE);
                    fmd[t] = __builtin_nontemporal_load(r + FMD * TILE);
                    mmd[t] = __builtin_nontemporal_load(r + MMD * TILE);
                    mfp[t] = (zm[t] & ZM_MFP_BITS) ? __builtin_nontemporal_load(r + MFP * TILE) : 0.0;
                    imd[t] = (zm[t] & ZM_IMD_BITS) ? __builtin_nontemporal_load(r + IMD * TILE) : 0.0;
                    fl[t] = ftile[t * TILE];
                    gr[t] = (TT > 1 || (fl[t] & REC_IN_MESH))
                                ? __builtin_nontemporal_load(reinterpret_cast<const int64_t*>(r) + GRAFT * TILE)
                                : 0;
                }
#pragma unroll
                for (int t = 0; t < TT; ++t) {
                    if (!kp.tp[t].scored) continue;
                    topic_step(t, kp.tp[t], fmd[t], mmd[t], mfp[t], imd[t], gr[t], fl[t]);
                }
            } else {
                for (int t = 0; t < T; ++t) {
                    const DevTopicParams& tp = s.tp[t];
                    if (!tp.scored) continue;
                    const double* const r = tile + (uint64_t)t * (NFIELD * TILE);
                    const uint32_t zmt = zmap_pair(s.zmap, zoff + 2 * t);
                    const uint8_t fl = ftile[t * TILE];
                    const int64_t graft = (fl & REC_IN_MESH) ? reinterpret_cast<const int64_t*>(r)[GRAFT * TILE] : 0;
                    const double fmd = __builtin_nontemporal_load(r + FMD * TILE),
                                 mmd = __builtin_nontemporal_load(r + MMD * TILE);
                    const double mfp = (zmt & ZM_MFP_BITS) ? __builtin_nontemporal_load(r + MFP * TILE) : 0.0;
                    const double imd = (zmt & ZM_IMD_BITS) ? __builtin_nontemporal_load(r + IMD * TILE) : 0.0;
                    topic_step(t, tp, fmd, mmd, mfp, imd, graft, fl);
                }
            }
            // the tail as the score-only pass forms it: P6 gathered whenever it is weighted
            const double bp = bp_read(s, p, st);
            const double p6 = pp.w6 != 0.0 ? ip_colocation(s, pp, p) : 0.0;
            part[SP_SCORE] = score_tail_parts(pp, score, p5, p6, bp, [&](uint32_t j, double x) { part[j] = x; });
            double lowest = 0.0;
#pragma unroll
            for (uint32_t j = 0; j < SP_CAUSE_NONE; ++j)
                if (part[j] < lowest) {  // the lowest j among the lowest negative parts; never a NaN
                    lowest = part[j];
                    cause = j;
                }
        }

        if (valid) {
            if (a.pair_parts) {
                double* const o = a.pair_parts + p * SP_PARTS;
#pragma unroll
                for (uint32_t j = 0; j < SP_PARTS; ++j) o[j] = part[j];
            }
            if (a.pair_cause) a.pair_cause[p] = (uint8_t)cause;
            if (a.pair_topic) a.pair_topic[p] = (uint8_t)worst;
        }

        bool sel = a.select == SS_PRESENT ? present : present && (st & PAIR_CONNECTED);
        if (sel && a.select == SS_MESH) sel = (ftile[a.topic * TILE] & REC_IN_MESH) != 0;
        uint32_t bin = 0;
        if (sel) {
            const double sc = part[SP_SCORE];  // gsx_score_stats's bin: a NaN is below no edge
#pragma unroll
            for (uint32_t k = 0; k < SS_MAX_EDGES; ++k) bin += (k < a.n_edges && !(sc < a.edges[k])) ? 1u : 0u;
            if (a.cause_hist) atomicAdd(&lc[bin * SP_CAUSES + cause], 1u);
            if (a.topic_hist) atomicAdd(&lt[bin * ntc + (worst == SP_TOPIC_NONE ? (uint32_t)T : worst)], 1u);
            if (a.peer_cause) atomicAdd(a.peer_cause + (size_t)(uint32_t)a.col[p] * SP_CAUSES + cause, 1u);
        }

        if (obs_view) {  // the run of lanes that share this lane's observer (k_score_stats)
            uint32_t obs = 0xFFFFFFFFu;
            if (valid) obs = a.pair_obs[p];
            const uint32_t prev = (uint32_t)__shfl_up((int)obs, 1, 64);
            bool head = lane == 0 || prev != obs;
            const uint64_t heads = __ballot(head);
            const uint64_t above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
            const uint32_t next = above ? (uint32_t)__builtin_ctzll(above) : 64u;
            const uint64_t run = (next == 64 ? ~0ull : (1ull << next) - 1) & (~0ull << lane);
            // the row goes on beyond this wave's pairs: its other segments add to the same counters
            const bool lo = lane == 0 && valid && p > 0 && a.pair_obs[p - 1] == obs;
            const bool hi = lane == 63 && p + 1 < s.n_pairs && a.pair_obs[p + 1] == obs;
            const uint64_t cl = __ballot(lo), ch = __ballot(hi);
            const bool shared = (lane == 0 && cl != 0) || (next == 64 && ch != 0);
            head = head && valid;
#pragma unroll
            for (uint32_t k = 0; k < SP_CAUSES; ++k) {
                const uint64_t b = __ballot(sel && cause == k);
                if (head) {
                    const uint32_t c = (uint32_t)__popcll(b & run);
                    if (c) {
                        uint32_t* dst = a.obs_cause + (size_t)obs * SP_CAUSES + k;
                        if (shared) atomicAdd(dst, c);
                        else *dst = c;
                    }
                }
            }
        }
    }

    __syncthreads();
    if (a.cause_hist)
        for (uint32_t i = threadIdx.x; i < nb * SP_CAUSES; i += SP_THREADS)
            if (const uint32_t c = lc[i]) atomicAdd(a.cause_hist + i, (unsigned long long)c);
    if (a.topic_hist)
        for (uint32_t i = threadIdx.x; i < nb * ntc; i += SP_THREADS)
            if (const uint32_t c = lt[i]) atomicAdd(a.topic_hist + i, (unsigned long long)c);
}

}  // namespace

// The counters are added to: the caller zeroes them first.
hipError_t launch_score_parts(const DevState& s, const KernParams& kp, const ScorePartsArgs& a, hipStream_t st) {
    if (s.n_pairs == 0) return hipSuccess;
    const dim3 grid((uint32_t)std::min<uint64_t>((s.n_pairs + SP_THREADS - 1) / SP_THREADS, COUNTER_GRID)),
        block(SP_THREADS);
    switch (s.n_topics) {
    case 1: hipLaunchKernelGGL(k_score_parts<1>, grid, block, 0, st, s, kp, a); break;
    case 2: hipLaunchKernelGGL(k_score_parts<2>, grid, block, 0, st, s, kp, a); break;
    case 4: hipLaunchKernelGGL(k_score_parts<4>, grid, block, 0, st, s, kp, a); break;
    case 8: hipLaunchKernelGGL(k_score_parts<8>, grid, block, 0, st, s, kp, a); break;
    default: hipLaunchKernelGGL(k_score_parts<0>, grid, block, 0, st, s, kp, a); break;
    }
    return hipGetLastError();
}

}  // namespace gsx
