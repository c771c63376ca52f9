// gsx_score_stats.hip — threshold standings of the score vector
// (gsx_score_stats), reduced on the device: the selected pairs per score bin
// for the whole engine, per observer row and per peer, and the lowest selected
// score per row and per peer, without the score vector ever leaving HBM.
//
// One pass over the pairs in pair order, a wave per 64 consecutive pairs,
// grid-stride over a bounded grid.  Per pair: flags (1 B), the topic's record
// flag under MESH (1 B), the score (8 B, selected pairs only), the observer
// (4 B, observer view) and the peer (4 B, peer view); every load is the wave's
// contiguous span.  What bounds the pass is how it accumulates:
//   * hist: one ballot per bin gives the wave's count (a scalar), summed per
//     wave over its iterations, then over the block's four waves in LDS, then
//     ONE global atomic per block and bin;
//   * observer view: a row's pairs are contiguous, so the lanes of a wave that
//     share pair_obs form a run.  The per-bin ballot masked to the run, popcount
//     taken by the run's first lane, is the row's count in this wave: one
//     update per (row segment, bin).  A run that neither began in the wave
//     before nor goes on in the wave after is the whole row: a plain store
//     (the outputs start zeroed).  Only the rows cut by a wave's edge add with
//     an atomic — at most two runs per wave, and a hub row of thousands of
//     pairs costs one atomic per bin and wave.  The row minimum follows the
//     same segmentation (a segmented shuffle-min over the run);
//   * peer view: the targets col[p] are scattered, nothing shares a
//     destination on chip: one no-return u32 atomic add per selected pair, and
//     an atomic min only when the lane's value is below the value read first.
// Minima are taken on score_key(), the order-preserving u64 image of a
// double, so the atomic is an integer min; k_ss_fill presets the key of +inf
// and k_ss_unkey turns the keys back into doubles in place.  Integer adds and
// integer mins commute: the result is bit-identical from run to run and does
// not depend on the grid.
#include "gsx_ops.h"

#include <algorithm>

namespace gsx {

namespace {

constexpr uint32_t SS_THREADS = 256, SS_WAVES = SS_THREADS / 64;

// Doubles ordered as unsigned integers: negative values have every bit
// flipped, the others the sign bit set (-inf < ... < -0.0 < +0.0 < ... < +inf).
__host__ __device__ __forceinline__ unsigned long long score_key(double s) {
    const unsigned long long b = (unsigned long long)__builtin_bit_cast(long long, s);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ double score_unkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return __builtin_bit_cast(double, (long long)b);
}
constexpr unsigned long long KEY_INF = 0xFFF0000000000000ull;  // score_key(+inf)

__global__ __launch_bounds__(SS_THREADS) void k_ss_fill(unsigned long long* __restrict__ a, uint64_t na,
                                                        unsigned long long* __restrict__ b, uint64_t nb) {
    for (uint64_t i = (uint64_t)blockIdx.x * SS_THREADS + threadIdx.x; i < na + nb; i += (uint64_t)gridDim.x * SS_THREADS)
        (i < na ? a[i] : b[i - na]) = KEY_INF;
}

__global__ __launch_bounds__(SS_THREADS) void k_ss_unkey(unsigned long long* __restrict__ a, uint64_t na,
                                                         unsigned long long* __restrict__ b, uint64_t nb) {
    for (uint64_t i = (uint64_t)blockIdx.x * SS_THREADS + threadIdx.x; i < na + nb;
         i += (uint64_t)gridDim.x * SS_THREADS) {
        unsigned long long* p = i < na ? a + i : b + (i - na);
        *p = (unsigned long long)__builtin_bit_cast(long long, score_unkey(*p));
    }
}

__global__ __launch_bounds__(SS_THREADS) void k_score_stats(ScoreStatsArgs a) {
    __shared__ uint32_t part[SS_MAX_BINS][SS_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t nb = a.n_edges + 1;
    const bool obs_view = a.obs_bins || a.obs_min;
    uint32_t hcnt[SS_MAX_BINS];  // this wave's selected pairs per bin (wave-uniform)
#pragma unroll
    for (uint32_t k = 0; k < SS_MAX_BINS; ++k) hcnt[k] = 0;

    // (base is wave-uniform: a wave's lanes stay in the loop together)
    for (uint64_t base = ((uint64_t)blockIdx.x * SS_WAVES + wave) * 64; base < a.n_pairs;
         base += (uint64_t)gridDim.x * SS_THREADS) {
        const uint64_t p = base + lane;
        const bool valid = p < a.n_pairs;
        bool sel = false;
        if (valid) {
            const uint8_t pf = a.pflags[p];
            sel = a.select == SS_PRESENT ? (pf & PAIR_PRESENT) != 0
                                         : (pf & (PAIR_PRESENT | PAIR_CONNECTED)) == (PAIR_PRESENT | PAIR_CONNECTED);
            if (sel && a.select == SS_MESH) sel = (a.rflags[flag_index(p, a.topic, a.n_topics)] & REC_IN_MESH) != 0;
        }
        uint32_t bin = 0;
        unsigned long long key = KEY_INF;
        if (sel) {
            const double s = a.score[p];
            // the edges the score is not below: a NaN is below none (the router's `score < threshold`
            // is false for it) and lands in the top bin
#pragma unroll
            for (uint32_t k = 0; k < SS_MAX_EDGES; ++k) bin += (k < a.n_edges && !(s < a.edges[k])) ? 1u : 0u;
            // the minima skip a NaN: its key would sort by its sign bit, below -inf or above +inf
            if (s == s) key = score_key(s);
        }

        // the run of lanes that share this lane's observer: [first lane with `head`, end]
        uint32_t obs = 0xFFFFFFFFu, end = 63;
        bool head = false, shared = false;
        uint64_t run = 0;
        if (obs_view) {
            if (valid) obs = a.pair_obs[p];
            const uint32_t prev = (uint32_t)__shfl_up((int)obs, 1, 64);
            head = lane == 0 || prev != obs;
            const uint64_t heads = __ballot(head);
            const uint64_t above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
            const uint32_t next = above ? (uint32_t)__builtin_ctzll(above) : 64u;
            end = next - 1;
            run = (next == 64 ? ~0ull : (1ull << next) - 1) & (~0ull << lane);  // (a head lane's: the whole run)
            // the row goes on beyond this wave's pairs: its other segments add to the same counters
            const bool lo = lane == 0 && valid && p > 0 && a.pair_obs[p - 1] == obs;
            const bool hi = lane == 63 && p + 1 < a.n_pairs && a.pair_obs[p + 1] == obs;
            const uint64_t cl = __ballot(lo), ch = __ballot(hi);
            shared = (lane == 0 && cl != 0) || (next == 64 && ch != 0);
            head = head && valid;
        }

#pragma unroll
        for (uint32_t k = 0; k < SS_MAX_BINS; ++k) {
            if (k < nb) {
                const uint64_t b = __ballot(sel && bin == k);
                hcnt[k] += (uint32_t)__popcll(b);
                if (a.obs_bins && head) {
                    const uint32_t c = (uint32_t)__popcll(b & run);
                    if (c) {
                        uint32_t* dst = a.obs_bins + (size_t)obs * nb + k;
                        if (shared) atomicAdd(dst, c);
                        else *dst = c;
                    }
                }
            }
        }

        if (a.obs_min) {  // segmented min: after the step of 2^j a lane holds its run's [lane, lane + 2^(j+1))
            unsigned long long m = key;
#pragma unroll
            for (uint32_t off = 1; off < 64; off <<= 1) {
                const unsigned long long o = __shfl_down(m, off, 64);
                if (lane + off <= end && o < m) m = o;
            }
            if (head && m != KEY_INF) {
                if (shared) atomicMin(a.obs_min + obs, m);
                else a.obs_min[obs] = m;
            }
        }

        if (sel && (a.peer_bins || a.peer_min)) {
            const uint32_t v = (uint32_t)a.col[p];
            if (a.peer_bins) atomicAdd(a.peer_bins + (size_t)v * nb + bin, 1u);
            // the read is a hint (a stale value is only ever higher): the atomic decides
            if (a.peer_min && key < a.peer_min[v]) atomicMin(a.peer_min + v, key);
        }
    }

    if (a.hist) {
        if (lane == 0)
#pragma unroll
            for (uint32_t k = 0; k < SS_MAX_BINS; ++k) part[k][wave] = hcnt[k];
        __syncthreads();
        if (threadIdx.x < nb) {
            unsigned long long t = 0;
            for (uint32_t w = 0; w < SS_WAVES; ++w) t += part[threadIdx.x][w];
            if (t) atomicAdd(a.hist + threadIdx.x, t);
        }
    }
}

uint32_t span_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + SS_THREADS - 1) / SS_THREADS, COUNTER_GRID); }

}  // namespace

// +inf, in key form, into both minimum arrays (either may be null / empty).
hipError_t launch_score_stats_fill(unsigned long long* obs_min, uint64_t n_obs, unsigned long long* peer_min,
                                   uint64_t n_peer, hipStream_t st) {
    if (!obs_min) n_obs = 0;
    if (!peer_min) n_peer = 0;
    if (n_obs + n_peer == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ss_fill, dim3(span_grid(n_obs + n_peer)), dim3(SS_THREADS), 0, st, obs_min, n_obs, peer_min,
                       n_peer);
    return hipGetLastError();
}

// The counters are added to and the minima lowered: the caller zeroes /
// fills them first (launch_score_stats_fill), and turns the minima's keys
// into doubles after (launch_score_stats_unkey).
hipError_t launch_score_stats(const ScoreStatsArgs& a, hipStream_t st) {
    if (a.n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_score_stats, dim3(span_grid(a.n_pairs)), dim3(SS_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_score_stats_unkey(unsigned long long* obs_min, uint64_t n_obs, unsigned long long* peer_min,
                                    uint64_t n_peer, hipStream_t st) {
    if (!obs_min) n_obs = 0;
    if (!peer_min) n_peer = 0;
    if (n_obs + n_peer == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ss_unkey, dim3(span_grid(n_obs + n_peer)), dim3(SS_THREADS), 0, st, obs_min, n_obs, peer_min,
                       n_peer);
    return hipGetLastError();
}

}  // namespace gsx
