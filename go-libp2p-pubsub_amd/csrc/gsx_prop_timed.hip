// gsx_prop_timed.hip — propagation on a tick clock with a latency per directed
// link (gsx_propagate_timed, gsx_timed_results, gsx_timed_stats).
//
// The rule is gsx_propagate's (gsx_propagate.hip): the same fwd bytes, pins and
// compacted senders (k_prop_fwd / k_prop_pin / k_prop_compact), the same
// bit-sliced node-major rows, the lowest-indexed sender of a tick as the first
// deliverer without atomics (a receiver walks its senders in ascending order
// and every per-receiver word has one writer).  What differs is the clock: a
// copy v sends at tick f reaches u at f + lat[(u -> v)], so the rows a receiver
// pulls at tick t are of different send ticks.  They live in a ring:
//
//   ring [R][node][W]   slot f mod R = what the node sends at tick f (its
//                       accepted first receipts of tick f - vd; at f = 0 what
//                       it published), valid under its bit in rocc [R][node/64];
//   mark [R][node/64]   slot a mod R = the nodes some copy reaches at tick a.
//
// One launch per tick.  A wave takes 64 nodes' mark word; a zero word (nearly
// all of them, with heterogeneous latencies) costs that one load.  For a
// marked node, a lane per row word pulls the senders' rows of tick t - lat,
// settles first receipts and duplicates (the P3 window against the node's own
// arrival ticks, arr [node][message] u16, contiguous), writes the node's send
// row of tick t + vd and pushes the marks of its receivers at t + vd + lat.
// R is a power of two >= largest latency + vd + 2: the slots tick t reads
// (send ticks t - maxlat .. t - 1), writes (send tick t + vd, marks up to
// t + vd + maxlat) and clears for the next tick (mark slot t - 1, rocc slot
// t + 1 + vd) are then all distinct, so no slot needs a launch of its own.
// Integer and bit work only; no LDS outside the stats and export kernels.
#include "gsx_ops.h"

#include <algorithm>

namespace gsx {

namespace {

__device__ __forceinline__ uint64_t t_elig(uint32_t fw, uint64_t own) {  // elig_word of gsx_propagate.hip
    const uint32_t m = fw & (FWD_FORWARD | FWD_PUBLISH);
    if (m == (FWD_FORWARD | FWD_PUBLISH)) return ~0ull;
    if (m == FWD_FORWARD) return ~own;
    if (m == FWD_PUBLISH) return own;
    return 0;
}
__device__ __forceinline__ bool t_bit(const uint64_t* __restrict__ row, uint32_t v) {
    return (row[v / 64] >> (v % 64)) & 1;
}

// Sources: origin / seen / send row of tick 0 (ring slot 0, zeroed by the
// caller), its occupancy bit, arrival tick 0.
__global__ __launch_bounds__(256) void k_timed_init(PropState ps, TimedState ts) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= ps.n_msgs) return;
    const uint32_t u = ps.msgs[k].source;
    if (u >= ps.n_nodes) return;
    const size_t i = (size_t)u * ps.n_words + k / 64;
    const unsigned long long bit = 1ull << (k % 64);
    atomicOr((unsigned long long*)&ts.origin[i], bit);
    atomicOr((unsigned long long*)&ts.seen[i], bit);
    atomicOr((unsigned long long*)&ts.ring[i], bit);
    atomicOr((unsigned long long*)&ts.rocc[u / 64], 1ull << (u % 64));
    ts.arr[(size_t)u * ps.n_words * 64 + k] = 0;
}

// Tick t.  INIT: tick 0, the sources only push (they hold their rows already).
template <bool INIT>
__global__ __launch_bounds__(256) void k_timed_tick(PropState ps, TimedState ts, uint32_t t) {
    const uint32_t W = ps.n_words, R1 = ts.R - 1, n = ps.n_nodes;
    const size_t orow = ((size_t)n + 63) / 64;
    const size_t plane = (size_t)n * W;
    const uint32_t fs = INIT ? 0u : t + ts.vd;  // the send tick of this tick's receipts
    uint64_t* __restrict__ ring_w = ts.ring + (size_t)(fs & R1) * plane;
    uint64_t* __restrict__ rocc_w = ts.rocc + (size_t)(fs & R1) * orow;
    const uint64_t* __restrict__ mark_t = INIT ? ts.rocc : ts.mark + (size_t)(t & R1) * orow;
    uint64_t* __restrict__ mark_prev = ts.mark + (size_t)((t - 1) & R1) * orow;
    uint64_t* __restrict__ rocc_next = ts.rocc + (size_t)((t + 1 + ts.vd) & R1) * orow;
    const uint32_t lane = threadIdx.x & 63u;
    const size_t wave = ((size_t)blockIdx.x * 256u + threadIdx.x) / 64, n_waves = (size_t)gridDim.x * 4;
    unsigned long long n_new = 0, n_dup = 0, n_in = 0, n_rej = 0, n_ign = 0, n_gray = 0, n_marked = 0;
    uint32_t last_tick = 0, last_copy = 0;
    for (size_t i = wave; i < orow; i += n_waves) {
        const uint64_t mw = mark_t[i];
        if (!INIT && lane == 0) {  // the slots the next tick reuses
            mark_prev[i] = 0;
            rocc_next[i] = 0;
        }
        if (!mw) continue;
        const uint32_t cnt = (uint32_t)__popcll(mw);
        if (lane == 0) n_marked += cnt;
        for (uint32_t j = lane; j < cnt * W; j += 64) {
            uint64_t x = mw;
            for (uint32_t s = j / W; s; --s) x &= x - 1;
            const uint32_t u = (uint32_t)i * 64 + (uint32_t)__builtin_ctzll(x);
            const uint32_t w = j % W;
            const size_t uw = (size_t)u * W + w;
            uint64_t row;  // what u sends at tick fs, word w
            if (INIT) {
                row = ring_w[uw];
            } else {
                const uint64_t seen = ts.seen[uw], own_u = ts.origin[uw];
                const uint64_t drp = ps.drop ? ps.drop[w] : 0ull, rej = ps.drop ? ps.reject[w] : 0ull;
                uint16_t* __restrict__ ar = ts.arr + ((size_t)u * W + w) * 64;
                uint64_t sa = seen;
                const int64_t k1 = ps.cend[u];
                for (int64_t k = ps.row_ptr[u]; k < k1; ++k) {
                    const uint2 en = ps.cent[k];
                    const uint32_t q = en.y, v = en.x & PIN_NODE_MASK;
                    const uint32_t l = ts.lat[q];
                    if (l > t) continue;
                    const uint32_t sl = (t - l) & R1;
                    if (!t_bit(ts.rocc + (size_t)sl * orow, v)) continue;
                    uint64_t c = ts.ring[(size_t)sl * plane + (size_t)v * W + w];
                    if (!c) continue;
                    // v's targets: eligibility, never back to its first deliverer, never to the origin
                    c &= t_elig(en.x >> PIN_FWD_SHIFT, ts.origin[(size_t)v * W + w]);
                    c &= ~ts.from[(size_t)ps.rev[q] * W + w] & ~own_u;
                    if (!c) continue;
                    const uint64_t nb = c & ~sa;  // not seen, not from a lower sender of this tick
                    sa |= nb;
                    if (nb) {
                        ts.from[(size_t)q * W + w] |= nb;
                        for (uint64_t b = nb; b; b &= b - 1) ar[__builtin_ctzll(b)] = (uint16_t)t;
                        const uint32_t fresh = (uint32_t)__popcll(nb & ~drp), inv = (uint32_t)__popcll(nb & drp & rej);
                        n_new += fresh;
                        n_rej += inv;
                        n_ign += __popcll(nb & drp & ~rej);
                        if (fresh) atomicAdd(&ts.fcnt[q], fresh);
                        if (inv) atomicAdd(&ts.icnt[q], inv);
                    }
                    uint64_t d = c & ~nb;
                    if (d) {
                        n_dup += __popcll(d);
                        uint32_t in = 0;
                        for (; d; d &= d - 1) in += t - ar[__builtin_ctzll(d)] <= ts.lim;
                        n_in += in;
                        if (in) atomicAdd(&ts.dcnt[q], in);
                    }
                }
                const uint64_t acc = sa ^ seen;
                if (acc) {
                    ts.seen[uw] = sa;
                    last_tick = t;
                }
                row = acc & ~drp;  // validation drops the rest: seen, not forwarded
                ring_w[uw] = row;  // (every word of a marked node: the slot's last tenant is gone)
                if (row) atomicOr((unsigned long long*)&rocc_w[u / 64], 1ull << (u % 64));
            }
            if (!row) continue;
            // u's sends of tick fs: mark each receiver at its arrival tick (a graylisting
            // receiver drops the copies before pushMsg: counted, never marked)
            const uint8_t need = INIT ? FWD_PUBLISH : FWD_FORWARD;
            for (int64_t r = ps.row_ptr[u]; r < ps.row_ptr[u + 1]; ++r) {
                if (!(ps.fwd[r] & need)) continue;
                const uint32_t q = ps.rev[r];
                if (q == NO_PAIR) continue;
                const uint32_t xn = (uint32_t)ps.col[r];
                const uint64_t s = row & ~ts.from[(size_t)r * W + w] & ~ts.origin[(size_t)xn * W + w];
                if (!s) continue;
                const uint32_t at = fs + ts.lat[q];
                if (at > ts.max_ticks) continue;  // still in flight when the call ends
                last_copy = at > last_copy ? at : last_copy;
                if (ps.rfwd[r] & FWD_GIN) {
                    n_gray += __popcll(s);
                    continue;
                }
                atomicOr((unsigned long long*)&ts.mark[(size_t)(at & R1) * orow + xn / 64], 1ull << (xn % 64));
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        last_tick = max(last_tick, (uint32_t)__shfl_down(last_tick, off, 64));
        last_copy = max(last_copy, (uint32_t)__shfl_down(last_copy, off, 64));
    }
    if (lane == 0 && last_tick) atomicMax(&ts.stats[TS_LAST_TICK], (unsigned long long)last_tick);
    if (lane == 0 && last_copy) atomicMax(&ts.stats[TS_LAST_COPY], (unsigned long long)last_copy);
    unsigned long long cntv[7] = {n_new, n_dup, n_in, n_rej, n_ign, n_gray, n_marked};
    const uint32_t slot[7] = {TS_DELIV, TS_DUPS, TS_DUPS_IN, TS_REJ, TS_IGN, TS_GRAY, TS_MARKED};
    block_count<7>(cntv, ts.stats, slot);
}

__global__ __launch_bounds__(256) void k_timed_add(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src,
                                                   uint64_t n) {
    for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < n; q += (uint64_t)gridDim.x * 256u) {
        const uint32_t c = src[q];
        if (c) dst[q] += c;
    }
}

// [node][64 W] -> [message][node]: a block transposes 64 nodes x 64 messages through LDS.
__global__ __launch_bounds__(256) void k_timed_export(PropState ps, TimedState ts, uint16_t* __restrict__ out) {
    __shared__ uint16_t tile[64][65];
    const uint32_t w = blockIdx.y, u0 = blockIdx.x * 64u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t M = (size_t)ps.n_words * 64;
    for (uint32_t i = wave; i < 64; i += 4) {
        const uint32_t u = u0 + i;
        tile[i][lane] = u < ps.n_nodes ? ts.arr[(size_t)u * M + w * 64 + lane] : (uint16_t)0xFFFF;
    }
    __syncthreads();
    for (uint32_t i = wave; i < 64; i += 4) {
        const uint32_t k = w * 64 + i, u = u0 + lane;
        if (k < ps.n_msgs && u < ps.n_nodes) out[(size_t)k * ps.n_nodes + u] = tile[lane][i];
    }
}

// gsx_timed_stats.  Block (w, node range): lane b of a wave holds message 64 w + b
// and walks the range's nodes, one coalesced 128-B row piece per node.  Up to
// TS_LDS_BINS bins the block counts in LDS ([message of the word][bin]) and
// flushes its non-zero counters; above, the bins spread the global adds.
constexpr uint32_t TS_LDS_BINS = 128;
__global__ __launch_bounds__(256) void k_timed_stats(PropState ps, TimedState ts, uint32_t nodes_per_block,
                                                     uint32_t bin_ticks, uint32_t n_bins, uint32_t* __restrict__ hist,
                                                     uint32_t* __restrict__ node_received,
                                                     unsigned long long* __restrict__ node_tick_sum) {
    __shared__ uint32_t cnt[64 * TS_LDS_BINS];
    const bool lds = n_bins <= TS_LDS_BINS;
    const uint32_t w = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lds)
        for (uint32_t i = threadIdx.x; i < 64 * n_bins; i += 256) cnt[i] = 0;
    __syncthreads();
    const uint32_t k = w * 64 + lane;
    const bool live = k < ps.n_msgs;
    const size_t M = (size_t)ps.n_words * 64;
    const uint32_t u_end = min(ps.n_nodes, (blockIdx.y + 1) * nodes_per_block);
    for (uint32_t u = blockIdx.y * nodes_per_block + wave; u < u_end; u += 4) {
        const uint32_t a = ts.arr[(size_t)u * M + k];
        const bool got = live && a != 0xFFFFu;
        if (got && hist) {
            const uint32_t b = min(a / bin_ticks, n_bins - 1);
            if (lds) atomicAdd(&cnt[lane * n_bins + b], 1u);
            else atomicAdd(&hist[(size_t)k * n_bins + b], 1u);
        }
        if (node_received || node_tick_sum) {
            uint32_t nr = got && a >= 1, ns = got ? a : 0u;
            for (int off = 32; off > 0; off >>= 1) {
                nr += __shfl_down(nr, off, 64);
                ns += __shfl_down(ns, off, 64);
            }
            if (lane == 0 && nr) {
                if (node_received) atomicAdd(&node_received[u], nr);
                if (node_tick_sum) atomicAdd(&node_tick_sum[u], (unsigned long long)ns);
            }
        }
    }
    __syncthreads();
    if (lds && hist)
        for (uint32_t i = threadIdx.x; i < 64 * n_bins; i += 256) {
            const uint32_t c = cnt[i], kk = w * 64 + i / n_bins;
            if (c && kk < ps.n_msgs) atomicAdd(&hist[(size_t)kk * n_bins + i % n_bins], c);
        }
}

inline unsigned nblk(uint64_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

}  // namespace

hipError_t launch_timed_init(const PropState& ps, const TimedState& ts, hipStream_t st) {
    if (ps.n_msgs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_timed_init, dim3(nblk(ps.n_msgs, 256)), dim3(256), 0, st, ps, ts);
    return hipGetLastError();
}

hipError_t launch_timed_tick(const PropState& ps, const TimedState& ts, uint32_t t, hipStream_t st) {
    if (ps.n_nodes == 0) return hipSuccess;
    // a wave per 64-node mark word, capped: the empty words of a tick are a few loads per wave
    const dim3 g(std::min(nblk(((uint64_t)ps.n_nodes + 63) / 64, 4), COUNTER_GRID)), b(256);
    if (t == 0) hipLaunchKernelGGL(k_timed_tick<true>, g, b, 0, st, ps, ts, t);
    else hipLaunchKernelGGL(k_timed_tick<false>, g, b, 0, st, ps, ts, t);
    return hipGetLastError();
}

hipError_t launch_timed_add(uint32_t* dst, const uint32_t* src, uint64_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_timed_add, dim3(std::min(nblk(n, 256), COUNTER_GRID)), dim3(256), 0, st, dst, src, n);
    return hipGetLastError();
}

hipError_t launch_timed_export(const PropState& ps, const TimedState& ts, uint16_t* tick_mn, hipStream_t st) {
    if (ps.n_nodes == 0 || ps.n_msgs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_timed_export, dim3(nblk(ps.n_nodes, 64), (ps.n_msgs + 63) / 64), dim3(256), 0, st, ps, ts,
                       tick_mn);
    return hipGetLastError();
}

hipError_t launch_timed_stats(const PropState& ps, const TimedState& ts, uint32_t bin_ticks, uint32_t n_bins,
                              uint32_t* hist, uint32_t* node_received, unsigned long long* node_tick_sum,
                              hipStream_t st) {
    if (ps.n_nodes == 0 || ps.n_msgs == 0) return hipSuccess;
    const uint32_t words = (ps.n_msgs + 63) / 64;
    // about 2048 blocks in all: fewer flush fewer LDS counters, more hide more load latency
    const uint32_t ranges = std::min({std::max(2048u / words, 1u), (ps.n_nodes + 3) / 4, 65535u});
    const uint32_t npb = (ps.n_nodes + ranges - 1) / ranges;
    hipLaunchKernelGGL(k_timed_stats, dim3(words, (ps.n_nodes + npb - 1) / npb), dim3(256), 0, st, ps, ts, npb,
                       bin_ticks, n_bins, hist, node_received, node_tick_sum);
    return hipGetLastError();
}

}  // namespace gsx
