// gsx_timed_traffic.hip — what the last timed propagation cost, and when
// (gsx_timed_traffic): its copies per message, node, link and tick bin, their
// bytes, and every node's peak upload and download per bin.
//
// A copy is message k sent by v to u.  v sends k at tick f (0 for its own
// messages, else arr[v][k] + vd) iff it holds k, k is accepted or its own, the
// pair (v -> u) carried the needed eligibility bit (PUBLISH for its own,
// FORWARD otherwise), u is not the peer v first got k from (from[(v -> u)]),
// u is not k's origin, and f <= max_ticks.  It arrives at f + lat[(u -> v)];
// past max_ticks it is IN_FLIGHT.  An arrived copy is GRAYLISTED when u's byte
// of v holds FWD_GIN, u's first receipt when k is in from[(u -> v)] (FIRST, or
// INVALID for the messages of drop[w]), else a duplicate (inside the P3 window
// iff arrival - arr[u][k] <= lim).  The eligibility is read from rfwd, the
// bytes the call's pin pass kept: a credit fold may have rewritten fwd.
//
// One wave per node u, lane = message of a 64-message word.  Per word the wave
// walks u's pairs q = (u -> v); per pair it gathers 128 B of arr[v], the
// origin word of v, the first-deliverer words of q and of its reverse, both
// rfwd bytes and both latencies, and classifies the copy v sent u (the
// receiver's side: class, arrival bin, window) and the copy u sent v (the
// sender's side: SENT / IN_FLIGHT; its send bin is the lane's own).  Every copy
// is so counted once on each side, by the wave that owns that side's node: the
// node and pair tables are written by their owner, and the node's bytes per
// bin live in an LDS table of the wave ([n_bins][2] u64), swept at the node's
// end for its peaks.  The per-message counters are lane-private over a node's
// pairs, then added to an LDS table of the block (the first TT_MW words; later
// words go to memory at once); the per-bin tables are LDS tables of the block
// up to TT_LDS_BINS bins, above that the lanes of a wave that share a bin add
// once.  Each non-zero block counter is flushed with one integer atomic.
// Integer adds only: the result does not depend on the schedule.
#include "gsx_device.h"
#include "gsx_wave.h"

#include <algorithm>

namespace gsx {

namespace {

constexpr uint32_t TT_MW = 16;         // message words of the block's LDS table: [TT_MW][TT_COLS][64] u32, 28 KB
constexpr uint32_t TT_LDS_BINS = 128;  // bins the block's LDS bin tables hold
constexpr uint32_t TT_MAX_BINS = 1024;
constexpr uint32_t TT_BLOCKS = 2048;   // blocks, about: each flushes its tables once

typedef unsigned long long u64a;

__device__ __forceinline__ void wave_sync() {  // the wave's LDS writes before its later LDS reads, lane to lane
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ u64a wave_sum64(u64a x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;  // (lane 0)
}
// g[key] += 1 for every active lane, the lanes of one key adding once
__device__ __forceinline__ void add_by_key(u64a* __restrict__ g, uint32_t key, bool active, uint32_t lane) {
    uint64_t m = __ballot(active);
    while (m) {
        const uint32_t l = (uint32_t)__builtin_ctzll(m);
        const uint32_t kk = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)l);
        const uint64_t peers = __ballot(active && key == kk);
        if (lane == l) atomicAdd(&g[kk], (u64a)__popcll(peers));
        m &= ~peers;
    }
}

// LB: n_bins <= TT_LDS_BINS, the block keeps the per-bin tables in LDS (4 waves);
// else 2 waves, each with a node table of TT_MAX_BINS bins.
template <bool LB>
__global__ __launch_bounds__(LB ? 256 : 128) void k_timed_traffic(PropState ps, TimedState ts, TimedTrafficArgs a) {
    constexpr uint32_t WAVES = LB ? 4 : 2, THREADS = WAVES * 64;
    constexpr uint32_t NB = LB ? TT_LDS_BINS : TT_MAX_BINS;
    __shared__ u64a nb_all[WAVES * NB * 2];                 // per wave: [bin][sent, arrived] bytes of its node
    __shared__ u64a bc[LB ? TT_LDS_BINS * TT_COLS : 1];     // [bin][column] copies
    __shared__ u64a bb[LB ? TT_LDS_BINS * 2 : 1];           // [bin][sent, arrived] bytes
    __shared__ uint32_t mt[TT_MW * TT_COLS * 64];           // [word][column][message of the word]
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t W = ps.n_words, n = ps.n_nodes, n_bins = a.n_bins, bin_ticks = a.bin_ticks;
    const uint32_t words = (ps.n_msgs + 63) / 64;  // (n_words may be padded: the padding holds no message)
    const uint32_t mw = words < TT_MW ? words : TT_MW;
    const size_t M = (size_t)W * 64;
    const uint32_t vd = ts.vd, max_ticks = ts.max_ticks, lim = ts.lim;
    const bool want_nb = a.bin_bytes || a.node_peak || a.node_peak_bin;
    const bool want_bins = want_nb || a.bin_copies;
    u64a* const nb = nb_all + (size_t)wave * NB * 2;
    if (want_nb)
        for (uint32_t i = lane; i < n_bins * 2; i += 64) nb[i] = 0;
    if (LB) {
        for (uint32_t i = threadIdx.x; i < n_bins * TT_COLS; i += THREADS) bc[i] = 0;
        for (uint32_t i = threadIdx.x; i < n_bins * 2; i += THREADS) bb[i] = 0;
    }
    if (a.msg_copies)
        for (uint32_t i = threadIdx.x; i < mw * TT_COLS * 64; i += THREADS) mt[i] = 0;
    __syncthreads();
    const uint32_t n_waves = gridDim.x * WAVES;
    for (uint32_t u = blockIdx.x * WAVES + wave; u < n; u += n_waves) {
        const int64_t q0 = ps.row_ptr[u], q1 = ps.row_ptr[u + 1];
        uint32_t nc[TT_COLS] = {0, 0, 0, 0, 0, 0, 0};  // the node's copies (wave-uniform)
        u64a up = 0, down = 0;                         // the lane's share of the node's bytes
        for (uint32_t w = 0; w < words; ++w) {
            const uint32_t k = w * 64 + lane;
            const bool live = k < ps.n_msgs;
            const uint32_t au = ts.arr[(size_t)u * M + k];
            const uint64_t own_uw = ts.origin[(size_t)u * W + w];
            const uint64_t drop_w = ps.drop ? ps.drop[w] : 0ull;
            const uint32_t sz = !live ? 0u : a.sizes ? a.sizes[k] : 1u;
            const bool own_u = (own_uw >> lane) & 1, dropped = (drop_w >> lane) & 1;
            const uint32_t fu = own_u ? 0u : au + vd;  // u's send tick
            const bool u_sends = live && au != 0xFFFFu && (own_u || !dropped) && fu <= max_ticks;
            uint32_t cm[TT_COLS] = {0, 0, 0, 0, 0, 0, 0};  // the lane's message: copies of this node's pairs
            for (int64_t q = q0; q < q1; ++q) {
                const uint32_t r = ps.rev[q];
                if (r == NO_PAIR || (r & HALO)) continue;
                const uint32_t v = (uint32_t)ps.col[q];
                const uint32_t f_vu = ps.rfwd[q], f_uv = ps.rfwd[r];  // the call's fwd bytes of (v -> u), (u -> v)
                const uint32_t l_vu = ts.lat[q], l_uv = ts.lat[r];    // ticks of a copy v sends u, u sends v
                const uint64_t from_q = ts.from[(size_t)q * W + w], from_r = ts.from[(size_t)r * W + w];
                const uint64_t own_vw = ts.origin[(size_t)v * W + w];
                const uint32_t av = ts.arr[(size_t)v * M + k];
                const bool own_v = (own_vw >> lane) & 1;
                const bool u_first_from_v = (from_q >> lane) & 1, v_first_from_u = (from_r >> lane) & 1;
                // the receiver's side: the copy v sent u
                const uint32_t fv = own_v ? 0u : av + vd;
                const bool sent_vu = live && av != 0xFFFFu && (own_v || !dropped) &&
                                     (f_vu & (own_v ? FWD_PUBLISH : FWD_FORWARD)) && !v_first_from_u && !own_u &&
                                     fv <= max_ticks;
                const uint32_t at = fv + l_vu;
                const bool arrived = sent_vu && at <= max_ticks;
                const bool gated = (f_uv & FWD_GIN) != 0;
                const uint32_t cls = gated ? TT_GRAY : !u_first_from_v ? TT_DUP : dropped ? TT_INVALID : TT_FIRST;
                const bool is_new = arrived && cls == TT_FIRST, is_dup = arrived && cls == TT_DUP;
                const bool is_inv = arrived && cls == TT_INVALID, is_gray = arrived && cls == TT_GRAY;
                const bool in_win = is_dup && at - au <= lim;
                // the sender's side: the copy u sent v
                const bool sent_uv = u_sends && (f_uv & (own_u ? FWD_PUBLISH : FWD_FORWARD)) && !u_first_from_v && !own_v;
                const bool flight = sent_uv && fu + l_uv > max_ticks;
                const uint64_t m_arr = __ballot(arrived);
                const uint64_t m_sent = __ballot(sent_uv);
                if (!(m_arr | m_sent)) continue;
                cm[TT_SENT] += sent_uv;
                cm[TT_FLIGHT] += flight;
                cm[TT_FIRST] += is_new;
                cm[TT_DUP] += is_dup;
                cm[TT_INVALID] += is_inv;
                cm[TT_GRAY] += is_gray;
                cm[TT_DUPWIN] += in_win;
                if (arrived) down += sz;
                if (sent_uv) up += sz;
                const uint32_t n_arr = (uint32_t)__popcll(m_arr);
                if (a.node_copies) {
                    nc[TT_SENT] += (uint32_t)__popcll(m_sent);
                    nc[TT_FLIGHT] += (uint32_t)__popcll(__ballot(flight));
                    if (n_arr) {
                        const uint32_t n_new = (uint32_t)__popcll(__ballot(is_new));
                        const uint32_t n_inv = (uint32_t)__popcll(__ballot(is_inv));
                        nc[TT_FIRST] += n_new;
                        nc[TT_INVALID] += n_inv;
                        if (gated) nc[TT_GRAY] += n_arr;
                        else nc[TT_DUP] += n_arr - n_new - n_inv;
                        nc[TT_DUPWIN] += (uint32_t)__popcll(__ballot(in_win));
                    }
                }
                if (n_arr && (a.pair_copies || a.pair_bytes)) {
                    u64a pb = n_arr;
                    if (a.pair_bytes && a.sizes) pb = wave_sum64(arrived ? sz : 0u);
                    if (lane == 0) {  // (q is this wave's: stored with one word, added over several)
                        if (words == 1) {
                            if (a.pair_copies) a.pair_copies[q] = n_arr;
                            if (a.pair_bytes) a.pair_bytes[q] = pb;
                        } else {
                            if (a.pair_copies) atomicAdd(&a.pair_copies[q], n_arr);
                            if (a.pair_bytes && pb) atomicAdd(&a.pair_bytes[q], pb);
                        }
                    }
                }
                if (want_bins && n_arr) {
                    const uint32_t b = min(at / bin_ticks, n_bins - 1);
                    if (want_nb && arrived && sz) atomicAdd(&nb[b * 2 + 1], (u64a)sz);
                    if (a.bin_copies) {
                        if (LB) {
                            if (arrived) atomicAdd(&bc[b * TT_COLS + cls], 1ull);
                            if (in_win) atomicAdd(&bc[b * TT_COLS + TT_DUPWIN], 1ull);
                        } else {
                            add_by_key(a.bin_copies, b * TT_COLS + cls, arrived, lane);
                            if (__ballot(in_win)) add_by_key(a.bin_copies, b * TT_COLS + TT_DUPWIN, in_win, lane);
                        }
                    }
                }
            }
            // the lane's message over the node's pairs; what u sent of it left in one bin, the lane's own
            if (want_bins && __ballot(cm[TT_SENT] != 0)) {
                const uint32_t b = min(fu / bin_ticks, n_bins - 1);
                const bool s = cm[TT_SENT] != 0;
                if (want_nb && s && sz) atomicAdd(&nb[b * 2], (u64a)sz * cm[TT_SENT]);
                if (a.bin_copies) {
                    if (LB) {
                        if (s) atomicAdd(&bc[b * TT_COLS + TT_SENT], (u64a)cm[TT_SENT]);
                        if (cm[TT_FLIGHT]) atomicAdd(&bc[b * TT_COLS + TT_FLIGHT], (u64a)cm[TT_FLIGHT]);
                    } else {
                        if (s) atomicAdd(&a.bin_copies[(size_t)b * TT_COLS + TT_SENT], (u64a)cm[TT_SENT]);
                        if (cm[TT_FLIGHT]) atomicAdd(&a.bin_copies[(size_t)b * TT_COLS + TT_FLIGHT], (u64a)cm[TT_FLIGHT]);
                    }
                }
            }
            if (a.msg_copies && live) {
#pragma unroll
                for (uint32_t c = 0; c < TT_COLS; ++c) {
                    if (!cm[c]) continue;
                    if (w < TT_MW) atomicAdd(&mt[(w * TT_COLS + c) * 64 + lane], cm[c]);
                    else atomicAdd(&a.msg_copies[(size_t)k * TT_COLS + c], cm[c]);
                }
            }
        }
        // the node's rows: plain stores by the wave that owns it
        if (a.node_copies && lane < TT_COLS) {
            uint32_t x = nc[0];
#pragma unroll
            for (uint32_t c = 1; c < TT_COLS; ++c) x = lane == c ? nc[c] : x;
            a.node_copies[(size_t)u * TT_COLS + lane] = x;
        }
        if (a.node_bytes) {
            const u64a su = wave_sum64(up), sd = wave_sum64(down);
            if (lane == 0) {
                a.node_bytes[(size_t)u * 2] = su;
                a.node_bytes[(size_t)u * 2 + 1] = sd;
            }
        }
        if (want_nb) {
            wave_sync();
            u64a pk[2] = {0, 0};
            uint32_t pkb[2] = {0, 0};
            for (uint32_t b = lane; b < n_bins; b += 64) {
#pragma unroll
                for (uint32_t d = 0; d < 2; ++d) {
                    const u64a x = nb[b * 2 + d];
                    if (!x) continue;
                    nb[b * 2 + d] = 0;
                    if (x > pk[d]) {  // (ascending b: the lane's lowest bin of its maximum)
                        pk[d] = x;
                        pkb[d] = b;
                    }
                    if (a.bin_bytes) {
                        if (LB) atomicAdd(&bb[b * 2 + d], x);
                        else atomicAdd(&a.bin_bytes[(size_t)b * 2 + d], x);
                    }
                }
            }
            if (a.node_peak || a.node_peak_bin) {
#pragma unroll
                for (uint32_t d = 0; d < 2; ++d)
                    for (int off = 32; off > 0; off >>= 1) {
                        const u64a ox = __shfl_down(pk[d], off, 64);
                        const uint32_t ob = __shfl_down(pkb[d], off, 64);
                        if (ox > pk[d] || (ox == pk[d] && ox && ob < pkb[d])) {
                            pk[d] = ox;
                            pkb[d] = ob;
                        }
                    }
                if (lane == 0) {
#pragma unroll
                    for (uint32_t d = 0; d < 2; ++d) {
                        if (a.node_peak) a.node_peak[(size_t)u * 2 + d] = pk[d];
                        if (a.node_peak_bin) a.node_peak_bin[(size_t)u * 2 + d] = pk[d] ? pkb[d] : 0u;
                    }
                }
            }
            wave_sync();
        }
    }
    __syncthreads();
    if (a.msg_copies)
        for (uint32_t i = threadIdx.x; i < mw * TT_COLS * 64; i += THREADS) {
            const uint32_t c = mt[i], k = (i / (TT_COLS * 64)) * 64 + (i & 63u), col = (i >> 6) % TT_COLS;
            if (c && k < ps.n_msgs) atomicAdd(&a.msg_copies[(size_t)k * TT_COLS + col], c);
        }
    if (LB) {
        if (a.bin_copies)
            for (uint32_t i = threadIdx.x; i < n_bins * TT_COLS; i += THREADS)
                if (bc[i]) atomicAdd(&a.bin_copies[i], bc[i]);
        if (a.bin_bytes)
            for (uint32_t i = threadIdx.x; i < n_bins * 2; i += THREADS)
                if (bb[i]) atomicAdd(&a.bin_bytes[i], bb[i]);
    }
}

}  // namespace

// Zeroes the requested outputs (the kernel adds to the tables several waves
// share and stores the rows a wave owns; a pair without copies is never
// stored), then the one pass.
hipError_t launch_timed_traffic(const PropState& ps, const TimedState& ts, const TimedTrafficArgs& a, hipStream_t st) {
    if (ps.n_nodes == 0 || ps.n_msgs == 0 || ps.n_pairs == 0) return hipSuccess;
    if (a.n_bins == 0 || a.n_bins > TT_MAX_BINS || a.bin_ticks == 0) return hipErrorInvalidValue;
    hipError_t rc = hipSuccess;
    auto zero = [&](void* p, size_t bytes) {
        if (p && rc == hipSuccess) rc = hipMemsetAsync(p, 0, bytes, st);
    };
    zero(a.msg_copies, 4 * (size_t)ps.n_msgs * TT_COLS);
    zero(a.pair_copies, 4 * ps.n_pairs);
    zero(a.pair_bytes, 8 * ps.n_pairs);
    zero(a.bin_copies, 8 * (size_t)a.n_bins * TT_COLS);
    zero(a.bin_bytes, 8 * (size_t)a.n_bins * 2);
    if (rc != hipSuccess) return rc;
    const bool lb = a.n_bins <= TT_LDS_BINS;
    const uint32_t waves = lb ? 4 : 2;
    const unsigned grid = std::min((ps.n_nodes + waves - 1) / waves, TT_BLOCKS * (lb ? 1u : 2u));
    if (lb) hipLaunchKernelGGL(k_timed_traffic<true>, dim3(grid), dim3(256), 0, st, ps, ts, a);
    else hipLaunchKernelGGL(k_timed_traffic<false>, dim3(grid), dim3(128), 0, st, ps, ts, a);
    return hipGetLastError();
}

}  // namespace gsx
