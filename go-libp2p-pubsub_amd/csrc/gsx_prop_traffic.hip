// gsx_prop_traffic.hip — what the last propagation call cost (gsx_prop_traffic):
// its copies per message, per node and per link, by what the receiver's
// router did with each, and their bytes.
//
// A copy is message k sent by v to u.  For the receiver's pair q = (u -> v)
// and a message word, the copies v sent u are k_prop_dup_rows' rule
//   sent = sset[v] & (elig(v -> u, own_v) | sel[rev q]) & ~from[rev q] & ~own_u
// (sset[v]: what v forwarded at a hop that ran, its own messages at hop 0;
// never back to the peer v first got the message from, never to its origin),
// also for a pair whose copies u's AcceptFrom drops (pin NO_PAIR while the
// reverse pair sends): those are the GRAYLISTED class.  Of the other pairs'
// copies, the ones in q's first-deliverer row are u's first receipts (FIRST,
// or INVALID for the messages of drop[w]); the rest are duplicates.  The
// first-deliverer rows of a tracked call hold the hop-1 receipts of dropped
// messages too (k_prop_hop<.., true>), so dseen is not needed.
//
// Two passes.  k_traffic_sendset ORs each node's history rows once (a node
// forwards a message at most once, so the OR loses nothing).
// k_traffic_pairs gives every pair one lane of a wave and walks the words:
// per word one gathered sset row, the first-deliverer rows of q and of its
// reverse, sel if present.  The eligibility comes from the bytes the call
// left behind (rfwd, pin), not from the scores: credits may have moved those.
// Per message: column popcounts of the wave's 64 rows (wave_transpose64) into
// an LDS table, one global atomic per non-zero counter at the end.  Per node:
// one atomic per (pair, non-zero column) on the receiver's side, one per pair
// on the sender's.  Integer adds only: the result does not depend on the
// schedule.
#include "gsx_device.h"
#include "gsx_wave.h"

#include <algorithm>
#include <cstdlib>

namespace gsx {

namespace {

constexpr uint32_t TR_THREADS = 256, TR_WAVES = TR_THREADS / 64;
constexpr uint32_t TR_WC = 16;  // words a block counts at a time: the LDS table is [TR_WC][TR_TAB][64] u32, 12 KB
constexpr uint32_t TR_TAB = 3;  // per message: every copy, first receipts (FIRST + INVALID), graylisted copies
constexpr uint32_t TR_BLOCKS = 2048;  // blocks of the pair pass, about (launch_prop_traffic)
constexpr uint32_t TR_BATCH = 4;  // history rows in flight per thread (k_traffic_sendset)

__device__ __forceinline__ uint64_t tr_elig(uint32_t fw, uint64_t own) {  // elig_word of gsx_propagate.hip
    const uint32_t m = fw & (FWD_FORWARD | FWD_PUBLISH);
    return m == (FWD_FORWARD | FWD_PUBLISH) ? ~0ull : m == FWD_FORWARD ? ~own : m == FWD_PUBLISH ? own : 0ull;
}
__device__ __forceinline__ bool tr_occ(const uint64_t* __restrict__ occ, uint32_t v) {
    return (occ[v / 64] >> (v % 64)) & 1;
}

// sset[node][word]: the node's history rows of the hops that ran (h < max_hops,
// row 0 its own messages), each under its occupancy bit.  Thread per (node,
// word); the rows are loaded TR_BATCH at a time.
__global__ __launch_bounds__(256) void k_traffic_sendset(PropState ps, uint64_t* __restrict__ sset) {
    const uint32_t W = ps.n_words;
    const size_t plane = (size_t)ps.n_nodes * W;
    const size_t occ_row = ((size_t)ps.n_nodes + 63) / 64;
    uint32_t h_end = ps.n_rows < ps.max_hops ? ps.n_rows : ps.max_hops;  // rows forwarded in a hop that ran
    if (h_end > 64) h_end = 64;                                          // (max_hops <= GSX_MAX_HOPS)
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < plane; i += (size_t)gridDim.x * 256u) {
        const uint32_t u = (uint32_t)(i / W);
        uint64_t rm = 0;  // bit h: the node is occupied at hop h
        for (uint32_t h = 0; h < h_end; ++h) rm |= (uint64_t)tr_occ(ps.occ + (size_t)h * occ_row, u) << h;
        uint64_t x = 0;
        while (rm) {
            uint32_t hs[TR_BATCH];
            bool on[TR_BATCH];
#pragma unroll
            for (uint32_t j = 0; j < TR_BATCH; ++j) {
                on[j] = rm != 0;
                hs[j] = rm ? (uint32_t)__builtin_ctzll(rm) : 0u;
                rm &= rm - 1;
            }
#pragma unroll
            for (uint32_t j = 0; j < TR_BATCH; ++j)
                if (on[j]) x |= ps.hist[(size_t)hs[j] * plane + i];
        }
        sset[i] = x;
    }
}

// Block (x, y): the words x * TR_WC .. of the pair tiles y * tiles_per_block ..;
// one wave per tile of 64 consecutive pairs, lane = pair.  FULL: the per-node
// or per-pair outputs are wanted; else only the per-message table is counted.
// `multi`: more than one word chunk, so a pair's counts come from several
// blocks and are added; else they are stored.
template <bool FULL>
__global__ __launch_bounds__(TR_THREADS) void k_traffic_pairs(PropState ps, TrafficArgs a, uint32_t tiles_per_block,
                                                              uint32_t multi) {
    __shared__ uint32_t cnt[TR_WC * TR_TAB * 64];  // [word of the chunk][table][message of the word]
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t W = ps.n_words;
    const uint32_t words = (ps.n_msgs + 63) / 64;  // (n_words may be padded: the padding holds no message)
    const uint32_t w0 = blockIdx.x * TR_WC;
    const uint32_t wn = words - w0 < TR_WC ? words - w0 : TR_WC;
    if (a.msg_copies) {
        for (uint32_t i = threadIdx.x; i < wn * TR_TAB * 64; i += TR_THREADS) cnt[i] = 0;
        __syncthreads();
    }
    const uint64_t E = ps.n_pairs;
    const uint64_t n_tiles = (E + 63) / 64;
    const uint64_t t_last = ((uint64_t)blockIdx.y + 1) * tiles_per_block;
    const uint64_t t_end = t_last < n_tiles ? t_last : n_tiles;
    for (uint64_t t = (uint64_t)blockIdx.y * tiles_per_block + wave; t < t_end; t += TR_WAVES) {
        const uint64_t q = t * 64 + lane;
        const bool in = q < E;
        const uint32_t r = in ? ps.rev[q] : NO_PAIR;
        const uint32_t rf = in ? ps.rfwd[q] : 0u;  // fwd of (v -> u) as the call's pin pass read it
        // v sends to u at all; u's AcceptFrom drops the copies (pin_of: NO_PAIR although the reverse pair sends)
        const bool sends = in && r != NO_PAIR && !(r & HALO) && (rf & FWD_SEND);
        if (!FULL && __ballot(sends) == 0) continue;
        const bool gated = sends && ps.pin[q] == NO_PAIR;
        const uint32_t u = in ? ps.pair_obs[q] : NO_PAIR;
        const uint32_t v = in ? (uint32_t)ps.col[q] : 0u;
        const bool v_src = sends && tr_occ(ps.occ, v), u_src = sends && tr_occ(ps.occ, u);
        const bool any_gray = __ballot(gated) != 0;
        const size_t vw = (size_t)v * W, uw = (size_t)u * W, rw = (size_t)r * W, qw = (size_t)q * W;
        uint32_t c_sent = 0, c_first = 0, c_inv = 0;
        unsigned long long bytes = 0;
        for (uint32_t wi = 0; wi < wn; ++wi) {
            const uint32_t w = w0 + wi;
            uint64_t s = 0, f = 0;
            if (sends) {
                uint64_t el = tr_elig(rf, v_src ? ps.hist[vw + w] : 0ull);  // (row 0 of hist: published)
                if (ps.sel) el |= ps.sel[rw + w];
                s = a.sset[vw + w] & el & ~ps.from_mask[rw + w];
                if (u_src) s &= ~ps.hist[uw + w];
                if (!gated) f = ps.from_mask[qw + w];
            }
            if (a.msg_copies) {
                uint32_t* const tab = cnt + wi * TR_TAB * 64 + lane;
                uint32_t c = (uint32_t)__popcll(wave_transpose64(s, lane));
                if (c) atomicAdd(tab, c);
                c = (uint32_t)__popcll(wave_transpose64(f, lane));
                if (c) atomicAdd(tab + 64, c);
                if (any_gray) {
                    c = (uint32_t)__popcll(wave_transpose64(gated ? s : 0ull, lane));
                    if (c) atomicAdd(tab + 128, c);
                }
            }
            if (FULL) {
                const uint64_t drop = ps.drop ? ps.drop[w] : 0ull;
                c_sent += (uint32_t)__popcll(s);
                c_first += (uint32_t)__popcll(f & ~drop);
                c_inv += (uint32_t)__popcll(f & drop);
                for (uint32_t j = 0; j < a.n_planes; ++j)  // (wave-uniform words: scalar loads)
                    bytes += (unsigned long long)__popcll(s & a.planes[(size_t)j * W + w]) << j;
            }
        }
        if (!FULL) continue;
        if (!a.planes) bytes = c_sent;
        if (in) {
            if (multi) {
                if (a.pair_copies && c_sent) atomicAdd(&a.pair_copies[q], c_sent);
                if (a.pair_bytes && bytes) atomicAdd(&a.pair_bytes[q], bytes);
            } else {
                if (a.pair_copies) a.pair_copies[q] = c_sent;
                if (a.pair_bytes) a.pair_bytes[q] = bytes;
            }
            if (c_sent && a.node_copies) atomicAdd(&a.node_copies[(size_t)v * TRAFFIC_COLS + TR_SENT], c_sent);
            if (bytes && a.node_bytes) atomicAdd(&a.node_bytes[(size_t)v * 2], bytes);
        }
        // the receiver's side: one atomic per (pair, non-zero class); a node's pairs are
        // neighbouring lanes, so the adds of a wave fall into a few cache lines
        if (in && c_sent) {
            const uint32_t x[4] = {c_first, gated ? 0u : c_sent - c_first - c_inv, c_inv, gated ? c_sent : 0u};
            if (a.node_copies) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (x[c]) atomicAdd(&a.node_copies[(size_t)u * TRAFFIC_COLS + TR_FIRST + c], x[c]);
            }
            if (a.node_bytes && bytes) atomicAdd(&a.node_bytes[(size_t)u * 2 + 1], bytes);
        }
    }
    if (!a.msg_copies) return;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < wn * 64; i += TR_THREADS) {
        const uint32_t wi = i >> 6, b = i & 63u;
        const uint32_t k = (w0 + wi) * 64 + b;
        if (k >= ps.n_msgs) continue;
        const uint32_t* const tab = cnt + wi * TR_TAB * 64 + b;
        const uint32_t tot = tab[0], fr = tab[64], gr = tab[128];
        if (!tot) continue;
        const bool dropped = ps.drop && ((ps.drop[w0 + wi] >> b) & 1);
        uint32_t* const out = a.msg_copies + (size_t)k * TRAFFIC_COLS;
        atomicAdd(out + TR_SENT, tot);
        if (fr) atomicAdd(out + (dropped ? TR_INVALID : TR_FIRST), fr);
        if (tot - fr - gr) atomicAdd(out + TR_DUP, tot - fr - gr);
        if (gr) atomicAdd(out + TR_GRAY, gr);
    }
}

}  // namespace

// Zeroes the requested outputs, then the two passes.  Grid of the pair pass:
// x = word chunk, y = tile range, sized for about TR_BLOCKS blocks in all
// (8 per CU; not tuned): fewer blocks flush fewer message counters, more
// blocks hide more gather latency.
hipError_t launch_prop_traffic(const PropState& ps, const TrafficArgs& a, hipStream_t st) {
    static_assert(TR_FIRST + 1 == TR_DUP && TR_DUP + 1 == TR_INVALID && TR_INVALID + 1 == TR_GRAY,
                  "k_traffic_pairs keeps the receiver's classes in column order");
    if (ps.n_nodes == 0 || ps.n_msgs == 0 || ps.n_pairs == 0) return hipSuccess;
    const bool full = a.node_copies || a.node_bytes || a.pair_copies || a.pair_bytes;
    if (!full && !a.msg_copies) return hipSuccess;
    constexpr uint32_t target = TR_BLOCKS;
    const uint32_t words = (ps.n_msgs + 63) / 64;
    const uint32_t chunks = (words + TR_WC - 1) / TR_WC;
    const bool multi = chunks > 1;
    hipError_t rc = hipSuccess;
    auto zero = [&](void* p, size_t bytes) {
        if (p && rc == hipSuccess) rc = hipMemsetAsync(p, 0, bytes, st);
    };
    zero(a.msg_copies, 4 * (size_t)ps.n_msgs * TRAFFIC_COLS);
    zero(a.node_copies, 4 * (size_t)ps.n_nodes * TRAFFIC_COLS);
    zero(a.node_bytes, 8 * (size_t)ps.n_nodes * 2);
    if (multi) {  // (one chunk: every pair's counts are stored)
        zero(a.pair_copies, 4 * ps.n_pairs);
        zero(a.pair_bytes, 8 * ps.n_pairs);
    }
    if (rc != hipSuccess) return rc;
    const uint64_t cells = (uint64_t)ps.n_nodes * ps.n_words;
    hipLaunchKernelGGL(k_traffic_sendset, dim3((unsigned)std::min<uint64_t>((cells + 255) / 256, 16384)), dim3(256), 0,
                       st, ps, a.sset);
    const uint64_t n_tiles = (ps.n_pairs + 63) / 64;
    const uint64_t ranges =
        std::min<uint64_t>({std::max(target / chunks, 1u), (n_tiles + TR_WAVES - 1) / TR_WAVES, 65535u});  // (grid y)
    const uint32_t tiles_per_block = (uint32_t)((n_tiles + ranges - 1) / ranges);
    const dim3 grid(chunks, (unsigned)((n_tiles + tiles_per_block - 1) / tiles_per_block));
    if (full) hipLaunchKernelGGL(k_traffic_pairs<true>, grid, dim3(TR_THREADS), 0, st, ps, a, tiles_per_block, multi ? 1u : 0u);
    else hipLaunchKernelGGL(k_traffic_pairs<false>, grid, dim3(TR_THREADS), 0, st, ps, a, tiles_per_block, 0u);
    return hipGetLastError();
}

}  // namespace gsx
