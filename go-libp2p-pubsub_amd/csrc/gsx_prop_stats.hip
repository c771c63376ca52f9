// gsx_prop_stats.hip — per-message and per-node summaries of the last
// propagation call (gsx_prop_stats), reduced on the device from the frontier
// history hist[hop][node][word], its occupancy bits and the dseen rows of
// dropped messages: the state k_prop_hops_export turns into [message][node]
// hop bytes, here counted without ever writing those bytes.
//
// It is a column popcount of a bit matrix.  A wave takes a tile of 64 nodes of
// one message word: lane l holds node l's 64 message bits of one hop row, a
// 6-step butterfly transposes the 64 x 64 bits across the wave, and lane b's
// popcount is the number of the tile's nodes that got message b at that hop
// (64 ballot-and-popcount steps instead of the transpose measured 19 % slower
// on 1M peers x 64 messages and 6 % faster on 1M x 1024, where the strided
// gather of the node-major rows is the bound, not the count: DESIGN.md).
// The counts go to a per-block LDS table [hop][message of the word] (65 x 64
// u32); a block owns one word and a range of tiles and flushes its non-zero
// counters with one global atomic add each.  Integer adds commute: the result
// does not depend on the schedule.
#include "gsx_device.h"
#include "gsx_wave.h"

#include <algorithm>
#include <cstdlib>

namespace gsx {

namespace {

constexpr uint32_t ST_THREADS = 256, ST_WAVES = ST_THREADS / 64;
constexpr uint32_t ST_BATCH = 4;  // history rows a wave loads before it reduces them

// (wave_transpose64, read_lane64: gsx_wave.h)

// hop(k, u) is k_prop_hops_export's: a history row counts only under the
// node's occupancy bit, rows 0 .. n_rows - 1 (row GSX_MAX_HOPS included), a
// later row wins over an earlier one, the messages of a word with drop[w]
// count at hop 1 from dseen whatever the rows say, the bits of the last word
// at or beyond n_msgs are ignored.  The rows are walked from the last hop
// down with the bits already counted masked out, which is "the later row
// wins".
__global__ __launch_bounds__(ST_THREADS) void k_prop_stats(PropState ps, uint32_t tiles_per_block,
                                                           uint32_t* __restrict__ msg_hop_hist,
                                                           uint32_t* __restrict__ node_received,
                                                           unsigned long long* __restrict__ node_hop_sum) {
    __shared__ uint32_t cnt[PROP_STATS_HOPS * 64];  // [hop][message of the word]
    const uint32_t w = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < PROP_STATS_HOPS * 64; i += ST_THREADS) cnt[i] = 0;
    __syncthreads();
    const uint32_t W = ps.n_words, n = ps.n_nodes;
    const uint32_t n_tiles = (n + 63) / 64;
    const size_t occ_row = n_tiles;  // an occupancy row: one aligned word per tile
    const size_t plane = (size_t)n * W;
    const uint32_t rows = ps.n_rows < PROP_STATS_HOPS ? ps.n_rows : PROP_STATS_HOPS;
    const uint32_t left = ps.n_msgs - w * 64;  // (w < ceil(n_msgs / 64): the launcher's grid)
    const uint64_t valid = left >= 64 ? ~0ull : ((1ull << left) - 1);
    const bool dropw = ps.drop && ps.drop[w] != 0;
    const uint32_t t_end = min(n_tiles, (blockIdx.y + 1) * tiles_per_block);
    for (uint32_t t = blockIdx.y * tiles_per_block + wave; t < t_end; t += ST_WAVES) {
        const uint32_t u = t * 64 + lane;
        const bool in = u < n;
        const size_t cell = (size_t)u * W + w;
        // lane h: the tile's occupancy word of hop h (row 64 apart); one test skips an empty row
        const uint64_t oc = lane < rows ? ps.occ[(size_t)lane * occ_row + t] : 0ull;
        const uint64_t oc64 = rows > 64 ? ps.occ[(size_t)64 * occ_row + t] : 0ull;
        uint64_t hm = __ballot(oc != 0);
        uint64_t got = 0;       // this node's messages counted so far
        uint32_t nr = 0, ns = 0;  // this node: receipts at hops 1 .. 64 of the word, their hop sum
        auto tally = [&](uint32_t h, uint64_t x) {
            x &= valid & ~got;
            got |= x;
            const uint32_t p = (uint32_t)__popcll(x);
            if (h) {
                nr += p;
                ns += h * p;
            }
            const uint32_t c = (uint32_t)__popcll(wave_transpose64(x, lane));
            if (c) atomicAdd(&cnt[h * 64 + lane], c);
        };
        if (dropw) tally(1, in ? ps.dseen[cell] : 0ull);
        if (oc64) tally(64, (in && ((oc64 >> lane) & 1)) ? ps.hist[(size_t)64 * plane + cell] : 0ull);
        while (hm) {
            uint32_t hs[ST_BATCH];
            uint64_t x[ST_BATCH];
#pragma unroll
            for (uint32_t j = 0; j < ST_BATCH; ++j) {
                hs[j] = hm ? 63u - (uint32_t)__builtin_clzll(hm) : ~0u;
                if (hm) hm &= ~(1ull << hs[j]);
            }
#pragma unroll
            for (uint32_t j = 0; j < ST_BATCH; ++j) {
                x[j] = 0;
                if (hs[j] != ~0u) {
                    const uint64_t ow = read_lane64(oc, hs[j]);
                    if (in && ((ow >> lane) & 1)) x[j] = ps.hist[(size_t)hs[j] * plane + cell];
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < ST_BATCH; ++j)
                if (hs[j] != ~0u) tally(hs[j], x[j]);
        }
        if (in && nr) {
            if (node_received) atomicAdd(&node_received[u], nr);
            if (node_hop_sum) atomicAdd(&node_hop_sum[u], (unsigned long long)ns);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < rows * 64; i += ST_THREADS) {
        const uint32_t c = cnt[i];
        const uint32_t k = w * 64 + (i & 63u);
        if (c && k < ps.n_msgs) atomicAdd(&msg_hop_hist[(size_t)k * PROP_STATS_HOPS + (i >> 6)], c);
    }
}

}  // namespace

// The outputs are added to: the caller zeroes them first.  Grid: x = word
// (neighbouring blocks read the same cache lines of the node-major rows), y =
// tile range.  The tile ranges are sized for about GSX_STATS_BLOCKS blocks in
// all (A/B; default 1024): fewer blocks flush fewer counters, more blocks hide
// more load latency.
hipError_t launch_prop_stats(const PropState& ps, uint32_t* msg_hop_hist, uint32_t* node_received,
                             unsigned long long* node_hop_sum, hipStream_t st) {
    if (ps.n_nodes == 0 || ps.n_msgs == 0) return hipSuccess;
    static const uint32_t target = [] {
        const char* v = getenv("GSX_STATS_BLOCKS");
        return v && atoi(v) > 0 ? (uint32_t)atoi(v) : 1024u;
    }();
    const uint32_t words = (ps.n_msgs + 63) / 64;  // (n_words may be padded: the padding holds no message)
    const uint32_t n_tiles = (ps.n_nodes + 63) / 64;
    const uint32_t ranges =
        std::min({std::max(target / words, 1u), (n_tiles + ST_WAVES - 1) / ST_WAVES, 65535u});  // (grid y)
    const uint32_t tiles_per_block = (n_tiles + ranges - 1) / ranges;
    const uint32_t gy = (n_tiles + tiles_per_block - 1) / tiles_per_block;
    hipLaunchKernelGGL(k_prop_stats, dim3(words, gy), dim3(ST_THREADS), 0, st, ps, tiles_per_block, msg_hop_hist,
                       node_received, node_hop_sum);
    return hipGetLastError();
}

}  // namespace gsx
