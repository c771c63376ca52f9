// gsx_mesh_stats.hip — the shape of the mesh (gsx_mesh_stats), reduced on the
// device: per topic the mesh links and what they are (outbound, one-sided,
// negative, active, by age, by class pair), the backoff entries and the fanout,
// the degree / outbound degree / in-degree of every (topic, node), and the
// units (joined (node, topic)) per degree bin and per heartbeat verdict (below
// Dlo, above Dhi, below Dout, eclipsed ...), without a record leaving HBM.
//
// Pass 1, k_mesh_pairs: a wave per 64-pair tile, grid-stride over a bounded
// grid, looping the topics.  Per tile, once: the pair flags, edge flags,
// observers, peers, reverse indices (contiguous spans), the fanout words and
// the two class bytes when asked.  Per (tile, topic): the 64 record flags, one
// contiguous 64-byte span (flag_index), and one backoff presence byte per pair
// and eight topics.  Gathers only for mesh links: the reverse pair's two flag
// bytes, the score (8 B, once per pair), the graft time (8 B, age_hist only).
// A (tile, topic) with no mesh link, backoff entry or fanout bit costs its flag
// load and one ballot.  How it accumulates (all integer adds: bit-identical
// from run to run, whatever the grid):
//   * the eight link totals: one ballot each, their popcounts added by eight
//     lanes to a per-block LDS table; age bins and class pairs: one ds_add per
//     mesh link to the same table; then ONE no-return global atomic per block
//     and non-zero counter;
//   * degree, outbound degree, honest degree, class degrees per (topic, node):
//     k_score_stats's segmented runs.  A row's pairs are contiguous, so the
//     lanes of a wave that share pair_obs form a run; the ballot masked to the
//     run, popcount taken by the run's first lane.  A run that neither began in
//     the wave before nor goes on in the wave after is the whole row: a plain
//     store (the outputs start zeroed); only rows cut by a wave's edge add with
//     an atomic, so a hub row of thousands of pairs costs one atomic per wave;
//   * in-degree: the targets col[p] are scattered: one no-return u32 atomic per
//     mesh link;
//   * the topics with a fanout link in a row: OR-ed over the run the same way.
// Pass 2, k_mesh_units: a lane per (topic, node), blockIdx.y the topic.  Reads
// the node tables pass 1 left, bins the units into the three histograms (a
// ds_add per unit) and the verdict columns (a ballot each), per-block LDS
// table, then one global atomic per block and non-zero counter.
// No floating-point arithmetic but `score < 0`.
#include "gsx_ops.h"

#include <algorithm>

namespace gsx {

namespace {

constexpr uint32_t MS_THREADS = 256, MS_WAVES = MS_THREADS / 64;
// Pass 1's ballot counters are, in order, LINKS, OUTBOUND, ONE_SIDED, NEGATIVE,
// ACTIVE, FANOUT_LINKS, BACKOFF, BACKOFF_EXPIRED; pass 2's UNITS, EMPTY,
// BELOW_DLO, ABOVE_DHI, BELOW_DOUT, FANOUT_UNITS, ECLIPSED, BELOW_HONEST: the
// column of counter k is nibble k of these.
constexpr uint32_t MS_LINK_CTRS = 8, MS_UNIT_CTRS = 8;
constexpr uint32_t MS_LINK_COLS = 0xDCB98765u, MS_UNIT_COLS = 0xFEA43210u;
static_assert(MS_LINKS == 5 && MS_OUTBOUND == 6 && MS_ONE_SIDED == 7 && MS_NEGATIVE == 8 && MS_ACTIVE == 9 &&
                  MS_FANOUT_LINKS == 11 && MS_BACKOFF == 12 && MS_BACKOFF_EXPIRED == 13 && MS_UNITS == 0 &&
                  MS_EMPTY == 1 && MS_BELOW_DLO == 2 && MS_ABOVE_DHI == 3 && MS_BELOW_DOUT == 4 &&
                  MS_FANOUT_UNITS == 10 && MS_ECLIPSED == 14 && MS_BELOW_HONEST == 15,
              "the nibbles above are the columns");

// lane k < 8 gets popcount(b[k]): the eight counts of a wave as one vector
__device__ __forceinline__ uint32_t lane_count8(const uint64_t (&b)[8], uint32_t lane) {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) c = lane == k ? (uint32_t)__popcll(b[k]) : c;
    return c;
}

// LDS table of pass 1: [topic][MS_LINK_CTRS | n_age_edges + 1 | C * C]
__global__ __launch_bounds__(MS_THREADS) void k_mesh_pairs(MeshStatsArgs a) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t T = a.n_topics, N = a.n_nodes, C = a.n_classes;
    const uint32_t nab = a.age_hist ? a.n_age_edges + 1 : 0, ncc = a.class_links ? C * C : 0;
    const uint32_t stride = MS_LINK_CTRS + nab + ncc;
    const bool node_view = a.node_deg || a.node_out || a.node_honest || a.node_class_deg || a.fan_any;
    for (uint32_t i = threadIdx.x; i < T * stride; i += MS_THREADS) lds[i] = 0;
    __syncthreads();

    // (base is wave-uniform: a wave's lanes stay in the loop together)
    for (uint64_t base = ((uint64_t)blockIdx.x * MS_WAVES + wave) * 64; base < a.n_pairs;
         base += (uint64_t)gridDim.x * MS_THREADS) {
        const uint64_t p = base + lane;
        const bool valid = p < a.n_pairs;
        const uint64_t wtile = wave_uniform(base / TILE);
        const uint8_t pf = valid ? a.pflags[p] : (uint8_t)0;
        const bool pc = (pf & (PAIR_PRESENT | PAIR_CONNECTED)) == (PAIR_PRESENT | PAIR_CONNECTED);
        const bool outbound = valid && (a.eflags[p] & EDGE_OUTBOUND);
        uint32_t obs = 0xFFFFFFFFu, v = 0, q = NO_PAIR;
        uint64_t fan = 0;
        if (valid) {
            obs = a.pair_obs[p];
            v = (uint32_t)a.col[p];
            if (a.rev) q = a.rev[p];
            if (a.fanout) fan = a.fanout[p];
        }
        // the reverse pair stands (exists, present and connected): its mesh bit is read per topic
        bool rev_ok = false;
        if (a.rev && pc && q < a.n_pairs)
            rev_ok = (a.pflags[q] & (PAIR_PRESENT | PAIR_CONNECTED)) == (PAIR_PRESENT | PAIR_CONNECTED);
        uint32_t cu = 0, cv = 0;
        bool honest = false;
        if (a.node_class && pc) {
            cu = min((uint32_t)a.node_class[obs], C - 1);
            cv = min((uint32_t)a.node_class[v], C - 1);
            honest = !((a.hostile_mask >> cv) & 1u);
        }

        // the run of lanes that share this lane's observer (k_score_stats)
        bool head = false, shared = false;
        uint64_t run = 0;
        if (node_view) {
            const uint32_t prev = (uint32_t)__shfl_up((int)obs, 1, 64);
            head = lane == 0 || prev != obs;
            const uint64_t heads = __ballot(head);
            const uint64_t above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
            const uint32_t next = above ? (uint32_t)__builtin_ctzll(above) : 64u;
            run = (next == 64 ? ~0ull : (1ull << next) - 1) & (~0ull << lane);  // (a head lane's: the whole run)
            // the row goes on beyond this wave's pairs: its other segments add to the same counters
            const bool lo = lane == 0 && valid && p > 0 && a.pair_obs[p - 1] == obs;
            const bool hi = lane == 63 && p + 1 < a.n_pairs && a.pair_obs[p + 1] == obs;
            const uint64_t cl = __ballot(lo), ch = __ballot(hi);
            shared = (lane == 0 && cl != 0) || (next == 64 && ch != 0);
            head = head && valid;
        }
        auto row_add = [&](uint32_t* dst, uint32_t c) {
            if (!c) return;
            if (shared) atomicAdd(dst, c);
            else *dst = c;
        };

        const uint8_t* const ftile = a.rflags + wtile * (uint64_t)T * TILE + lane;
        double sc = 0.0;
        bool have_sc = false;
        uint32_t bo = 0;
        uint64_t fbits = 0;  // (a head lane's) the topics with a fanout link in its run
        for (uint32_t t = 0; t < T; ++t) {
            const uint8_t fl = valid ? ftile[(size_t)t * TILE] : (uint8_t)0;
            const bool mesh = pc && (fl & REC_IN_MESH);
            if ((t & 7u) == 0) bo = (a.bo8 && valid) ? a.bo8[(size_t)(t >> 3) * a.n_pairs + p] : 0u;
            const bool bop = (bo >> (t & 7u)) & 1u, fbit = (fan >> t) & 1ull;
            uint64_t b[8];
            b[0] = __ballot(mesh);
            if (b[0] == 0 && __ballot(bop || fbit) == 0) continue;  // (wave-uniform)
            uint32_t* const tab = lds + t * stride;

            bool one = false, neg = false;
            if (mesh) {
                if (a.rev) one = !(rev_ok && (a.rflags[flag_index(q, t, T)] & REC_IN_MESH));
                if (a.score) {
                    if (!have_sc) {
                        sc = a.score[p];
                        have_sc = true;
                    }
                    neg = sc < 0.0;  // a NaN is not below 0
                }
                if (nab) {
                    const int64_t graft = reinterpret_cast<const int64_t*>(a.rec)[rec_index(p, t, T, GRAFT)];
                    const int64_t age = (int64_t)((uint64_t)a.now - (uint64_t)graft);
                    uint32_t bin = 0;
#pragma unroll
                    for (uint32_t k = 0; k < MS_MAX_AGE_EDGES; ++k)
                        bin += (k < a.n_age_edges && !(age < a.age_edges[k])) ? 1u : 0u;
                    atomicAdd(&tab[MS_LINK_CTRS + bin], 1u);
                }
                if (ncc) atomicAdd(&tab[MS_LINK_CTRS + nab + cu * C + cv], 1u);
                if (a.node_in) atomicAdd(a.node_in + (size_t)t * N + v, 1u);
            }
            const bool live = bop && a.backoff[(size_t)t * a.n_pairs + p] > a.now;
            b[1] = __ballot(mesh && outbound);
            b[2] = __ballot(one);
            b[3] = __ballot(neg);
            b[4] = __ballot(mesh && (fl & REC_ACTIVE));
            b[5] = __ballot(fbit);
            b[6] = __ballot(live);
            b[7] = __ballot(bop && !live);
            const uint32_t c8 = lane_count8(b, lane);
            if (lane < MS_LINK_CTRS && c8) atomicAdd(&tab[lane], c8);

            if (node_view) {
                const uint64_t hb = a.node_honest ? __ballot(mesh && honest) : 0ull;
                const size_t at = (size_t)t * N + obs;
                if (head) {
                    if (a.node_deg) row_add(a.node_deg + at, (uint32_t)__popcll(b[0] & run));
                    if (a.node_out) row_add(a.node_out + at, (uint32_t)__popcll(b[1] & run));
                    if (a.node_honest) row_add(a.node_honest + at, (uint32_t)__popcll(hb & run));
                    if (b[5] & run) fbits |= 1ull << t;
                }
                if (a.node_class_deg)
                    for (uint32_t c = 0; c < C; ++c) {
                        const uint64_t cb = __ballot(mesh && cv == c);
                        if (head) row_add(a.node_class_deg + at * C + c, (uint32_t)__popcll(cb & run));
                    }
            }
        }
        if (a.fan_any && head && fbits) {
            if (shared) atomicOr(a.fan_any + obs, (unsigned long long)fbits);
            else a.fan_any[obs] = fbits;
        }
    }

    __syncthreads();
    for (uint32_t i = threadIdx.x; i < T * stride; i += MS_THREADS) {
        const uint32_t c = lds[i];
        if (!c) continue;
        const uint32_t t = i / stride, k = i % stride;
        if (k < MS_LINK_CTRS) {
            if (a.tot) atomicAdd(a.tot + (size_t)t * MS_COLS + ((MS_LINK_COLS >> (4 * k)) & 15u), (unsigned long long)c);
        } else if (k < MS_LINK_CTRS + nab) {
            atomicAdd(a.age_hist + (size_t)t * nab + (k - MS_LINK_CTRS), (unsigned long long)c);
        } else {
            atomicAdd(a.class_links + (size_t)t * ncc + (k - MS_LINK_CTRS - nab), (unsigned long long)c);
        }
    }
}

__global__ __launch_bounds__(MS_THREADS) void k_mesh_units(MeshStatsArgs a) {
    __shared__ uint32_t hist[3][MS_MAX_BINS];
    __shared__ uint32_t ver[MS_UNIT_CTRS];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t = blockIdx.y, N = a.n_nodes, top = a.n_bins - 1;
    for (uint32_t i = threadIdx.x; i < 3 * MS_MAX_BINS; i += MS_THREADS) (&hist[0][0])[i] = 0;
    if (threadIdx.x < MS_UNIT_CTRS) ver[threadIdx.x] = 0;
    __syncthreads();

    // (base is block-uniform: every lane stays in the loop for the ballots)
    for (uint64_t base = (uint64_t)blockIdx.x * MS_THREADS; base < N; base += (uint64_t)gridDim.x * MS_THREADS) {
        const uint64_t u = base + threadIdx.x;
        const bool valid = u < N;
        const size_t at = (size_t)t * N + u;
        const bool unit = valid && joined_node(a.sub, (uint32_t)u, t);
        uint32_t deg = 0, out = 0, in = 0, hon = 0;
        bool fanu = false, good = false;
        if (valid) {
            if (a.node_deg) deg = a.node_deg[at];
            if (a.node_out) out = a.node_out[at];
            if (a.node_in) in = a.node_in[at];
            if (a.fan_any) fanu = (a.fan_any[u] >> t) & 1ull;
            if (a.node_class && a.node_honest) {  // the verdicts of a node that is not hostile itself
                hon = a.node_honest[at];
                good = !((a.hostile_mask >> min((uint32_t)a.node_class[u], a.n_classes - 1)) & 1u);
            }
        }
        if (unit) {
            if (a.deg_hist) atomicAdd(&hist[0][min(deg, top)], 1u);
            if (a.out_hist) atomicAdd(&hist[1][min(out, top)], 1u);
            if (a.in_hist) atomicAdd(&hist[2][min(in, top)], 1u);
        }
        if (a.tot) {
            uint64_t b[8];
            b[0] = __ballot(unit);
            b[1] = __ballot(unit && deg == 0);
            b[2] = __ballot(unit && (int64_t)deg < (int64_t)a.d_lo);
            b[3] = __ballot(unit && (int64_t)deg > (int64_t)a.d_hi);
            b[4] = __ballot(unit && (int64_t)out < (int64_t)a.d_out);
            b[5] = __ballot(fanu);
            b[6] = __ballot(unit && good && deg >= 1 && hon == 0);
            b[7] = __ballot(unit && good && hon < a.min_honest);
            const uint32_t c8 = lane_count8(b, lane);
            if (lane < MS_UNIT_CTRS && c8) atomicAdd(&ver[lane], c8);
        }
    }

    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 3 * MS_MAX_BINS; i += MS_THREADS) {
        const uint32_t c = (&hist[0][0])[i], h = i / MS_MAX_BINS, k = i % MS_MAX_BINS;
        if (!c) continue;  // (only bins < n_bins of a histogram that was asked for were added to)
        unsigned long long* const dst = h == 0 ? a.deg_hist : h == 1 ? a.out_hist : a.in_hist;
        atomicAdd(dst + (size_t)t * a.n_bins + k, (unsigned long long)c);
    }
    if (a.tot && threadIdx.x < MS_UNIT_CTRS)
        if (const uint32_t c = ver[threadIdx.x])
            atomicAdd(a.tot + (size_t)t * MS_COLS + ((MS_UNIT_COLS >> (4 * threadIdx.x)) & 15u), (unsigned long long)c);
}

}  // namespace

// Everything is added to: the caller zeroes the outputs and the scratch first.
hipError_t launch_mesh_pairs(const MeshStatsArgs& a, hipStream_t st) {
    if (a.n_pairs == 0 || a.n_topics == 0) return hipSuccess;
    const uint32_t stride = MS_LINK_CTRS + (a.age_hist ? a.n_age_edges + 1 : 0) + (a.class_links ? a.n_classes * a.n_classes : 0);
    const size_t lds = sizeof(uint32_t) * a.n_topics * stride;  // <= 64 * (8 + 9 + 64) * 4 B
    const dim3 grid((uint32_t)std::min<uint64_t>((a.n_pairs + MS_THREADS - 1) / MS_THREADS, COUNTER_GRID)), block(MS_THREADS);
    hipLaunchKernelGGL(k_mesh_pairs, grid, block, lds, st, a);
    return hipGetLastError();
}

hipError_t launch_mesh_units(const MeshStatsArgs& a, hipStream_t st) {
    if (a.n_nodes == 0 || a.n_topics == 0) return hipSuccess;
    const uint32_t bx = (uint32_t)std::min<uint64_t>(((uint64_t)a.n_nodes + MS_THREADS - 1) / MS_THREADS,
                                                     std::max(COUNTER_GRID / a.n_topics, 1u));
    hipLaunchKernelGGL(k_mesh_units, dim3(bx, a.n_topics), dim3(MS_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace gsx
