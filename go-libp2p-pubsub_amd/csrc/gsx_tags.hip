// gsx_tags.hip — the tag tracer (tag_tracer.go) and a forced TrimOpenConns on
// the device.
//
// State (TagState, gsx_device.h): one u8 delivery tag per (pair, topic), tiled
// like rflag.  A tag byte is written by the lane that owns its pair (or, for
// events, its unique key) only: no atomics anywhere, every result is
// bit-identical from run to run.  Nothing here is floating point.
//
//   k_tag_events         one lane per (pair, topic) key of the call (the host
//                        merged equal keys): tag = min(cap, tag + add)
//   k_tag_decay          DecayFixed as one streaming pass: 16-byte loads, four
//                        bytes per register subtracted with saturation at once,
//                        a store only where a byte changed
//   k_tag_clear_unjoined Leave / un-joining subscriptions: the tags of topics
//                        the pair's observer has not joined become 0
//   k_tag_fold           one lane per pair: its first-deliverer row and its
//                        same-hop duplicates of the last propagation as two
//                        popcounts, one byte written
//   k_tag_export         tiled -> topic-major
//   k_conn_values        one lane per pair, 64 consecutive pairs per wave: per
//                        topic one 64-byte span of tags and one of record flags
//   k_conn_trim          per observer row: a threshold search over the value
//                        (<= 64 x 255), then an index-ordered prefix among the
//                        ties; one wave per row, one 1024-thread block per row
//                        above CONN_LONG_ROW pairs
#include "gsx_ops.h"

#include <algorithm>

namespace gsx {

namespace {

constexpr uint32_t T_THREADS = 256;

inline unsigned grid_for(uint64_t n, uint64_t cap = 8192) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + T_THREADS - 1) / T_THREADS, cap));
}

__device__ __forceinline__ uint8_t tag_add(uint8_t tag, uint32_t add, uint32_t cap) {
    const uint32_t s = (uint32_t)tag + add;  // (add <= cap <= 255)
    return (uint8_t)(s < cap ? s : cap);
}

// BumpSumBounded(0, cap), tag_tracer.go:115-119, 150
__global__ __launch_bounds__(T_THREADS) void k_tag_events(TagState t, const DevTagEvent* __restrict__ ev, uint32_t n) {
    const uint32_t i = blockIdx.x * T_THREADS + threadIdx.x;
    if (i >= n) return;
    const DevTagEvent e = ev[i];
    uint8_t* p = t.tags + flag_index(e.pair, e.topic, t.n_topics);
    *p = tag_add(*p, e.add, t.cap);
}

// The four bytes of x, each minus the same byte of y, saturating at 0.
__device__ __forceinline__ uint32_t sub_sat_u8x4(uint32_t x, uint32_t y) {
    constexpr uint32_t H = 0x80808080u;
    const uint32_t z = ((x | H) - (y & ~H)) ^ ((x ^ ~y) & H);  // bytewise x - y, no borrow across bytes
    const uint32_t b = ((~x & y) | (~(x ^ y) & z)) & H;        // bit 7 of a byte: its x < y
    return z & ~((b >> 7) * 0xFFu);
}

// DecayFixed(amount), tag_tracer.go:118, `steps` intervals at once
__global__ __launch_bounds__(T_THREADS) void k_tag_decay(uint4* __restrict__ tags, uint64_t n16, uint32_t y) {
    for (uint64_t i = (uint64_t)blockIdx.x * T_THREADS + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * T_THREADS) {
        const uint4 a = tags[i];
        if ((a.x | a.y | a.z | a.w) == 0) continue;  // (all sixteen are 0 and stay 0)
        tags[i] = uint4{sub_sat_u8x4(a.x, y), sub_sat_u8x4(a.y, y), sub_sat_u8x4(a.z, y), sub_sat_u8x4(a.w, y)};
    }
}

// removeDeliveryTag, tag_tracer.go:128-140
__global__ __launch_bounds__(T_THREADS) void k_tag_clear_unjoined(TagState t) {
    const uint64_t all = t.n_topics >= 64 ? ~0ull : ((1ull << t.n_topics) - 1);
    for (uint64_t q = (uint64_t)blockIdx.x * T_THREADS + threadIdx.x; q < t.n_pairs; q += (uint64_t)gridDim.x * T_THREADS) {
        for (uint64_t miss = ~t.sub[t.pair_obs[q]] & all; miss; miss &= miss - 1) {
            uint8_t* p = t.tags + flag_index(q, (uint32_t)__builtin_ctzll(miss), t.n_topics);
            if (*p) *p = 0;
        }
    }
}

__device__ __forceinline__ bool occ_at(const uint64_t* __restrict__ occ, uint32_t v) {
    return (occ[v / 64] >> (v % 64)) & 1;
}

// DeliverMessage, tag_tracer.go:187-199, for every ACCEPT message of the last
// propagation at once (gsx.h, gsx_tag_fold_prop).
__global__ __launch_bounds__(T_THREADS) void k_tag_fold(TagState t, PropState ps, const uint64_t* __restrict__ dup_rows,
                                                        const uint64_t* __restrict__ acc, uint32_t near) {
    const uint32_t W = ps.n_words;
    const size_t occ_row = ((size_t)ps.n_nodes + 63) / 64;
    const size_t plane = (size_t)ps.n_nodes * W;
    const uint32_t rows = ps.n_rows < (uint32_t)MAX_HOPS + 1 ? ps.n_rows : (uint32_t)MAX_HOPS + 1;
    for (uint64_t q = (uint64_t)blockIdx.x * T_THREADS + threadIdx.x; q < t.n_pairs; q += (uint64_t)gridDim.x * T_THREADS) {
        const uint32_t u = ps.pair_obs[q];
        if (!joined_node(t.sub, u, ps.topic)) continue;  // bumpDeliveryTag fails, :146-149
        uint32_t n = 0;
        for (uint32_t w = 0; w < W; ++w) n += (uint32_t)__popcll(ps.from_mask[q * W + w] & acc[w]);
        if (near) {
            const uint32_t v = (uint32_t)ps.col[q];
            uint64_t hm = 0;  // bit h - 1: v forwarded something at hop h - 1 and u received something new at hop h
            for (uint32_t h = 1; h < rows; ++h)
                if (occ_at(ps.occ + (size_t)(h - 1) * occ_row, v) && occ_at(ps.occ + (size_t)h * occ_row, u))
                    hm |= 1ull << (h - 1);
            if (hm)
                for (uint32_t w = 0; w < W; ++w) {
                    const uint64_t d = dup_rows[q * W + w] & acc[w];
                    if (!d) continue;
                    uint64_t same = 0;
                    for (uint64_t m = hm; m; m &= m - 1) {
                        const uint32_t h = (uint32_t)__builtin_ctzll(m) + 1;
                        same |= ps.hist[(size_t)(h - 1) * plane + (size_t)v * W + w] &
                                ps.hist[(size_t)h * plane + (size_t)u * W + w];
                    }
                    n += (uint32_t)__popcll(d & same);
                }
        }
        if (!n) continue;
        const uint64_t prod = (uint64_t)n * t.bump;
        const uint64_t add = prod < t.cap ? prod : t.cap;
        uint8_t* p = t.tags + flag_index(q, ps.topic, t.n_topics);
        *p = tag_add(*p, (uint32_t)add, t.cap);
    }
}

__global__ __launch_bounds__(T_THREADS) void k_tag_export(TagState t, uint8_t* __restrict__ out) {
    for (uint64_t q = (uint64_t)blockIdx.x * T_THREADS + threadIdx.x; q < t.n_pairs; q += (uint64_t)gridDim.x * T_THREADS)
        for (uint32_t k = 0; k < t.n_topics; ++k) out[(size_t)k * t.n_pairs + q] = t.tags[flag_index(q, k, t.n_topics)];
}

// GetTagInfo(p).Value from this tracer's decaying tags; IsProtected for
// pubsub:<direct> (tag_tracer.go:81-91) and any pubsub:<topic> (:93-101).
__global__ __launch_bounds__(T_THREADS) void k_conn_values(TagState t, uint32_t* __restrict__ value,
                                                           uint8_t* __restrict__ protect, uint32_t* __restrict__ key) {
    for (uint64_t q = (uint64_t)blockIdx.x * T_THREADS + threadIdx.x; q < t.n_pairs; q += (uint64_t)gridDim.x * T_THREADS) {
        const uint8_t pf = t.pflags[q];
        uint32_t val = 0;
        uint8_t pr = 0;
        if (pf & PAIR_PRESENT) {
            const size_t base = flag_index(q, 0, t.n_topics);
            uint8_t mesh = 0;
            for (uint32_t k = 0; k < t.n_topics; ++k) {
                val += t.tags[base + (size_t)k * TILE];
                mesh |= t.rflags[base + (size_t)k * TILE];
            }
            pr = (uint8_t)(((t.eflags[q] & EDGE_DIRECT) ? CONN_DIRECT : 0) | ((mesh & REC_IN_MESH) ? CONN_MESH : 0));
        }
        if (value) value[q] = val;
        if (protect) protect[q] = pr;
        if (key) key[q] = ((pf & (PAIR_PRESENT | PAIR_CONNECTED)) != (PAIR_PRESENT | PAIR_CONNECTED)) ? CONN_KEY_OUT
                          : pr                                                                      ? CONN_KEY_PROT
                                                                                                    : val;
    }
}

// Sum of a per-lane count over the NW waves that share a row.  Every lane of
// the NW waves calls it (NW > 1: one block, two barriers).
template <int NW>
__device__ __forceinline__ uint32_t row_sum(uint32_t c, uint32_t* lds) {
#pragma unroll
    for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o, 64);
    if (NW == 1) return c;
    __syncthreads();  // (the last call's reads are done)
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = c;
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += lds[w];
    return s;
}

// One row b .. en of keys by NW waves (lane g of NW * 64).
template <int NW>
__device__ void trim_row(const uint32_t* __restrict__ key, int64_t b, int64_t en, uint32_t low_water,
                         uint8_t* __restrict__ trim, uint32_t* __restrict__ n_out, uint32_t* lds) {
    constexpr uint32_t GS = NW * 64;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t g = NW == 1 ? lane : threadIdx.x;
    auto count_le = [&](uint32_t thr) {
        uint32_t c = 0;
        for (int64_t i = b + g; i < en; i += GS) c += key[i] <= thr ? 1u : 0u;
        return row_sum<NW>(c, lds);
    };
    const uint32_t conns = count_le(CONN_KEY_PROT), unprot = count_le(CONN_VALUE_MAX);
    const uint32_t over = conns > low_water ? conns - low_water : 0u;
    const uint32_t k = over < unprot ? over : unprot;
    uint32_t thr = 0, need = 0;
    if (k) {  // the smallest value with at least k unprotected pairs at or below it
        uint32_t lo = 0, hi = CONN_VALUE_MAX;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) / 2;
            if (count_le(mid) >= k) hi = mid;
            else lo = mid + 1;
        }
        thr = lo;
        need = k - (thr ? count_le(thr - 1) : 0u);  // pairs to take among the ties, by index
    }
    uint32_t run = 0;  // ties before this chunk
    for (int64_t c0 = b; c0 < en; c0 += GS) {
        const int64_t i = c0 + g;
        const uint32_t kv = i < en ? key[i] : CONN_KEY_OUT;
        const bool tie = k && kv == thr;
        const unsigned long long bal = __ballot(tie);
        uint32_t before = run + (uint32_t)__popcll(bal & ((1ull << lane) - 1));
        uint32_t total = (uint32_t)__popcll(bal);
        if (NW > 1) {
            __syncthreads();
            if (lane == 0) lds[threadIdx.x >> 6] = total;
            __syncthreads();
            total = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const uint32_t x = lds[w];
                if ((uint32_t)w < (threadIdx.x >> 6)) before += x;
                total += x;
            }
        }
        if (i < en) trim[i] = (k && (kv < thr || (tie && before < need))) ? 1 : 0;
        run += total;
    }
    if (g == 0) n_out[0] = k;
}

__global__ __launch_bounds__(T_THREADS) void k_conn_trim(const int64_t* __restrict__ row_ptr, uint32_t n_nodes,
                                                         const uint32_t* __restrict__ key, uint32_t low_water,
                                                         uint8_t* __restrict__ trim, uint32_t* __restrict__ node_trimmed) {
    const uint32_t waves = gridDim.x * (T_THREADS / 64);
    for (uint32_t u = blockIdx.x * (T_THREADS / 64) + threadIdx.x / 64; u < n_nodes; u += waves) {
        const int64_t b = row_ptr[u], en = row_ptr[u + 1];
        if (en - b > (int64_t)CONN_LONG_ROW) continue;  // k_conn_trim_long's
        trim_row<1>(key, b, en, low_water, trim, node_trimmed + u, nullptr);
    }
}

__global__ __launch_bounds__(1024) void k_conn_trim_long(const int64_t* __restrict__ row_ptr,
                                                         const uint32_t* __restrict__ long_rows, uint32_t n_long,
                                                         const uint32_t* __restrict__ key, uint32_t low_water,
                                                         uint8_t* __restrict__ trim, uint32_t* __restrict__ node_trimmed) {
    __shared__ uint32_t lds[16];
    for (uint32_t j = blockIdx.x; j < n_long; j += gridDim.x) {
        const uint32_t u = long_rows[j];
        trim_row<16>(key, row_ptr[u], row_ptr[u + 1], low_water, trim, node_trimmed + u, lds);
    }
}

}  // namespace

hipError_t launch_tag_events(const TagState& t, const DevTagEvent* ev, uint32_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_tag_events, dim3((n + T_THREADS - 1) / T_THREADS), dim3(T_THREADS), 0, st, t, ev, n);
    return hipGetLastError();
}

hipError_t launch_tag_decay(const TagState& t, uint32_t sub, hipStream_t st) {
    const uint64_t n16 = t.n_tiles * t.n_topics * TILE / 16;  // (whole tiles: a multiple of 64 bytes)
    if (n16 == 0 || sub == 0) return hipSuccess;
    hipLaunchKernelGGL(k_tag_decay, dim3(grid_for(n16)), dim3(T_THREADS), 0, st, reinterpret_cast<uint4*>(t.tags), n16,
                       std::min(sub, 255u) * 0x01010101u);
    return hipGetLastError();
}

hipError_t launch_tag_clear_unjoined(const TagState& t, hipStream_t st) {
    if (t.n_pairs == 0 || !t.sub) return hipSuccess;
    hipLaunchKernelGGL(k_tag_clear_unjoined, dim3(grid_for(t.n_pairs)), dim3(T_THREADS), 0, st, t);
    return hipGetLastError();
}

hipError_t launch_tag_fold(const TagState& t, const PropState& ps, const uint64_t* dup_rows, const uint64_t* acc,
                           uint32_t near, hipStream_t st) {
    if (t.n_pairs == 0 || ps.n_words == 0) return hipSuccess;
    hipLaunchKernelGGL(k_tag_fold, dim3(grid_for(t.n_pairs)), dim3(T_THREADS), 0, st, t, ps, dup_rows, acc, near);
    return hipGetLastError();
}

hipError_t launch_tag_export(const TagState& t, uint8_t* out, hipStream_t st) {
    if (t.n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_tag_export, dim3(grid_for(t.n_pairs)), dim3(T_THREADS), 0, st, t, out);
    return hipGetLastError();
}

hipError_t launch_conn_values(const TagState& t, uint32_t* value, uint8_t* protect, uint32_t* key, hipStream_t st) {
    if (t.n_pairs == 0 || (!value && !protect && !key)) return hipSuccess;
    hipLaunchKernelGGL(k_conn_values, dim3(grid_for(t.n_pairs)), dim3(T_THREADS), 0, st, t, value, protect, key);
    return hipGetLastError();
}

hipError_t launch_conn_trim(const TagState& t, const int64_t* row_ptr, const uint32_t* key, uint32_t low_water,
                            const uint32_t* long_rows, uint32_t n_long, uint8_t* trim, uint32_t* node_trimmed,
                            hipStream_t st) {
    if (t.n_nodes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_conn_trim, dim3(grid_for((uint64_t)t.n_nodes * 64)), dim3(T_THREADS), 0, st, row_ptr, t.n_nodes,
                       key, low_water, trim, node_trimmed);
    if (hipError_t rc = hipGetLastError()) return rc;
    if (n_long) {
        hipLaunchKernelGGL(k_conn_trim_long, dim3(std::min(n_long, 1024u)), dim3(1024), 0, st, row_ptr, long_rows, n_long,
                           key, low_water, trim, node_trimmed);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace gsx
