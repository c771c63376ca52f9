// gsx_gater.hip — the peer gater (peer_gater.go) and the whole
// GossipSubRouter.AcceptFrom (gossipsub.go:583-594) on the device.
//
// State (GaterState, gsx_device.h): validate / throttle / last_throttle per
// observer; connected, expire and the four counters (one 32-byte record) per
// (observer, IP) group; the bound group per pair.  A group belongs to one
// observer, and only that observer's events, decay lane and fold lane write
// it: no floating-point atomic anywhere, every result is bit-identical from
// run to run.
//
//   k_gater_events      one lane per observer, its events in the given order
//   k_gater_decay       grid-stride over the groups, then over the observers
//   k_gater_hot         the per-observer `hot` byte of one AcceptFrom call
//   k_accept_from       64 consecutive pairs per wave: edge flags (1 B), score
//                       (8 B), pair flags (1 B) and the observer (4 B) as the
//                       wave's contiguous spans; a lane of a cold observer
//                       stops there, so a wave whose rows are all cold gathers
//                       nothing.  A hot lane reads its bound group (4 B) and
//                       gathers the group's 32-byte record, then one hash,
//                       three multiplies, five adds and one IEEE division.
//   k_gater_fold_count  the last propagation's rows as integer counts per
//                       group and per observer (u32 atomics)
//   k_gater_fold_apply  one lane per group / observer applies them
//
// Numerics: built with -ffp-contract=off; `total` is evaluated left to right
// with separate multiplies and adds as the Go source's expression is; the two
// divisions are plain binary64 `/` (v_div_scale / v_div_fmas / v_div_fixup
// sequences, correctly rounded), no reciprocal shortcut.
#include "gsx_ops.h"

#include <algorithm>

namespace gsx {

namespace {

constexpr uint32_t G_THREADS = 256;

__device__ __forceinline__ double decay_to_zero(double x, double decay, double dtz) {
    x *= decay;
    return x < dtz ? 0.0 : x;
}

__global__ __launch_bounds__(G_THREADS) void k_gater_events(GaterState g, const uint32_t* __restrict__ pair_obs,
                                                            const DevGaterEvent* __restrict__ ev,
                                                            const uint32_t* __restrict__ group_off, uint32_t n_og) {
    const uint32_t i = blockIdx.x * G_THREADS + threadIdx.x;
    if (i >= n_og) return;
    const uint32_t b = group_off[i], en = group_off[i + 1];
    const uint32_t u = pair_obs[ev[b].pair];
    double validate = g.validate[u], throttle = g.throttle[u];
    int64_t last = g.last_throttle[u];
    for (uint32_t k = b; k < en; ++k) {
        const DevGaterEvent e = ev[k];
        if (e.kind == GEV_VALIDATE) {  // :393-398
            validate = validate + 1;
            continue;
        }
        if (e.kind == GEV_THROTTLE) {  // :421-425
            last = e.now_ns;
            throttle = throttle + 1;
            continue;
        }
        uint32_t grp = g.bind[e.pair];
        if (e.kind == GEV_ADD) {  // getPeerStats + connected++ (:369-375)
            if (grp == GATER_UNBOUND) {
                grp = e.group;
                if (grp >= g.n_groups) continue;  // (the host resolves it inside the arrays)
                g.bind[e.pair] = grp;
            }
            g.connected[grp] += 1;
            continue;
        }
        if (grp == GATER_UNBOUND) continue;  // a peer the gater never added (gsx.h)
        double* c = g.ctr + 4 * (size_t)grp;
        switch (e.kind) {
            case GEV_REMOVE:  // :377-386
                g.connected[grp] -= 1;
                g.expire[grp] = e.now_ns + g.retain_ns;
                g.bind[e.pair] = GATER_UNBOUND;
                break;
            case GEV_DELIVER: c[GC_DELIVER] = c[GC_DELIVER] + e.weight; break;  // :400-414
            case GEV_DUPLICATE: c[GC_DUPLICATE] = c[GC_DUPLICATE] + 1; break;   // :437-443
            case GEV_IGNORE: c[GC_IGNORE] = c[GC_IGNORE] + 1; break;            // :427-429
            case GEV_REJECT: c[GC_REJECT] = c[GC_REJECT] + 1; break;            // :431-433
            default: break;
        }
    }
    g.validate[u] = validate;
    g.throttle[u] = throttle;
    g.last_throttle[u] = last;
}

// decayStats, :219-259
__global__ __launch_bounds__(G_THREADS) void k_gater_decay(GaterState g, int64_t now) {
    const uint64_t stride = (uint64_t)gridDim.x * G_THREADS;
    const uint64_t t0 = (uint64_t)blockIdx.x * G_THREADS + threadIdx.x;
    for (uint64_t i = t0; i < g.n_groups; i += stride) {
        const uint32_t conn = g.connected[i];
        if (conn > 0) {
            double4* p = reinterpret_cast<double4*>(g.ctr) + i;
            double4 c = *p;
            if (c.x == 0 && c.y == 0 && c.z == 0 && c.w == 0) continue;  // (0 * decay = 0: nothing to store)
            c.x = decay_to_zero(c.x, g.source_decay, g.decay_to_zero);
            c.y = decay_to_zero(c.y, g.source_decay, g.decay_to_zero);
            c.z = decay_to_zero(c.z, g.source_decay, g.decay_to_zero);
            c.w = decay_to_zero(c.w, g.source_decay, g.decay_to_zero);
            *p = c;
        } else if (g.expire[i] < now) {  // delete(pg.ipStats, ip): a later AddPeer starts from zeros
            reinterpret_cast<double4*>(g.ctr)[i] = double4{0.0, 0.0, 0.0, 0.0};
            g.expire[i] = 0;
        }
    }
    for (uint64_t u = t0; u < g.n_obs; u += stride) {
        g.validate[u] = decay_to_zero(g.validate[u], g.global_decay, g.decay_to_zero);
        g.throttle[u] = decay_to_zero(g.throttle[u], g.global_decay, g.decay_to_zero);
    }
}

// The three tests of :330-342 that do not depend on the peer.
__global__ __launch_bounds__(G_THREADS) void k_gater_hot(GaterState g, int64_t now) {
    const uint32_t u = blockIdx.x * G_THREADS + threadIdx.x;
    if (u >= g.n_obs) return;
    const int64_t last = g.last_throttle[u];
    const double throttle = g.throttle[u], validate = g.validate[u];
    bool hot = true;
    // time.Since(lastThrottle) > Quiet; the zero time is always further back
    // (a throttle stamped after `now` is not in the past: not quiet)
    if (last == GATER_NEVER ||
        (now >= last && (g.quiet_ns < 0 || (uint64_t)now - (uint64_t)last > (uint64_t)g.quiet_ns)))
        hot = false;
    else if (throttle == 0) hot = false;
    else if (validate != 0 && throttle / validate < g.threshold) hot = false;
    g.hot[u] = hot ? 1 : 0;
}

__global__ __launch_bounds__(G_THREADS) void k_accept_from(GaterState g, AcceptArgs a) {
    for (uint64_t i = (uint64_t)blockIdx.x * G_THREADS + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * G_THREADS) {
        const uint64_t p = a.pairs ? a.pairs[i] : i;
        uint8_t st = ACCEPT_ALL;
        if (!(a.eflags[p] & EDGE_DIRECT)) {          // gossipsub.go:584-587
            if (a.score[p] < a.graylist_threshold) {  // :589-591
                st = ACCEPT_NONE;
            } else if (a.gater && (a.pflags[p] & PAIR_PRESENT) && g.hot[a.pair_obs[p]]) {
                const uint32_t grp = g.bind[p];
                if (grp != GATER_UNBOUND) {
                    const double4 c = reinterpret_cast<const double4*>(g.ctr)[grp];
                    // deliver, duplicate, ignore, reject = x, y, z, w (GC_*); :347
                    double total = c.x + g.duplicate_weight * c.y;
                    total = total + g.ignore_weight * c.z;
                    total = total + g.reject_weight * c.w;
                    if (total != 0) {
                        const double threshold = (1 + c.x) / (1 + total);  // :356
                        const double u = (double)(h4(a.seed, TAG_GATER, p, a.draw) >> 11) * 0x1p-53;
                        if (!(u < threshold)) st = ACCEPT_CONTROL;  // :357-362
                    }
                }
            }
        }
        a.out[i] = st;
    }
}

__global__ __launch_bounds__(G_THREADS) void k_gater_fold_count(GaterState g, const uint32_t* __restrict__ pair_obs,
                                                                const uint64_t* __restrict__ from_mask,
                                                                const uint64_t* __restrict__ dup_rows,
                                                                const uint64_t* __restrict__ cls, uint32_t W,
                                                                uint32_t* __restrict__ gcnt, uint32_t* __restrict__ ocnt) {
    for (uint64_t q = (uint64_t)blockIdx.x * G_THREADS + threadIdx.x; q < g.n_pairs; q += (uint64_t)gridDim.x * G_THREADS) {
        uint32_t nd = 0, nj = 0, ni = 0, nt = 0, nc = 0;
        for (uint32_t w = 0; w < W; ++w) {
            const uint64_t f = from_mask[q * W + w];
            nd += (uint32_t)__popcll(f & cls[w]);          // GSX_VALIDATION_ACCEPT
            nj += (uint32_t)__popcll(f & cls[W + w]);      // REJECT
            ni += (uint32_t)__popcll(f & cls[2 * W + w]);  // IGNORE
            nt += (uint32_t)__popcll(f & cls[3 * W + w]);  // THROTTLE
            nc += (uint32_t)__popcll(dup_rows[q * W + w]);
        }
        const uint32_t na = nd + nj + ni + nt;
        if ((na | nc) == 0) continue;
        const uint32_t u = pair_obs[q];
        if (na) atomicAdd(ocnt + 2 * (size_t)u, na);
        if (nt) atomicAdd(ocnt + 2 * (size_t)u + 1, nt);
        const uint32_t grp = g.bind[q];
        if (grp == GATER_UNBOUND) continue;
        uint32_t* c = gcnt + 4 * (size_t)grp;
        if (nd) atomicAdd(c + GC_DELIVER, nd);
        if (nc) atomicAdd(c + GC_DUPLICATE, nc);
        if (ni) atomicAdd(c + GC_IGNORE, ni);
        if (nj) atomicAdd(c + GC_REJECT, nj);
    }
}

__global__ __launch_bounds__(G_THREADS) void k_gater_fold_apply(GaterState g, uint32_t* __restrict__ gcnt,
                                                                uint32_t* __restrict__ ocnt, double weight, int64_t now) {
    const uint64_t stride = (uint64_t)gridDim.x * G_THREADS;
    const uint64_t t0 = (uint64_t)blockIdx.x * G_THREADS + threadIdx.x;
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    for (uint64_t i = t0; i < g.n_groups; i += stride) {
        const uint4 k = reinterpret_cast<const uint4*>(gcnt)[i];
        if ((k.x | k.y | k.z | k.w) == 0) continue;
        double4* p = reinterpret_cast<double4*>(g.ctr) + i;
        double4 c = *p;
        if (weight == 1.0) {
            c.x = add_ones_capped(c.x, k.x, inf);
        } else {
            for (uint32_t s = 0; s < k.x; ++s) c.x = c.x + weight;
        }
        c.y = add_ones_capped(c.y, k.y, inf);
        c.z = add_ones_capped(c.z, k.z, inf);
        c.w = add_ones_capped(c.w, k.w, inf);
        *p = c;
        reinterpret_cast<uint4*>(gcnt)[i] = uint4{0, 0, 0, 0};
    }
    for (uint64_t u = t0; u < g.n_obs; u += stride) {
        const uint2 k = reinterpret_cast<const uint2*>(ocnt)[u];
        if ((k.x | k.y) == 0) continue;
        if (k.x) g.validate[u] = add_ones_capped(g.validate[u], k.x, inf);
        if (k.y) {
            g.throttle[u] = add_ones_capped(g.throttle[u], k.y, inf);
            g.last_throttle[u] = now;
        }
        reinterpret_cast<uint2*>(ocnt)[u] = uint2{0, 0};
    }
}

inline unsigned grid_for(uint64_t n) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + G_THREADS - 1) / G_THREADS, 4096));
}

}  // namespace

hipError_t launch_gater_events(const GaterState& g, const uint32_t* pair_obs, const DevGaterEvent* ev,
                               const uint32_t* group_off, uint32_t n_obs_groups, hipStream_t st) {
    if (n_obs_groups == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gater_events, dim3((n_obs_groups + G_THREADS - 1) / G_THREADS), dim3(G_THREADS), 0, st, g,
                       pair_obs, ev, group_off, n_obs_groups);
    return hipGetLastError();
}

hipError_t launch_gater_decay(const GaterState& g, int64_t now, hipStream_t st) {
    if (g.n_groups == 0 && g.n_obs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gater_decay, dim3(grid_for(std::max<uint64_t>(g.n_groups, g.n_obs))), dim3(G_THREADS), 0, st, g,
                       now);
    return hipGetLastError();
}

hipError_t launch_accept_from(const GaterState& g, const AcceptArgs& a, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    if (a.gater && g.n_obs) {
        hipLaunchKernelGGL(k_gater_hot, dim3((g.n_obs + G_THREADS - 1) / G_THREADS), dim3(G_THREADS), 0, st, g, a.now);
        if (hipError_t rc = hipGetLastError()) return rc;
    }
    hipLaunchKernelGGL(k_accept_from, dim3(grid_for(a.n)), dim3(G_THREADS), 0, st, g, a);
    return hipGetLastError();
}

hipError_t launch_gater_fold_count(const GaterState& g, const uint32_t* pair_obs, const uint64_t* from_mask,
                                   const uint64_t* dup_rows, const uint64_t* cls, uint32_t n_words, uint32_t* gcnt,
                                   uint32_t* ocnt, hipStream_t st) {
    if (g.n_pairs == 0 || n_words == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gater_fold_count, dim3(grid_for(g.n_pairs)), dim3(G_THREADS), 0, st, g, pair_obs, from_mask,
                       dup_rows, cls, n_words, gcnt, ocnt);
    return hipGetLastError();
}

hipError_t launch_gater_fold_apply(const GaterState& g, uint32_t* gcnt, uint32_t* ocnt, double weight, int64_t now,
                                   hipStream_t st) {
    if (g.n_groups == 0 && g.n_obs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gater_fold_apply, dim3(grid_for(std::max<uint64_t>(g.n_groups, g.n_obs))), dim3(G_THREADS), 0,
                       st, g, gcnt, ocnt, weight, now);
    return hipGetLastError();
}

}  // namespace gsx
