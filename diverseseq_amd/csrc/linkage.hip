// Hierarchical-clustering tree of a precomputed N x N distance matrix: the tree stage of ctree.
//
// Replaces, for diverse_seq/cluster.py:216-230 (AgglomerativeClustering(metric="precomputed",
// linkage="average")), what sklearn runs underneath: scipy.cluster.hierarchy.linkage(X[triu], "average"),
// i.e. scipy's nearest-neighbour chain (_hierarchy.nn_chain) and its union-find relabelling (`label`);
// and, with the same kernels, scipy's other methods built by the same two algorithms: "complete",
// "weighted" and "ward" (nn_chain, another update of the merged row) and "single" (_hierarchy.
// mst_single_linkage, Prim's loop).  ("centroid" and "median" are scipy's fast_linkage: not built.)
// The result is scipy's Z bit for bit -- same pairs, same heights, same sizes -- so every tie resolves
// the same way:
//   * an argmin over row x takes the LOWEST index among equal values (scipy's strict `<` in ascending
//     order), and the previous chain element wins a tie against it;
//   * a merge of a < b writes row / column b by scipy's _hierarchy_distance_update.pxi, same operands in
//     the same order (-ffp-contract=off: no fma; real divisions and square roots), d_xi = D[i][a],
//     d_yi = D[i][b], d_xy the merge height:
//       average   (double(na) * d_xi + double(nb) * d_yi) / double(na + nb)
//       complete  d_yi > d_xi ? d_yi : d_xi                      (Cython's max(d_xi, d_yi), not fmax)
//       weighted  0.5 * (d_xi + d_yi)
//       ward      t = 1.0 / double(na + nb + ni); sqrt(double(ni + na) * t * d_xi * d_xi
//                 + double(ni + nb) * t * d_yi * d_yi - double(ni) * t * d_xy * d_xy)
//   * the records are stable-sorted by height and relabelled on the host, as scipy does (single
//     linkage's records too: mst_single_linkage ends in the same sort and `label`).
//
// Device pipeline (one stream, no host round trip inside the loop):
//   1. linkage_prepare_kernel: every entry is checked (sklearn's check_array looks at the whole matrix:
//      NaN / +-inf anywhere -> DVS_ERR_VALUE) and the upper triangle is copied over the lower one (only
//      D[i][j], i < j, counts: X[np.triu_indices(n, 1)]); 32 x 32 tile pairs through LDS.  For ward, a
//      negative entry of the upper triangle is flagged too (DVS_ERR_VALUE: scipy's sqrt of a negative
//      gives NaN heights, whose stable sort is undefined).
//   2. linkage_nn_chain_kernel<method>: ONE persistent workgroup of 1024 threads runs the whole chain.  Every
//      step depends on the one before, so a grid would pay a grid barrier per step (~4 us, MI355X barrier-xcd)
//      where a workgroup barrier costs a few hundred cycles.  The chain, the sizes, the records and a
//      compacted, ascending list of the active clusters live in global scratch (N may exceed the LDS);
//      scans walk the list, never a dead column.  Column b is kept consistent by mirrored writes.
//      The loop is bounded: at most 3 (n - 1) argmin steps (n - 1 of them end in a merge, every other
//      one pushes a cluster and a merge pops two), else an error word and an early return.
//   2'. linkage_mst_single_kernel (single): the same workgroup shape runs Prim's loop, exactly n - 1 steps of
//      one row read and one argmin over the compacted list of unmerged points; D is only read.
//
// At the end of the file, host only: dvs_linkage_cut, the flat clusters of such a tree at a height or at a number of
// clusters (the partitions of scipy's fcluster "distance" and "maxclust").
#include "dvs_internal.h"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace {

constexpr int LNK_THREADS = 1024;
constexpr int LNK_WAVES = LNK_THREADS / 64;
constexpr int LNK_UNROLL = 4;  // independent loads in flight per thread and pass
constexpr uint32_t LNK_TILE = 32;
constexpr uint32_t LNK_NONE = 0xFFFFFFFFu;

// status words (device): [0] prepare / loop outcome (LNK_NONFINITE and LNK_NEGATIVE are bits), [1] the distance
// kernel's zero-division flag
enum : uint32_t { LNK_OK = 0, LNK_NONFINITE = DVS_LNK_NONFINITE, LNK_NO_CONVERGE = 2, LNK_NEGATIVE = DVS_LNK_NEGATIVE };

// scipy's _LINKAGE_METHODS codes (the ABI's `method`)
enum : int { LNK_SINGLE = 0, LNK_COMPLETE = 1, LNK_AVERAGE = 2, LNK_CENTROID = 3, LNK_MEDIAN = 4, LNK_WARD = 5,
             LNK_WEIGHTED = 6 };

template <typename K>
__device__ __forceinline__ bool lnk_better(double v, K i, double bv, K bi) {
    return v < bv || (v == bv && i < bi);
}

// The workgroup's least (value, key) by lnk_better, into every thread's bv / bk: shuffles within each wave, then the
// per-wave minima through LDS buffer ph and one barrier.  Callers alternate ph: a buffer is written again only after
// the next call's barrier, which every reader of this call has passed.  (The chain kernel writes the same reduction
// out inline: through this helper its average instantiation compiles to other code, 66 VGPRs instead of 70.)
template <typename K>
__device__ __forceinline__ void lnk_block_argmin(double &bv, K &bk, double (&s_v)[2][LNK_WAVES], K (&s_k)[2][LNK_WAVES],
                                                 uint32_t ph) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const K ok = __shfl_xor(bk, o, 64);
        if (lnk_better(ov, ok, bv, bk)) {
            bv = ov;
            bk = ok;
        }
    }
    if (lane == 0) {
        s_v[ph][wave] = bv;
        s_k[ph][wave] = bk;
    }
    __syncthreads();
    bv = s_v[ph][0];
    bk = s_k[ph][0];
#pragma unroll
    for (int w = 1; w < LNK_WAVES; w++)
        if (lnk_better(s_v[ph][w], s_k[ph][w], bv, bk)) {
            bv = s_v[ph][w];
            bk = s_k[ph][w];
        }
}

// Check + mirror, one 32 x 32 tile pair (bi >= bj) per workgroup: the upper tile (bj, bi) is staged in LDS and
// written transposed over the lower tile (bi, bj); both are checked.  A diagonal tile mirrors onto itself.
// SIGN (ward): a negative entry above the diagonal sets LNK_NEGATIVE.
template <bool SIGN>
__global__ __launch_bounds__(256) void linkage_prepare_kernel(double *__restrict__ D, uint32_t n,
                                                              uint32_t *__restrict__ status) {
    __shared__ double s_up[LNK_TILE][LNK_TILE + 1];
    const uint32_t bi = blockIdx.x, bj = blockIdx.y;
    if (bj > bi) return;
    const uint32_t tx = threadIdx.x & (LNK_TILE - 1), ty = threadIdx.x / LNK_TILE;  // 32 x 8
    bool bad = false, neg = false;
    // the upper tile: rows bj * 32 + r, columns bi * 32 + tx
    for (uint32_t r = ty; r < LNK_TILE; r += 256 / LNK_TILE) {
        const uint32_t row = bj * LNK_TILE + r, col = bi * LNK_TILE + tx;
        double v = 0.0;
        if (row < n && col < n) {
            v = D[size_t(row) * n + col];
            bad |= !__builtin_isfinite(v);
            if constexpr (SIGN) neg |= row < col && v < 0.0;
        }
        s_up[r][tx] = v;
    }
    // the lower tile's own entries are checked before they are overwritten (a diagonal tile is its own upper tile)
    if (bi != bj)
        for (uint32_t r = ty; r < LNK_TILE; r += 256 / LNK_TILE) {
            const uint32_t row = bi * LNK_TILE + r, col = bj * LNK_TILE + tx;
            if (row < n && col < n) bad |= !__builtin_isfinite(D[size_t(row) * n + col]);
        }
    __syncthreads();
    // lower tile entry (bi * 32 + r, bj * 32 + tx) = upper entry (bj * 32 + tx, bi * 32 + r)
    for (uint32_t r = ty; r < LNK_TILE; r += 256 / LNK_TILE) {
        const uint32_t row = bi * LNK_TILE + r, col = bj * LNK_TILE + tx;
        if (row < n && col < n && row > col) D[size_t(row) * n + col] = s_up[tx][r];
    }
    if (bad) atomicOr(status, LNK_NONFINITE);
    if constexpr (SIGN)
        if (neg) atomicOr(status, LNK_NEGATIVE);
}

// scipy's _hierarchy_distance_update.pxi for the merge of x = a < y = b (see the top of the file); dna, dnb, dn:
// double(na), double(nb), double(na + nb), hoisted out of the loop
template <int METHOD>
__device__ __forceinline__ double lnk_merged(double d_xi, double d_yi, double d_xy, uint32_t na, uint32_t nb,
                                             uint32_t ni, double dna, double dnb, double dn) {
    if constexpr (METHOD == LNK_AVERAGE) {
        return (dna * d_xi + dnb * d_yi) / dn;
    } else if constexpr (METHOD == LNK_COMPLETE) {
        return d_yi > d_xi ? d_yi : d_xi;
    } else if constexpr (METHOD == LNK_WEIGHTED) {
        return 0.5 * (d_xi + d_yi);
    } else {
        static_assert(METHOD == LNK_WARD, "nn_chain methods: average, complete, weighted, ward");
        const double t = 1.0 / double(na + nb + ni);
        return sqrt(double(ni + na) * t * d_xi * d_xi + double(ni + nb) * t * d_yi * d_yi - double(ni) * t * d_xy * d_xy);
    }
}

// scratch of the loop (global): size[n], chain[n], act[2][n] (the active list and its next compaction)
// records (global, copied out): rec_h[n - 1], rec_pair[2 (n - 1)], rec_size[n - 1]
template <int METHOD>
__global__ __launch_bounds__(LNK_THREADS) void linkage_nn_chain_kernel(
    double *__restrict__ D, uint32_t n, uint32_t *__restrict__ size, uint32_t *__restrict__ chain,
    uint32_t *act_a, uint32_t *act_b, double *__restrict__ rec_h,  // (act_a / act_b swap roles every merge)
    uint32_t *__restrict__ rec_pair, uint32_t *__restrict__ rec_size, uint32_t *__restrict__ status) {
    __shared__ double s_v[2][LNK_WAVES];  // per-wave minima, alternating buffers: one barrier per argmin step
    __shared__ uint32_t s_i[2][LNK_WAVES];
    __shared__ uint32_t s_pos;            // position of the merged-away cluster in the active list
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (status[0] != LNK_OK) return;  // (the prepare pass found a non-finite entry, or a negative one for ward)
    for (uint32_t i = tid; i < n; i += LNK_THREADS) {
        size[i] = 1;
        act_a[i] = i;
    }
    __syncthreads();
    uint32_t *act = act_a, *act_next = act_b;
    uint32_t m = n;               // active clusters
    uint32_t chain_len = 0;       // (every value below is uniform over the workgroup)
    uint32_t x = 0, prev = 0;     // chain[chain_len - 1], chain[chain_len - 2]
    uint32_t steps = 0, ph = 0;
    const uint32_t max_steps = 3u * (n - 1u);
    for (uint32_t k = 0; k + 1 < n; k++) {
        if (chain_len == 0) {  // the smallest active cluster starts a chain
            x = act[0];
            if (tid == 0) chain[0] = x;
            chain_len = 1;
        }
        uint32_t y;
        double cur;
        for (;;) {
            if (steps++ >= max_steps) {
                if (tid == 0) status[0] = LNK_NO_CONVERGE;
                return;
            }
            const double *row = D + size_t(x) * n;
            const double c_prev = chain_len > 1 ? row[prev] : 0.0;
            double bv = __builtin_inf();
            uint32_t bi = LNK_NONE;
            for (uint32_t t0 = tid; t0 < m; t0 += LNK_UNROLL * LNK_THREADS) {
                uint32_t ii[LNK_UNROLL];
                double vv[LNK_UNROLL];
#pragma unroll
                for (int u = 0; u < LNK_UNROLL; u++) {
                    const uint32_t t = t0 + u * LNK_THREADS;
                    ii[u] = t < m ? act[t] : LNK_NONE;
                    if (ii[u] == x) ii[u] = LNK_NONE;
                }
#pragma unroll
                for (int u = 0; u < LNK_UNROLL; u++) vv[u] = ii[u] != LNK_NONE ? row[ii[u]] : __builtin_inf();
#pragma unroll
                for (int u = 0; u < LNK_UNROLL; u++)
                    if (ii[u] != LNK_NONE && lnk_better(vv[u], ii[u], bv, bi)) {
                        bv = vv[u];
                        bi = ii[u];
                    }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(bv, o, 64);
                const uint32_t oi = __shfl_xor(bi, o, 64);
                if (lnk_better(ov, oi, bv, bi)) {
                    bv = ov;
                    bi = oi;
                }
            }
            if (lane == 0) {
                s_v[ph][wave] = bv;
                s_i[ph][wave] = bi;
            }
            __syncthreads();
            bv = s_v[ph][0];
            bi = s_i[ph][0];
#pragma unroll
            for (int w = 1; w < LNK_WAVES; w++)
                if (lnk_better(s_v[ph][w], s_i[ph][w], bv, bi)) {
                    bv = s_v[ph][w];
                    bi = s_i[ph][w];
                }
            ph ^= 1u;
            // scipy: cur = D[x][prev] (or +inf), then `if D[x][i] < cur` in ascending i
            if (chain_len > 1 && !(bv < c_prev)) {
                y = prev;
                cur = c_prev;
            } else {
                y = bi;
                cur = bv;
            }
            if (chain_len > 1 && y == prev) break;
            if (chain_len >= n || y >= n) {  // (cannot happen on a finite matrix; never write past the chain)
                if (tid == 0) status[0] = LNK_NO_CONVERGE;
                return;
            }
            if (tid == 0) chain[chain_len] = y;
            chain_len++;
            prev = x;
            x = y;
        }
        // merge x and y: a < b, b takes the new cluster
        const uint32_t a = x < y ? x : y, b = x < y ? y : x;
        const uint32_t na = size[a], nb = size[b];
        const double dna = double(na), dnb = double(nb), dn = double(na + nb);
        const double *ra = D + size_t(a) * n;
        double *rb = D + size_t(b) * n;
        for (uint32_t t0 = tid; t0 < m; t0 += LNK_UNROLL * LNK_THREADS) {
            uint32_t ii[LNK_UNROLL], ni[LNK_UNROLL] = {};
            double va[LNK_UNROLL], vb[LNK_UNROLL];
#pragma unroll
            for (int u = 0; u < LNK_UNROLL; u++) {
                const uint32_t t = t0 + u * LNK_THREADS;
                ii[u] = t < m ? act[t] : LNK_NONE;
                if (ii[u] == a) s_pos = t;
                if (ii[u] == a || ii[u] == b) ii[u] = LNK_NONE;
            }
#pragma unroll
            for (int u = 0; u < LNK_UNROLL; u++) {
                va[u] = ii[u] != LNK_NONE ? ra[ii[u]] : 0.0;
                vb[u] = ii[u] != LNK_NONE ? rb[ii[u]] : 0.0;
                if constexpr (METHOD == LNK_WARD) ni[u] = ii[u] != LNK_NONE ? size[ii[u]] : 0u;
            }
#pragma unroll
            for (int u = 0; u < LNK_UNROLL; u++)
                if (ii[u] != LNK_NONE) {
                    const double d = lnk_merged<METHOD>(va[u], vb[u], cur, na, nb, ni[u], dna, dnb, dn);
                    rb[ii[u]] = d;
                    D[size_t(ii[u]) * n + b] = d;
                }
        }
        __syncthreads();  // (s_pos; every thread has read size[a], size[b] and, for ward, size[i])
        const uint32_t p = s_pos;
        if (tid == 0) {
            rec_pair[2 * k] = a;
            rec_pair[2 * k + 1] = b;
            rec_h[k] = cur;
            rec_size[k] = na + nb;
            size[a] = 0;
            size[b] = na + nb;
        }
        for (uint32_t t = tid; t < m; t += LNK_THREADS)
            if (t != p) act_next[t - (t > p ? 1u : 0u)] = act[t];
        __syncthreads();  // (the new list, the chain and the sizes are visible to every thread)
        uint32_t *sw = act;
        act = act_next;
        act_next = sw;
        m--;
        chain_len -= 2;
        if (chain_len > 0) x = chain[chain_len - 1];
        if (chain_len > 1) prev = chain[chain_len - 2];
    }
}

// scipy's mst_single_linkage: from x = 0, each of the n - 1 steps marks x merged, lowers dm[i] to D[x][i] where that is
// smaller (strict >), takes the argmin of dm over the unmerged points (strict <, ascending: the lowest index wins a
// tie), records (x, y, dm[y]) and goes on from x = y.  Scratch (global): dm[n], act[2][n].  act holds the unmerged
// points in ascending order with x among them, at position p; the pass that reads them writes the list without x into
// act_next, and the argmin's key (index << 32 | position in act_next) hands y and its position to the next step.
// One barrier per step (the argmin's); D is only read.
__global__ __launch_bounds__(LNK_THREADS) void linkage_mst_single_kernel(
    const double *__restrict__ D, uint32_t n, double *__restrict__ dm, uint32_t *act_a, uint32_t *act_b,
    double *__restrict__ rec_h, uint32_t *__restrict__ rec_pair, uint32_t *__restrict__ status) {
    __shared__ double s_v[2][LNK_WAVES];
    __shared__ uint64_t s_k[2][LNK_WAVES];
    const uint32_t tid = threadIdx.x;
    if (status[0] != LNK_OK) return;  // (the prepare pass found a non-finite entry)
    for (uint32_t i = tid; i < n; i += LNK_THREADS) {
        dm[i] = __builtin_inf();
        act_a[i] = i;
    }
    __syncthreads();
    uint32_t *act = act_a, *act_next = act_b;
    uint32_t m = n;            // points in act, x included (every value below is uniform over the workgroup)
    uint32_t x = 0, p = 0, ph = 0;
    for (uint32_t k = 0; k + 1 < n; k++) {
        const double *row = D + size_t(x) * n;
        double bv = __builtin_inf();
        uint64_t bk = ~uint64_t(0);
        for (uint32_t t0 = tid; t0 < m; t0 += LNK_UNROLL * LNK_THREADS) {
            uint32_t ii[LNK_UNROLL];
            double dv[LNK_UNROLL], mv[LNK_UNROLL];
#pragma unroll
            for (int u = 0; u < LNK_UNROLL; u++) {
                const uint32_t t = t0 + u * LNK_THREADS;
                ii[u] = t < m ? act[t] : LNK_NONE;
                if (t == p) ii[u] = LNK_NONE;
                if (ii[u] != LNK_NONE) act_next[t - (t > p ? 1u : 0u)] = ii[u];
            }
#pragma unroll
            for (int u = 0; u < LNK_UNROLL; u++) {
                dv[u] = ii[u] != LNK_NONE ? row[ii[u]] : 0.0;
                mv[u] = ii[u] != LNK_NONE ? dm[ii[u]] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < LNK_UNROLL; u++)
                if (ii[u] != LNK_NONE) {
                    if (mv[u] > dv[u]) {
                        mv[u] = dv[u];
                        dm[ii[u]] = dv[u];
                    }
                    const uint32_t t = t0 + u * LNK_THREADS;
                    const uint64_t key = uint64_t(ii[u]) << 32 | (t - (t > p ? 1u : 0u));
                    if (lnk_better(mv[u], key, bv, bk)) {
                        bv = mv[u];
                        bk = key;
                    }
                }
        }
        lnk_block_argmin(bv, bk, s_v, s_k, ph);  // (also orders this step's act_next / dm writes before the next step)
        ph ^= 1u;
        const uint32_t y = uint32_t(bk >> 32);
        if (y >= n) {  // (cannot happen: an unmerged point is left and every dm is finite)
            if (tid == 0) status[0] = LNK_NO_CONVERGE;
            return;
        }
        if (tid == 0) {
            rec_pair[2 * k] = x;
            rec_pair[2 * k + 1] = y;
            rec_h[k] = bv;
        }
        uint32_t *sw = act;
        act = act_next;
        act_next = sw;
        m--;
        x = y;
        p = uint32_t(bk);
    }
}

// byte offsets of the scratch block: what is copied back first, then what stays on the device (dm: single linkage's)
struct LnkLayout {
    size_t status, rec_h, rec_pair, rec_size, out_bytes, size, chain, act_a, act_b, dm, bytes;
    explicit LnkLayout(uint32_t n) {
        auto up8 = [](size_t v) { return (v + 7) & ~size_t(7); };
        const size_t m1 = size_t(n) - 1;
        status = 0;
        rec_h = 16;
        rec_pair = rec_h + m1 * 8;
        rec_size = up8(rec_pair + 2 * m1 * 4);
        out_bytes = up8(rec_size + m1 * 4);
        size = out_bytes;
        chain = size + size_t(n) * 4;
        act_a = chain + size_t(n) * 4;
        act_b = act_a + size_t(n) * 4;
        dm = up8(act_b + size_t(n) * 4);
        bytes = dm + size_t(n) * 8;
    }
};

const char *lnk_name(int method) {
    switch (method) {
        case LNK_SINGLE: return "single";
        case LNK_COMPLETE: return "complete";
        case LNK_AVERAGE: return "average";
        case LNK_WARD: return "ward";
        case LNK_WEIGHTED: return "weighted";
        default: return "unknown";
    }
}

// the chain kernel of one nn_chain method, or single linkage's loop, enqueued behind the prepare pass
hipError_t lnk_launch_tree(dvs_ctx *ctx, int method, double *d_dist, uint32_t n, char *base, const LnkLayout &L) {
    auto u32 = [&](size_t off) { return reinterpret_cast<uint32_t *>(base + off); };
    auto f64 = [&](size_t off) { return reinterpret_cast<double *>(base + off); };
    auto chain = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(1), dim3(LNK_THREADS), 0, ctx->stream, d_dist, n, u32(L.size), u32(L.chain),
                           u32(L.act_a), u32(L.act_b), f64(L.rec_h), u32(L.rec_pair), u32(L.rec_size), u32(L.status));
    };
    switch (method) {
        case LNK_SINGLE:
            hipLaunchKernelGGL(linkage_mst_single_kernel, dim3(1), dim3(LNK_THREADS), 0, ctx->stream, d_dist, n, f64(L.dm),
                               u32(L.act_a), u32(L.act_b), f64(L.rec_h), u32(L.rec_pair), u32(L.status));
            break;
        case LNK_COMPLETE: chain(linkage_nn_chain_kernel<LNK_COMPLETE>); break;
        case LNK_AVERAGE: chain(linkage_nn_chain_kernel<LNK_AVERAGE>); break;
        case LNK_WARD: chain(linkage_nn_chain_kernel<LNK_WARD>); break;
        case LNK_WEIGHTED: chain(linkage_nn_chain_kernel<LNK_WEIGHTED>); break;
        default: return hipErrorInvalidValue;  // (the entries check the method first)
    }
    return hipGetLastError();
}

// scipy's label(): the records in height order (stable), union-find roots as cluster ids n, n + 1, ...,
// the smaller root first, the size from the union
void linkage_relabel(uint32_t n, const double *rec_h, const uint32_t *rec_pair, uint32_t *pairs, double *heights,
                     uint32_t *sizes) {
    const uint32_t m1 = n - 1;
    std::vector<uint32_t> order(m1);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t p, uint32_t q) { return rec_h[p] < rec_h[q]; });
    std::vector<uint32_t> parent(2 * size_t(n) - 1), usize(2 * size_t(n) - 1, 1u);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t v) {
        uint32_t r = v;
        while (parent[r] != r) r = parent[r];
        while (parent[v] != r) {  // path compression
            const uint32_t nx = parent[v];
            parent[v] = r;
            v = nx;
        }
        return r;
    };
    for (uint32_t j = 0; j < m1; j++) {
        const uint32_t q = order[j];
        const uint32_t xr = find(rec_pair[2 * q]), yr = find(rec_pair[2 * q + 1]);
        const uint32_t lab = n + j;
        pairs[2 * j] = std::min(xr, yr);
        pairs[2 * j + 1] = std::max(xr, yr);
        heights[j] = rec_h[q];
        parent[xr] = parent[yr] = lab;
        usize[lab] = usize[xr] + usize[yr];
        sizes[j] = usize[lab];
    }
}

}  // namespace

// the prepare pass (check + mirror; `sign`: ward's, a negative entry above the diagonal flagged too) on the context's
// stream; *d_status collects DVS_LNK_NONFINITE / DVS_LNK_NEGATIVE
hipError_t dvs_linkage_enqueue_prepare(dvs_ctx *ctx, double *d_dist, uint32_t n, bool sign, uint32_t *d_status) {
    const uint32_t tiles = (n + LNK_TILE - 1) / LNK_TILE;
    if (sign)
        hipLaunchKernelGGL(linkage_prepare_kernel<true>, dim3(tiles, tiles), dim3(256), 0, ctx->stream, d_dist, n, d_status);
    else
        hipLaunchKernelGGL(linkage_prepare_kernel<false>, dim3(tiles, tiles), dim3(256), 0, ctx->stream, d_dist, n, d_status);
    return hipGetLastError();
}

// DVS_ERR_UNSUPPORTED / DVS_ERR_VALUE unless `method` (scipy's code) is one the device builds
static int linkage_check_method(dvs_ctx *ctx, int method) {
    if (method == LNK_CENTROID || method == LNK_MEDIAN)
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED,
                             "%s linkage is scipy's fast_linkage, not built on the device (single, complete, average, "
                             "weighted, ward)", method == LNK_CENTROID ? "centroid" : "median");
    if (method != LNK_SINGLE && method != LNK_COMPLETE && method != LNK_AVERAGE && method != LNK_WARD &&
        method != LNK_WEIGHTED)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "unknown linkage method %d", method);
    return DVS_OK;
}

// A consumer's run (dvs_internal.h dvs_square_consumer): the tree of the n x n matrix at d_dist (a working buffer:
// overwritten; single linkage only reads it once it is mirrored), enqueued on the context's stream behind whatever
// wrote the matrix.  Returns when the host outputs are written.
static int linkage_run(dvs_ctx *ctx, double *d_dist, uint32_t n, const uint32_t *d_zerodiv, int method, uint32_t *pairs,
                       double *heights, uint32_t *sizes) {
    const LnkLayout L(n);
    PooledBuf scratch{ctx};
    if (int rc = dvs_dev_alloc(ctx, &scratch.p, L.bytes, "linkage scratch")) return rc;
    char *base = scratch.as<char>();
    uint32_t *d_status = reinterpret_cast<uint32_t *>(base + L.status);
    std::vector<uint64_t> host((L.out_bytes + 7) / 8);
    const char *what = lnk_name(method);
    hipError_t e = dvs_status_begin(ctx, d_status, 16, 1, d_zerodiv);
    if (e == hipSuccess) e = dvs_linkage_enqueue_prepare(ctx, d_dist, n, method == LNK_WARD, d_status);
    if (e == hipSuccess) e = lnk_launch_tree(ctx, method, d_dist, n, base, L);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), base, L.out_bytes, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t se = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, what);
    if (se != hipSuccess) return dvs_hip_fail(ctx, se, what);
    const char *hb = reinterpret_cast<const char *>(host.data());
    const uint32_t *st = reinterpret_cast<const uint32_t *>(hb + L.status);
    if (st[1]) return dvs_set_error(ctx, DVS_ERR_ZERODIV, "division by zero");  // 0 / 0, distance.py:283
    if (st[0] & LNK_NONFINITE)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "Input contains NaN or infinity: the %u x %u distance matrix", n, n);
    if (st[0] & LNK_NEGATIVE)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "ward linkage needs non-negative distances: the %u x %u distance matrix "
                             "has a negative entry above its diagonal", n, n);
    if (st[0] != LNK_OK)
        return dvs_set_error(ctx, DVS_ERR_RUNTIME, "%s linkage: the loop did not finish within its bound of steps", what);
    linkage_relabel(n, reinterpret_cast<const double *>(hb + L.rec_h), reinterpret_cast<const uint32_t *>(hb + L.rec_pair),
                    pairs, heights, sizes);
    return DVS_OK;
}

// the method, then n: a caller's matrix is refused in sklearn's words (it checks every entry, as sklearn does)
dvs_square_consumer dvs_linkage_consumer(dvs_ctx *ctx, uint32_t n, bool given, int method, uint32_t *pairs, double *heights,
                                         uint32_t *sizes) {
    dvs_square_consumer c{"dvs_linkage"};
    c.check = [=] {
        if (int rc = linkage_check_method(ctx, method)) return rc;
        if (n >= 2) return int(DVS_OK);
        if (given) return dvs_set_error(ctx, DVS_ERR_VALUE, "Found array with %u sample(s) while a minimum of 2 is required", n);
        return dvs_set_error(ctx, DVS_ERR_VALUE, "need at least two sequences to build a tree");
    };
    c.extra_bytes = [=] { return LnkLayout(n).bytes; };
    snprintf(c.extra_what, sizeof c.extra_what, "its tree");
    c.writes_matrix = true;
    c.run = [=](double *d_dist, const uint32_t *d_zerodiv) {
        return linkage_run(ctx, d_dist, n, d_zerodiv, method, pairs, heights, sizes);
    };
    return c;
}

// The flat clusters of a cut (host only): the first m merges applied, m from the criterion; the merges name their
// children by scipy's ids (leaves 0 .. n - 1, merge j makes n + j), so a parent's id is above its children's and one
// pass from the top hands every node its root.
extern "C" int dvs_linkage_cut(dvs_ctx *ctx, uint32_t n, const uint32_t *pairs, const double *heights, int criterion,
                               double value, uint32_t *labels_out, uint32_t *n_clusters_out) {
    if (!pairs || !heights || !labels_out || !n_clusters_out) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (n < 2) return dvs_set_error(ctx, DVS_ERR_VALUE, "a tree of %u leaves cannot be cut: 2 at least", n);
    const uint32_t nm = n - 1;
    for (uint32_t j = 0; j < nm; j++)
        if (heights[j] != heights[j] || (j && heights[j] < heights[j - 1]))
            return dvs_set_error(ctx, DVS_ERR_VALUE, "merge %u: the heights of a linkage matrix must not decrease (or be NaN)", j);
    uint32_t m = 0;
    if (criterion == DVS_CUT_HEIGHT) {
        if (value != value) return dvs_set_error(ctx, DVS_ERR_VALUE, "the height of a cut cannot be NaN");
        while (m < nm && heights[m] <= value) m++;
    } else if (criterion == DVS_CUT_NCLUSTERS) {
        if (!(value >= 1.0) || value != std::floor(value))
            return dvs_set_error(ctx, DVS_ERR_VALUE, "the number of clusters must be an integer of 1 or more, not %g", value);
        m = value >= double(n) ? 0u : n - uint32_t(value);
        while (m > 0 && m < nm && heights[m] == heights[m - 1]) m++;  // (a cut never separates merges of equal height)
    } else {
        return dvs_set_error(ctx, DVS_ERR_VALUE, "unknown cut criterion %d", criterion);
    }
    std::vector<uint32_t> up(size_t(n) + m);
    for (uint32_t v = 0; v < n + m; v++) up[v] = v;
    for (uint32_t j = 0; j < m; j++) {
        const uint32_t x = pairs[2 * j], y = pairs[2 * j + 1];
        if (x >= n + j || y >= n + j || x == y || up[x] != x || up[y] != y)
            return dvs_set_error(ctx, DVS_ERR_VALUE, "merge %u joins %u and %u: not two clusters that exist at that point", j, x, y);
        up[x] = up[y] = n + j;
    }
    for (uint32_t v = n + m; v-- > 0;)
        if (up[v] != v) up[v] = up[up[v]];  // (the parent's entry is its root already)
    std::vector<uint32_t> label_of(size_t(n) + m, 0xFFFFFFFFu);
    uint32_t count = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t &l = label_of[up[i]];
        if (l == 0xFFFFFFFFu) l = count++;
        labels_out[i] = l;
    }
    *n_clusters_out = count;
    return DVS_OK;
}

// The in-order walk (host only, iterative: a caterpillar of any depth is fine).  A node on the stack is either to be
// expanded (its right child, the merge itself and its left child pushed, so that they come off left first) or, marked,
// a merge met between its two subtrees: it owns the gap behind the leaf emitted last.
int dvs_cophenet_walk(dvs_ctx *ctx, uint32_t n, const uint32_t *pairs, const double *heights, uint32_t *order,
                      uint32_t *pos, uint32_t *gap, double *c_bar) {
    if (n < 2) return dvs_set_error(ctx, DVS_ERR_VALUE, "a tree of %u leaves has no cophenetic distances: 2 at least", n);
    const uint32_t nm = n - 1;
    std::vector<uint32_t> size(2 * size_t(n) - 1, 1u);
    std::vector<bool> used(2 * size_t(n) - 1, false);
    long double sum = 0.0L;
    for (uint32_t j = 0; j < nm; j++) {
        const uint32_t x = pairs[2 * j], y = pairs[2 * j + 1];
        if (x >= n + j || y >= n + j || x == y || used[x] || used[y])
            return dvs_set_error(ctx, DVS_ERR_VALUE, "merge %u joins %u and %u: not two clusters that exist at that point", j, x, y);
        used[x] = used[y] = true;
        size[n + j] = size[x] + size[y];
        sum += (long double)(uint64_t(size[x]) * size[y]) * (long double)heights[j];
    }
    *c_bar = double(sum / ((long double)n * (long double)nm / 2.0L));
    constexpr uint32_t MARK = 0x80000000u;  // (ids stay below 2^31: n is bounded by the square entries' row limit)
    std::vector<uint32_t> stack;
    stack.push_back(2 * n - 2);
    uint32_t at = 0;
    while (!stack.empty()) {
        const uint32_t v = stack.back();
        stack.pop_back();
        if (v & MARK) {
            gap[at - 1] = v & ~MARK;
        } else if (v < n) {
            pos[v] = at;
            order[at++] = v;
        } else {
            const uint32_t j = v - n;
            stack.push_back(pairs[2 * j + 1]);
            stack.push_back(j | MARK);
            stack.push_back(pairs[2 * j]);
        }
    }
    return DVS_OK;
}

// scipy.cluster.hierarchy.cophenet(Z) as the square matrix, on the host: per leaf the running maximum of the gaps to
// the right of its position and of those to the left
extern "C" int dvs_linkage_cophenet(dvs_ctx *ctx, uint32_t n, const uint32_t *pairs, const double *heights, double *coph) {
    if (n == 0) return DVS_OK;
    if (!pairs || !heights || !coph) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (n > 0x40000000u) return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "a tree of %u leaves: 2^30 at most", n);
    std::vector<uint32_t> order(n), pos(n), gap(n - 1 ? n - 1 : 1);
    double c_bar;
    if (int rc = dvs_cophenet_walk(ctx, n, pairs, heights, order.data(), pos.data(), gap.data(), &c_bar)) return rc;
    for (uint32_t i = 0; i < n; i++) {
        double *row = coph + size_t(i) * n;
        const uint32_t p = pos[i];
        row[i] = 0.0;
        uint32_t m = 0;
        for (uint32_t q = p + 1; q < n; q++) {
            m = std::max(m, gap[q - 1]);
            row[order[q]] = heights[m];
        }
        m = 0;
        for (uint32_t q = p; q-- > 0;) {
            m = std::max(m, gap[q]);
            row[order[q]] = heights[m];
        }
    }
    return DVS_OK;
}
