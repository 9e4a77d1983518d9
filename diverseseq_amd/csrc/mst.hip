// The minimum spanning tree of a collection's distances without the matrix (include/dvs_hip.h "minimum spanning tree",
// DESIGN.md 4.18): Boruvka rounds, each one pass of the strip driver (crossdist.hip dvs_strip_run) with
// mst_foreign_min_kernel behind every strip, the components merged on the host between the passes.  At the end of the
// file, host only: dvs_linkage_from_mst, the single-linkage tree of such a spanning tree in dvs_linkage's layout.  No
// counterpart in the reference.
#include "dvs_internal.h"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace {

constexpr uint32_t NONE = DVS_NONE;

// For every row r of a strip (mq x n; position i = q0 + r) the least (w, j) over the columns j of another component
// (labels[j] != labels[i]) whose cell d = strip[r][j] is not NaN: w = d, or with a core vector max(d, core[i], core[j])
// (the mutual-reachability distance).  A tie goes to the lower j.  The row's own cell needs no special case: position
// i carries its own label.  Every row of the strip is written: (NONE, NaN) where no such column exists.
// Rows of up to MST_WAVE_ROW cells take a wave each (MST_WAVES rows per workgroup: a tall strip of short rows fills
// the device, and no barrier is needed); longer rows take a workgroup each, the waves' results meeting in LDS in wave
// order.  Either way a lane walks columns lane, lane + 64 (or + MST_THREADS), ...: every cell is read once, coalesced,
// the labels and the core values of the columns beside it (n x 12 bytes that stay in L2).  No atomics: the same bits
// on every run.
constexpr int MST_THREADS = 256;
constexpr uint32_t MST_WAVES = MST_THREADS / 64;
constexpr uint32_t MST_WAVE_ROW = 1024;

__device__ __forceinline__ bool mst_less(double w, uint32_t j, double bw, uint32_t bj) { return w < bw || (w == bw && j < bj); }

template <bool ROW_PER_WAVE>
__global__ __launch_bounds__(MST_THREADS) void mst_foreign_min_kernel(const double *__restrict__ strip, uint32_t n,
                                                                      uint32_t mq, uint32_t q0,
                                                                      const uint32_t *__restrict__ labels,
                                                                      const double *__restrict__ core,
                                                                      uint32_t *__restrict__ out_j,
                                                                      double *__restrict__ out_w) {
    __shared__ double s_w[MST_WAVES];
    __shared__ uint32_t s_j[MST_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = ROW_PER_WAVE ? blockIdx.x * MST_WAVES + wave : blockIdx.x;
    if (r >= mq) return;  // (the whole wave; ROW_PER_WAVE only: a row per workgroup has mq workgroups)
    const double *g = strip + uint64_t(r) * n;
    const uint32_t mine = labels[q0 + r];
    const double ci = core ? core[q0 + r] : 0.0;
    double bw = INFINITY;
    uint32_t bj = NONE;
    const uint32_t first = ROW_PER_WAVE ? lane : tid, step = ROW_PER_WAVE ? 64u : uint32_t(MST_THREADS);
#pragma unroll 4
    for (uint32_t j = first; j < n; j += step) {
        const double d = g[j];  // (three loads that do not depend on each other: the unrolled steps' loads go out together)
        const uint32_t lj = labels[j];
        double w = d;
        if (core) {
            const double cj = core[j];
            w = ci > w ? ci : w;
            w = cj > w ? cj : w;
        }
        if (d == d && lj != mine && mst_less(w, j, bw, bj)) {  // (a lane's columns ascend: < alone would do here)
            bw = w;
            bj = j;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ew = __shfl_xor(bw, o, 64);
        const uint32_t ej = __shfl_xor(bj, o, 64);
        if (mst_less(ew, ej, bw, bj)) {
            bw = ew;
            bj = ej;
        }
    }
    if (!ROW_PER_WAVE) {
        if (lane == 0) {
            s_w[wave] = bw;
            s_j[wave] = bj;
        }
        __syncthreads();
        bw = s_w[0];
        bj = s_j[0];
#pragma unroll
        for (uint32_t x = 1; x < MST_WAVES; x++)
            if (mst_less(s_w[x], s_j[x], bw, bj)) {
                bw = s_w[x];
                bj = s_j[x];
            }
    }
    if (ROW_PER_WAVE ? lane == 0 : tid == 0) {
        out_j[r] = bj;
        out_w[r] = bj == NONE ? double(NAN) : bw;
    }
}

struct mst_edge {
    double w;
    uint32_t lo, hi;
    bool operator<(const mst_edge &o) const { return w != o.w ? w < o.w : lo != o.lo ? lo < o.lo : hi < o.hi; }
};

constexpr uint32_t MST_MAX_ROUNDS = 32;  // (a round at least halves the components that have a pick: 32 serve any uint32 n)

}  // namespace

// The minimum spanning tree (forest, where NaN cells disconnect the positions) of a stage whose queries and references
// are the same n positions, by the order (weight, lower position, higher position) of its edges, under which it is
// unique (include/dvs_hip.h "minimum spanning tree").  Boruvka: the labels start as the identity; a round is one
// dvs_strip_run whose consumer uploads the labels, launches the kernel above behind each strip and copies the strip's
// candidates to the host at q0; then, on the host, every component takes the least (w, lo, hi) among its rows'
// candidates, the picks are sorted and applied through a union-find (union by lower root, path halving: a component's
// root is its lowest position) that drops a pick whose ends already share a root -- a mutual pick arrives twice, and an
// asymmetric matrix may close a cycle --, and every position is relabelled with its root.  It ends when one component
// is left or no component has a pick.  The labels, the core vector and the candidates share one block, allocated by
// the first round's begin and kept: the labels are uploaded whole every round, the core vector once, and the kernel
// writes every row's candidate before the copy behind it reads it.
int dvs_mst_strips(dvs_ctx *ctx, const dvs_cross_stage &st, const double *core, uint32_t *edges, double *weights,
                   uint32_t *n_edges, uint32_t *n_rounds) {
    const uint32_t n = st.n;
    if (n == 0) return DVS_OK;
    if (!edges || !weights || !n_edges) return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_mst: null argument");
    if (core)
        for (uint32_t i = 0; i < n; i++)
            if (!(core[i] >= 0.0) || std::isinf(core[i]))
                return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_mst: core distance %g of position %u: finite and not negative", core[i], i);
    if (int rc = st.check()) return rc;  // (before the host arrays: the source's own errors, the row limit)
    *n_edges = 0;
    if (n_rounds) *n_rounds = 0;
    if (n == 1) return DVS_OK;
    std::vector<uint32_t> labels, parent, cand_j, best;
    std::vector<double> cand_w;
    std::vector<mst_edge> picks, tree;
    try {
        labels.resize(n), parent.resize(n), cand_j.resize(n), best.resize(n), cand_w.resize(n);
        picks.reserve(n), tree.reserve(n - 1);
    } catch (const std::exception &) {
        return dvs_set_error(ctx, DVS_ERR_NOMEM, "dvs_mst: no host memory for the labels and candidates of %u positions", n);
    }
    std::iota(labels.begin(), labels.end(), 0u);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t x) {
        while (parent[x] != x) {
            parent[x] = parent[parent[x]];
            x = parent[x];
        }
        return x;
    };
    PooledBuf d_buf{ctx};  // core [n] f64 (or nothing), candidate weights [rows] f64, labels [n] u32, candidate columns [rows] u32
    double *d_core = nullptr, *d_cw = nullptr;
    uint32_t *d_labels = nullptr, *d_cj = nullptr;
    dvs_strip_consumer c{};
    c.begin = [&](uint32_t rows) {
        hipError_t e = hipSuccess;
        if (!d_buf.p) {
            const size_t n_core = core ? n : 0;
            if (int rc = dvs_dev_alloc(ctx, &d_buf.p, (n_core + rows) * 8 + (size_t(n) + rows) * 4, "spanning-tree labels and candidates"))
                return rc;
            d_cw = d_buf.as<double>() + n_core;
            d_core = core ? d_buf.as<double>() : nullptr;
            d_labels = reinterpret_cast<uint32_t *>(d_cw + rows);
            d_cj = d_labels + n;
            if (core) e = hipMemcpyAsync(d_core, core, size_t(n) * 8, hipMemcpyHostToDevice, ctx->stream);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(d_labels, labels.data(), size_t(n) * 4, hipMemcpyHostToDevice, ctx->stream);
        return e == hipSuccess ? DVS_OK : dvs_hip_fail(ctx, e, "spanning-tree labels upload");
    };
    c.strip = [&](uint32_t q0, uint32_t mq, double *d_strip) {
        if (n <= MST_WAVE_ROW)
            hipLaunchKernelGGL(mst_foreign_min_kernel<true>, dim3((mq + MST_WAVES - 1) / MST_WAVES), dim3(MST_THREADS), 0,
                               ctx->stream, d_strip, n, mq, q0, d_labels, d_core, d_cj, d_cw);
        else
            hipLaunchKernelGGL(mst_foreign_min_kernel<false>, dim3(mq), dim3(MST_THREADS), 0, ctx->stream, d_strip, n, mq, q0,
                               d_labels, d_core, d_cj, d_cw);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(cand_j.data() + q0, d_cj, size_t(mq) * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(cand_w.data() + q0, d_cw, size_t(mq) * 8, hipMemcpyDeviceToHost, ctx->stream);
        return e;
    };
    uint32_t rounds = 0;
    for (uint32_t components = n; components > 1;) {
        if (rounds == MST_MAX_ROUNDS)
            return dvs_set_error(ctx, DVS_ERR_RUNTIME, "dvs_mst: %u components left after %u rounds (internal error)", components, rounds);
        if (int rc = dvs_strip_run(ctx, st, c)) return rc;
        rounds++;
        // best[l]: the row of component l (its lowest position) whose candidate is the component's least so far
        std::fill(best.begin(), best.end(), NONE);
        auto edge_of = [&](uint32_t i) {
            const uint32_t j = cand_j[i];
            return mst_edge{cand_w[i], i < j ? i : j, i < j ? j : i};
        };
        for (uint32_t i = 0; i < n; i++) {
            if (cand_j[i] >= n) continue;  // (NONE: no column of another component)
            uint32_t &b = best[labels[i]];
            if (b == NONE || edge_of(i) < edge_of(b)) b = i;
        }
        picks.clear();
        for (uint32_t l = 0; l < n; l++)
            if (best[l] != NONE) picks.push_back(edge_of(best[l]));
        if (picks.empty()) break;  // a forest: what is left is joined by NaN cells only
        std::sort(picks.begin(), picks.end());
        for (const mst_edge &p : picks) {
            const uint32_t a = find(p.lo), b = find(p.hi);
            if (a == b) continue;
            parent[a > b ? a : b] = a > b ? b : a;
            tree.push_back(p);
            components--;
        }
        for (uint32_t i = 0; i < n; i++) labels[i] = find(i);
    }
    std::sort(tree.begin(), tree.end());
    for (size_t e = 0; e < tree.size(); e++) {
        edges[2 * e] = tree[e].lo;
        edges[2 * e + 1] = tree[e].hi;
        weights[e] = tree[e].w;
    }
    *n_edges = uint32_t(tree.size());
    if (n_rounds) *n_rounds = rounds;
    return DVS_OK;
}

// The n - 1 edges of a spanning tree in ascending weight -> the single-linkage tree in dvs_linkage's layout (host only):
// edge e joins the clusters its two ends are in at that point into cluster n + e, the lower id first.
extern "C" int dvs_linkage_from_mst(dvs_ctx *ctx, uint32_t n, const uint32_t *edges, const double *weights, uint32_t *pairs,
                                    double *heights, uint32_t *sizes) {
    if (!edges || !weights || !pairs || !heights || !sizes) return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_linkage_from_mst: null argument");
    if (n < 2) return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_linkage_from_mst: a tree of %u leaves: 2 at least", n);
    std::vector<uint32_t> parent, id, size;
    try {
        parent.resize(n), id.resize(n), size.assign(n, 1u);
    } catch (const std::exception &) {
        return dvs_set_error(ctx, DVS_ERR_NOMEM, "dvs_linkage_from_mst: no host memory for the union-find of %u leaves", n);
    }
    std::iota(parent.begin(), parent.end(), 0u);
    std::iota(id.begin(), id.end(), 0u);
    auto find = [&](uint32_t x) {
        while (parent[x] != x) {
            parent[x] = parent[parent[x]];
            x = parent[x];
        }
        return x;
    };
    for (uint32_t e = 0; e + 1 < n; e++) {
        const uint32_t x = edges[2 * e], y = edges[2 * e + 1];
        if (weights[e] != weights[e] || (e && weights[e] < weights[e - 1]))
            return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_linkage_from_mst: edge %u: the weights must not decrease (or be NaN)", e);
        if (x >= n || y >= n)
            return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_linkage_from_mst: edge %u joins %u and %u of %u leaves (a forest has no tree)", e, x, y, n);
        const uint32_t a = find(x), b = find(y);
        if (a == b) return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_linkage_from_mst: edge %u (%u, %u) closes a cycle", e, x, y);
        pairs[2 * e] = std::min(id[a], id[b]);
        pairs[2 * e + 1] = std::max(id[a], id[b]);
        heights[e] = weights[e];
        parent[b] = a;
        size[a] += size[b];
        id[a] = n + e;
        sizes[e] = size[a];
    }
    return DVS_OK;
}
