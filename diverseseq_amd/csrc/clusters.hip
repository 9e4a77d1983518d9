// The scores of a labelling of the rows (include/dvs_hip.h "flat clusters"): cluster_scores_kernel behind
// each strip of the strip driver (crossdist.hip dvs_strip_run), the medoids on the host.  The cut that makes a labelling
// from a tree is a function of the tree alone and lives in linkage.hip.
#include "dvs_internal.h"

namespace {

constexpr uint32_t NONE = DVS_NONE;

// The scores of a labelling over the rows of a strip (mq x n; row r of the strip is position q0 + r of the n labelled
// positions, the columns are the same n positions): include/dvs_hip.h "flat clusters".  order[start[c] .. start[c + 1])
// lists the positions of cluster c in ascending order (a stable counting sort by label, once per call on the host).
// One workgroup per row; wave w takes the clusters c = w, w + 4, ...: its 64 lanes stride over the cluster's list and
// add the row's cells, the own position skipped (cell (i, i) is never read), a lane its cells in list order, the 64
// partials by the xor-shuffle tree -- an order that (n, labels) fix, so the strip height, the grid and the run cannot
// change a bit.  A wave keeps its own cluster's sum and the least mean of the others (ascending c, strict <: a tie
// stays with the lower c; a NaN mean compares false and is never taken) in registers; the four waves meet in LDS in
// wave order under the same rule.  No atomics; LDS does not grow with n or K.
constexpr int CLS_THREADS = 256;
constexpr uint32_t CLS_WAVES = CLS_THREADS / 64;
__global__ __launch_bounds__(CLS_THREADS) void cluster_scores_kernel(
    const double *__restrict__ strip, uint32_t n, uint32_t q0, const uint32_t *__restrict__ order,
    const uint32_t *__restrict__ start, const uint32_t *__restrict__ label, uint32_t n_clusters, double *__restrict__ within,
    double *__restrict__ a_out, double *__restrict__ b_out, uint32_t *__restrict__ neighbour, double *__restrict__ silhouette) {
    __shared__ double s_mean[CLS_WAVES];
    __shared__ uint32_t s_c[CLS_WAVES];
    __shared__ double s_own;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t self = q0 + blockIdx.x, own = label[self];
    const double *g = strip + uint64_t(blockIdx.x) * n;
    double best = NAN, own_sum = 0.0;
    uint32_t bc = NONE;
    for (uint32_t c = wave; c < n_clusters; c += CLS_WAVES) {
        const uint32_t p0 = start[c], p1 = start[c + 1];
        if (p0 == p1) continue;  // an empty cluster
        double s = 0.0;
#pragma unroll 4
        for (uint32_t p = p0 + lane; p < p1; p += 64) {
            const uint32_t j = order[p];
            if (j != self) s += g[j];
        }
        s = dvs_wave_sum(s);
        if (c == own) {
            own_sum = s;
        } else {
            const double mean = s / double(p1 - p0);
            if (bc == NONE ? mean == mean : mean < best) {
                best = mean;
                bc = c;
            }
        }
    }
    if (lane == 0) {
        s_mean[wave] = best;
        s_c[wave] = bc;
        if (own % CLS_WAVES == wave) s_own = own_sum;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    best = s_mean[0];
    bc = s_c[0];
#pragma unroll
    for (uint32_t w = 1; w < CLS_WAVES; w++) {
        const double e = s_mean[w];
        const uint32_t ec = s_c[w];
        if (ec != NONE && (bc == NONE || e < best || (e == best && ec < bc))) {
            best = e;
            bc = ec;
        }
    }
    const uint32_t size = start[own + 1] - start[own];
    const double w_i = s_own, a = size > 1 ? w_i / double(size - 1) : 0.0, b = bc == NONE ? NAN : best;
    double sil = 0.0;
    if (size > 1 && !(a == 0.0 && b == 0.0)) sil = (b - a) / (a > b ? a : b);
    within[blockIdx.x] = w_i;
    a_out[blockIdx.x] = a;
    b_out[blockIdx.x] = b;
    neighbour[blockIdx.x] = bc;
    silhouette[blockIdx.x] = sil;
}

}  // namespace

// The scores of a labelling over a stage whose queries and references are the same n positions: the positions sorted
// by label once (a stable counting sort: order, start) and uploaded in front of the first strip, cluster_scores_kernel
// behind each strip's distances, its five outputs copied out strip by strip; the medoids from the n sums on the host.
int dvs_cluster_scores_strips(dvs_ctx *ctx, const dvs_cross_stage &st, const uint32_t *labels, uint32_t n_clusters,
                              double *within, double *a, double *b, uint32_t *neighbour, double *silhouette,
                              uint32_t *medoids) {
    const uint32_t n = st.n;
    if (n == 0) return DVS_OK;
    if (!labels || !within) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    for (uint32_t i = 0; i < n; i++)
        if (labels[i] >= n_clusters)
            return dvs_set_error(ctx, DVS_ERR_VALUE, "row %u carries label %u: below the number of clusters (%u)", i,
                                 labels[i], n_clusters);
    // one block: order [n], start [K + 1], label [n], then per strip row four doubles and the neighbour
    const size_t o_start = size_t(n) * 4, o_label = o_start + (size_t(n_clusters) + 1) * 4;
    const size_t o_out = (o_label + size_t(n) * 4 + 7) / 8 * 8;
    PooledBuf d_buf{ctx};
    std::vector<uint32_t> start, order;
    uint32_t *d_order, *d_start, *d_label, *d_nb;
    double *d_within, *d_a, *d_b, *d_sil;
    dvs_strip_consumer c{};
    c.begin = [&](uint32_t rows) {
        start.assign(size_t(n_clusters) + 1, 0);
        order.resize(n);
        for (uint32_t i = 0; i < n; i++) start[labels[i] + 1]++;
        for (uint32_t k = 0; k < n_clusters; k++) start[k + 1] += start[k];
        std::vector<uint32_t> next(start.begin(), start.end() - 1);
        for (uint32_t i = 0; i < n; i++) order[next[labels[i]]++] = i;
        if (int rc = dvs_dev_alloc(ctx, &d_buf.p, o_out + size_t(rows) * 36, "cluster lists and scores")) return rc;
        char *base = d_buf.as<char>();
        d_order = reinterpret_cast<uint32_t *>(base), d_start = reinterpret_cast<uint32_t *>(base + o_start);
        d_label = reinterpret_cast<uint32_t *>(base + o_label);
        d_within = reinterpret_cast<double *>(base + o_out), d_a = d_within + rows, d_b = d_a + rows, d_sil = d_b + rows;
        d_nb = reinterpret_cast<uint32_t *>(d_sil + rows);
        hipError_t e = hipMemcpyAsync(d_order, order.data(), size_t(n) * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_start, start.data(), start.size() * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_label, labels, size_t(n) * 4, hipMemcpyHostToDevice, ctx->stream);
        return e == hipSuccess ? DVS_OK : dvs_hip_fail(ctx, e, "cluster lists upload");
    };
    c.strip = [&](uint32_t q0, uint32_t mq, double *d_strip) {
        hipLaunchKernelGGL(cluster_scores_kernel, dim3(mq), dim3(CLS_THREADS), 0, ctx->stream, d_strip, n, q0, d_order,
                           d_start, d_label, n_clusters, d_within, d_a, d_b, d_nb, d_sil);
        hipError_t ce = hipGetLastError();
        auto out = [&](void *host, const void *dev, size_t width) {
            if (ce == hipSuccess && host)
                ce = hipMemcpyAsync(static_cast<char *>(host) + size_t(q0) * width, dev, size_t(mq) * width,
                                    hipMemcpyDeviceToHost, ctx->stream);
        };
        out(within, d_within, 8);
        out(a, d_a, 8);
        out(b, d_b, 8);
        out(silhouette, d_sil, 8);
        out(neighbour, d_nb, 4);
        return ce;
    };
    if (int rc = dvs_strip_run(ctx, st, c)) return rc;
    if (medoids) {
        for (uint32_t k = 0; k < n_clusters; k++) {
            uint32_t best = NONE;
            for (uint32_t p = start[k]; p < start[k + 1]; p++) {  // ascending rows: strict < keeps the lowest of a tie
                const uint32_t i = order[p];
                if (within[i] == within[i] && (best == NONE || within[i] < within[best])) best = i;
            }
            medoids[k] = best;
        }
    }
    return DVS_OK;
}
