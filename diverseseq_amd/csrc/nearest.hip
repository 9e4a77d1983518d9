// The k nearest references of every query (include/dvs_hip.h "nearest references"): cross_topk_kernel
// behind each strip of the strip driver (crossdist.hip dvs_strip_run).  No counterpart in the reference.
#include "dvs_internal.h"

#include <cmath>

namespace {

constexpr uint32_t NONE = DVS_NONE;

// The kk smallest cells of every row of a strip (mq x n) in ascending order of (distance, column): a tie goes to the
// lower column, so the answer is unique.  One workgroup per row, kk passes: pass t takes the least (distance, column)
// above the one pass t - 1 took -- every thread over its columns, then a fixed tree over the workgroup.  No atomics:
// the same bits and columns on every run.  NaN compares false with everything and is never taken; when fewer than kk
// cells are left the remaining slots get column NONE and distance NaN.  Rows of up to TOPK_LDS cells are read from
// HBM once.  (kk n reads per row against 4 096 bins x 16 f64 instructions, or 3 000 merge steps, per cell.)
constexpr int TOPK_THREADS = 256;
constexpr uint32_t TOPK_LDS = 2048;
__global__ __launch_bounds__(TOPK_THREADS) void cross_topk_kernel(const double *__restrict__ strip, uint32_t n, uint32_t kk,
                                                                  uint32_t *__restrict__ idx, double *__restrict__ val) {
    __shared__ double s_cells[TOPK_LDS];
    __shared__ double s_d[TOPK_THREADS / 64];
    __shared__ uint32_t s_j[TOPK_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *g = strip + uint64_t(blockIdx.x) * n;
    const bool in_lds = n <= TOPK_LDS;
    if (in_lds) {
        for (uint32_t j = tid; j < n; j += TOPK_THREADS) s_cells[j] = g[j];
        __syncthreads();
    }
    uint32_t *oi = idx + uint64_t(blockIdx.x) * kk;
    double *od = val + uint64_t(blockIdx.x) * kk;
    auto less = [](double d, uint32_t j, double e, uint32_t k2) { return d < e || (d == e && j < k2); };
    double ld = -INFINITY;  // the cell the previous pass took; nothing yet: every cell that is not NaN lies above it
    uint32_t lj = NONE;
    for (uint32_t t = 0; t < kk; t++) {
        double bd = INFINITY;
        uint32_t bj = NONE;
        for (uint32_t j = tid; j < n; j += TOPK_THREADS) {
            const double d = in_lds ? s_cells[j] : g[j];
            if ((d > ld || (d == ld && lj != NONE && j > lj)) && less(d, j, bd, bj)) {
                bd = d;
                bj = j;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double e = __shfl_xor(bd, o, 64);
            const uint32_t ej = __shfl_xor(bj, o, 64);
            if (less(e, ej, bd, bj)) {
                bd = e;
                bj = ej;
            }
        }
        __syncthreads();  // (the previous pass's readers)
        if (lane == 0) {
            s_d[wave] = bd;
            s_j[wave] = bj;
        }
        __syncthreads();
        bd = s_d[0];
        bj = s_j[0];
#pragma unroll
        for (int w = 1; w < TOPK_THREADS / 64; w++)
            if (less(s_d[w], s_j[w], bd, bj)) {
                bd = s_d[w];
                bj = s_j[w];
            }
        if (bj == NONE) {  // (the same for every thread) nothing left above the last one taken
            for (uint32_t u = t + tid; u < kk; u += TOPK_THREADS) {
                oi[u] = NONE;
                od[u] = NAN;
            }
            return;
        }
        if (tid == 0) {
            oi[t] = bj;
            od[t] = bd;
        }
        ld = bd;
        lj = bj;
    }
}

}  // namespace

// the kk nearest references of every query into the host arrays idx, dist (m x kk)
int dvs_nearest_strips(dvs_ctx *ctx, const dvs_cross_stage &st, uint32_t kk, uint32_t *idx, double *dist) {
    if (kk == 0 || kk > st.n)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "%u nearest of %u references: between 1 and the number of references", kk, st.n);
    if (kk > DVS_TOPK_MAX)
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "%u nearest: %u at most (a full ranking takes the matrix)", kk, DVS_TOPK_MAX);
    if (st.m == 0) return DVS_OK;
    if (!idx || !dist) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    PooledBuf d_idx{ctx}, d_val{ctx};
    dvs_strip_consumer c{};
    c.begin = [&](uint32_t rows) {
        const int rc = dvs_dev_alloc(ctx, &d_idx.p, size_t(rows) * kk * 4, "nearest references");
        return rc ? rc : dvs_dev_alloc(ctx, &d_val.p, size_t(rows) * kk * 8, "nearest distances");
    };
    c.strip = [&](uint32_t q0, uint32_t mq, double *d_strip) {
        hipLaunchKernelGGL(cross_topk_kernel, dim3(mq), dim3(TOPK_THREADS), 0, ctx->stream, d_strip, st.n, kk,
                           d_idx.as<uint32_t>(), d_val.as<double>());
        hipError_t e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync(idx + size_t(q0) * kk, d_idx.p, size_t(mq) * kk * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(dist + size_t(q0) * kk, d_val.p, size_t(mq) * kk * 8, hipMemcpyDeviceToHost, ctx->stream);
        return e;
    };
    return dvs_strip_run(ctx, st, c);
}
