// The cophenetic correlation of a tree with the distances it was built from (include/dvs_hip.h "cophenetic distances",
// DESIGN.md 4.11): cophenet_kernel behind each strip of the strip driver (crossdist.hip dvs_strip_run), Pearson's r on the
// host.  The in-order walk of the tree (dvs_cophenet_walk) is a function of the tree alone and lives in linkage.hip.
#include "dvs_internal.h"

#include <algorithm>
#include <cmath>

namespace {

// The five shifted moments of a row of distances against the same row of cophenetic distances (include/dvs_hip.h
// "cophenetic distances"; strip as for cluster_scores_kernel: row r is position q0 + r of the n leaves).  order, pos,
// gap: the tree's in-order walk.  One workgroup per row, at p = pos[self]: the positions to the right of p, then those
// to the left, COPH_CHUNK at a time and COPH_ITEMS consecutive ones per thread, under a running inclusive maximum of
// the gaps crossed since p -- a thread over its own items, the 64 lanes by shuffle-up, the waves and the chunks before
// through a carry in LDS (an integer maximum: exact in any shape).  Position q then has c = heights[that maximum] and
// d = strip[row n + order[q]]; x = d - c_bar, y = c - c_bar go into the thread's five sums in position order, the 256
// partials meet in the xor-shuffle tree and in wave order in LDS: an order that (n, the tree) fix.  Cell (i, i) is
// never read.  No atomics; LDS does not grow with n.  sums[a * rows + r]; coph_strip (may be NULL): row r's cophenetic
// distances by column, 0 on the diagonal.
constexpr int COPH_THREADS = 256, COPH_ITEMS = 4;
constexpr uint32_t COPH_WAVES = COPH_THREADS / 64, COPH_CHUNK = COPH_THREADS * COPH_ITEMS;
__global__ __launch_bounds__(COPH_THREADS) void cophenet_kernel(
    const double *__restrict__ strip, uint32_t n, uint32_t q0, const uint32_t *__restrict__ order,
    const uint32_t *__restrict__ pos, const uint32_t *__restrict__ gap, const double *__restrict__ heights, double c_bar,
    uint32_t rows, double *__restrict__ sums, double *__restrict__ coph_strip) {
    __shared__ uint32_t s_top[2][COPH_WAVES];
    __shared__ double s_part[5][COPH_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t self = q0 + blockIdx.x, p = pos[self];
    const double *g = strip + uint64_t(blockIdx.x) * n;
    double *cg = coph_strip ? coph_strip + uint64_t(blockIdx.x) * n : nullptr;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // x, y, x x, y y, x y
    uint32_t flip = 0;
#pragma unroll 1
    for (int side = 0; side < 2; side++) {
        const uint32_t count = side == 0 ? n - 1 - p : p;  // positions on this side of p; offset t: p + 1 + t, or p - 1 - t
        uint32_t carry = 0;                                // the maximum over the chunks before
#pragma unroll 1
        for (uint32_t c0 = 0; c0 < count; c0 += COPH_CHUNK) {
            const uint32_t t0 = c0 + tid * COPH_ITEMS;
            uint32_t m[COPH_ITEMS], col[COPH_ITEMS];
#pragma unroll
            for (int k = 0; k < COPH_ITEMS; k++) {
                const uint32_t t = t0 + k;
                const bool live = t < count;
                const uint32_t q = side == 0 ? p + 1 + t : p - 1 - t;  // (the gap crossed on the way: q - 1, or q)
                m[k] = live ? gap[side == 0 ? q - 1 : q] : 0u;
                col[k] = live ? order[q] : 0u;
            }
#pragma unroll
            for (int k = 1; k < COPH_ITEMS; k++) m[k] = max(m[k], m[k - 1]);
            uint32_t w = m[COPH_ITEMS - 1];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t u = __shfl_up(w, o, 64);
                if (lane >= uint32_t(o)) w = max(w, u);
            }
            if (lane == 63) s_top[flip][wave] = w;
            __syncthreads();  // (two buffers: the writers of the chunk after next have passed the next chunk's barrier)
            uint32_t before = carry;  // everything between p and this thread's first item
#pragma unroll
            for (uint32_t x = 0; x < COPH_WAVES; x++) {
                const uint32_t top = s_top[flip][x];
                if (x < wave) before = max(before, top);
                carry = max(carry, top);
            }
            const uint32_t left = __shfl_up(w, 1, 64);
            if (lane > 0) before = max(before, left);
            flip ^= 1;
#pragma unroll
            for (int k = 0; k < COPH_ITEMS; k++) {
                if (t0 + k >= count) continue;
                const double c = heights[max(m[k], before)], d = g[col[k]];
                const double x = d - c_bar, y = c - c_bar;
                acc[0] += x;
                acc[1] += y;
                acc[2] += x * x;
                acc[3] += y * y;
                acc[4] += x * y;
                if (cg) cg[col[k]] = c;
            }
        }
    }
    if (cg && tid == 0) cg[self] = 0.0;
#pragma unroll
    for (int a = 0; a < 5; a++) {
        const double v = dvs_wave_sum(acc[a]);
        if (lane == 0) s_part[a][wave] = v;
    }
    __syncthreads();
    if (tid < 5) {
        double v = s_part[tid][0];
#pragma unroll
        for (uint32_t x = 1; x < COPH_WAVES; x++) v += s_part[tid][x];
        sums[size_t(tid) * rows + blockIdx.x] = v;
    }
}

// Pearson's r from the 5 n shifted row sums ([5][n]: x, y, x x, y y, x y), in long double: NaN when either centred sum
// of squares is not above the rounding error of its own terms (n = 2, a constant matrix: scipy's 0 / 0)
double cophenet_correlation(const double *row_sums, uint32_t n) {
    long double s[5];
    for (int a = 0; a < 5; a++) {
        s[a] = 0.0L;
        for (uint32_t i = 0; i < n; i++) s[a] += (long double)row_sums[size_t(a) * n + i];
    }
    const long double M = (long double)n * (long double)(n - 1);
    const long double sxx = s[2] - s[0] * s[0] / M, syy = s[3] - s[1] * s[1] / M, sxy = s[4] - s[0] * s[1] / M;
    const long double eps = 2.0L * ((long double)n + 8.0L) * 0x1p-52L;
    if (!(sxx > eps * s[2]) || !(syy > eps * s[3])) return NAN;
    return double(sxy / sqrtl(sxx * syy));
}

}  // namespace

// The cophenetic correlation of a tree over a stage whose queries and references are the tree's n leaves: the in-order
// walk on the host, its three lists and the heights uploaded in front of the first strip in one pooled block that also
// holds the strip's 5 sums per row; cophenet_kernel behind each strip's distances, the sums (and, when asked for, the
// cophenetic rows, from a second strip buffer) copied out strip by strip; r from the 5 n sums on the host.
int dvs_cophenet_strips(dvs_ctx *ctx, const dvs_cross_stage &st, const uint32_t *pairs, const double *heights, double *corr,
                        double *row_sums, double *coph) {
    const uint32_t n = st.n;
    if (n == 0) return DVS_OK;
    if (!pairs || !heights || !corr) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (int rc = dvs_rows_check(ctx, n)) return rc;  // (bounds the walk's vectors, too)
    // one block: order [n], pos [n], gap [n - 1], then the heights [n - 1], then per strip row five doubles
    const size_t o_pos = size_t(n) * 4, o_gap = o_pos + size_t(n) * 4;
    const size_t o_h = (o_gap + size_t(n - 1) * 4 + 7) / 8 * 8, o_out = o_h + size_t(n - 1) * 8;
    std::vector<uint64_t> host((o_out + 7) / 8);
    char *hb = reinterpret_cast<char *>(host.data());
    double c_bar = 0.0;
    if (int rc = dvs_cophenet_walk(ctx, n, pairs, heights, reinterpret_cast<uint32_t *>(hb), reinterpret_cast<uint32_t *>(hb + o_pos),
                                   reinterpret_cast<uint32_t *>(hb + o_gap), &c_bar))
        return rc;
    std::copy(heights, heights + (n - 1), reinterpret_cast<double *>(hb + o_h));
    std::vector<double> own_sums;
    PooledBuf d_buf{ctx}, d_coph{ctx};
    uint32_t rows = 0;
    dvs_strip_consumer c{};
    c.begin = [&](uint32_t strip_rows) {
        rows = strip_rows;
        if (!row_sums) {
            own_sums.resize(size_t(5) * n);
            row_sums = own_sums.data();
        }
        int rc = dvs_dev_alloc(ctx, &d_buf.p, o_out + size_t(rows) * 40, "tree lists and row sums");
        if (!rc && coph) rc = dvs_dev_alloc(ctx, &d_coph.p, size_t(rows) * n * 8, "cophenetic strip");
        if (rc) return rc;
        const hipError_t e = hipMemcpyAsync(d_buf.p, hb, o_out, hipMemcpyHostToDevice, ctx->stream);
        return e == hipSuccess ? DVS_OK : dvs_hip_fail(ctx, e, "tree lists upload");
    };
    c.strip = [&](uint32_t q0, uint32_t mq, double *d_strip) {
        char *base = d_buf.as<char>();
        const uint32_t *d_order = reinterpret_cast<uint32_t *>(base), *d_pos = reinterpret_cast<uint32_t *>(base + o_pos),
                       *d_gap = reinterpret_cast<uint32_t *>(base + o_gap);
        const double *d_heights = reinterpret_cast<double *>(base + o_h);
        double *d_sums = reinterpret_cast<double *>(base + o_out);
        hipLaunchKernelGGL(cophenet_kernel, dim3(mq), dim3(COPH_THREADS), 0, ctx->stream, d_strip, n, q0, d_order, d_pos,
                           d_gap, d_heights, c_bar, rows, d_sums, d_coph.as<double>());
        hipError_t ce = hipGetLastError();
        for (int a = 0; a < 5 && ce == hipSuccess; a++)
            ce = hipMemcpyAsync(row_sums + size_t(a) * n + q0, d_sums + size_t(a) * rows, size_t(mq) * 8,
                                hipMemcpyDeviceToHost, ctx->stream);
        if (ce == hipSuccess && coph)
            ce = hipMemcpyAsync(coph + size_t(q0) * n, d_coph.p, size_t(mq) * n * 8, hipMemcpyDeviceToHost, ctx->stream);
        return ce;
    };
    if (int rc = dvs_strip_run(ctx, st, c)) return rc;
    *corr = cophenet_correlation(row_sums, n);
    return DVS_OK;
}
