// Pairwise Jensen-Shannon divergence of the rows of a k-mer matrix:
//   D[i][j] = H((f_i + f_j) / 2) - (H(f_i) + H(f_j)) / 2,   f = counts / total, H in bits,
// the total_jsd of the two-member set SummedRecords::new([i, j]) (src/records.rs:27-68; paper/paper.md Table 1:
// identical -> 0, no k-mer in common -> 1).  The divergence itself, not its square root.
//
// Two kernels.  jsd_pairs_kernel takes one 32 x 32 tile of the lower triangle per workgroup, the diagonal tiles
// included: the halved frequencies of its 32 i-rows and 32 j-rows are staged in LDS 64 bins at a time (one correctly
// rounded quotient per staged count, exact_div_u32), every thread owns a 2 x 2 block of pairs and adds
// -m log2 m (m = f_i / 2 + f_j / 2, log2_tab through a 2 KB table filled once per workgroup) for its four pairs bin
// after bin: four LDS reads feed four logarithms, and a count read from HBM feeds 32 pairs.  A pair below the diagonal
// leaves H(mean) in its cell; a pair ON the diagonal has mean == f_i, so its sum is H(f_i), written to d_h: the row
// entropies come out of the very expression and bin order of H(mean), once per row.  jsd_finish_kernel then turns
// every cell below the diagonal into the clamped divergence and mirrors it through an LDS transpose.  Two rows with
// equal counts have mean == f_i == f_j bit for bit, H(mean) == H(f_i) == H(f_j), and their cell is exactly 0.
// Each pair is summed by one thread in bin order: no atomics, no cross-lane sums, the same bits on every run and in
// both entries.  A row without a valid k-mer (total 0) is staged as zeros and gets NaN off the diagonal from the
// finish kernel, as euclid_kernel's 0 / 0 does.
//
// The kernel is bound by FP64 issue: 16 f64 instructions and one 16-byte table read per bin and pair, against four
// 8-byte LDS reads per bin and thread and one staged count per 32 pairs (DESIGN.md 4.8 has the measurements).
#include "dvs_internal.h"
#include "select_dev.h"

#include <type_traits>

namespace {

constexpr int JSD_THREADS = 256;
constexpr uint32_t JSD_TILE = 32;    // rows of a tile on either side; a thread owns rows t, t + 16 of both
constexpr uint32_t JSD_CHUNK = 64;   // bins staged at a time
constexpr uint32_t JSD_LD = 2 * JSD_TILE + 1;  // doubles per staged bin: 32 i-rows, 32 j-rows, one of padding

// acc -= m log2 m.  An empty bin (m == 0) takes the logarithm of 2^-1000 instead and adds -0 * -1000, which leaves
// acc as it is: no branch, so the chains of a thread's 2 x 2 block interleave.  (A count row's m is 0 or >= 2^-33.)
__device__ __forceinline__ void jsd_add(double &acc, double m, const double2 *tab) {
    acc = fma(-m, log2_tab(fmax(m, 0x1p-1000), tab), acc);
}

template <typename T>
__global__ __launch_bounds__(JSD_THREADS) void jsd_pairs_kernel(const T *__restrict__ mat,
                                                                const uint32_t *__restrict__ totals, uint64_t B,
                                                                uint32_t n, double *__restrict__ dist,
                                                                double *__restrict__ d_h) {
    __shared__ double2 tab[128];
    __shared__ double s_f[JSD_CHUNK * JSD_LD];  // s_f[b * JSD_LD + r]: half the frequency of tile row r in bin b
    __shared__ double s_tot[2 * JSD_TILE], s_rt[2 * JSD_TILE];
    const uint32_t bi = blockIdx.x, bj = blockIdx.y;
    if (bj > bi) return;  // above the diagonal
    const uint32_t tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    if (tid < 128) log2_tab_fill(tab, int(tid));
    if (tid < 2 * JSD_TILE) {
        const uint32_t row = tid < JSD_TILE ? bi * JSD_TILE + tid : bj * JSD_TILE + (tid - JSD_TILE);
        const double t = row < n ? double(totals[row]) : 0.0;
        s_tot[tid] = t;
        s_rt[tid] = t > 0.0 ? 1.0 / t : 0.0;
    }
    double acc00 = 0.0, acc01 = 0.0, acc10 = 0.0, acc11 = 0.0;  // acc[a][b]: rows ty + 16 a and tx + 16 b
    const uint32_t sb = tid & (JSD_CHUNK - 1), sr0 = tid / JSD_CHUNK;  // staging: bin sb of rows sr0, sr0 + 4, ...
    for (uint64_t c0 = 0; c0 < B; c0 += JSD_CHUNK) {
        const uint32_t cn = uint32_t(B - c0 < JSD_CHUNK ? B - c0 : JSD_CHUNK);
        __syncthreads();  // (the table and the totals the first time; the previous chunk's readers after that)
        if (sb < cn) {
#pragma unroll 4
            for (uint32_t r = sr0; r < 2 * JSD_TILE; r += JSD_THREADS / JSD_CHUNK) {
                const uint32_t row = r < JSD_TILE ? bi * JSD_TILE + r : bj * JSD_TILE + (r - JSD_TILE);
                const double t = s_tot[r];
                double f = 0.0;
                if (row < n && t > 0.0) f = 0.5 * count_freq_x(mat[uint64_t(row) * B + c0 + sb], t, s_rt[r]);
                s_f[sb * JSD_LD + r] = f;
            }
        }
        __syncthreads();
#pragma unroll 2
        for (uint32_t b = 0; b < cn; b++) {
            const double *s = s_f + b * JSD_LD;
            const double i0 = s[ty], i1 = s[ty + 16], j0 = s[JSD_TILE + tx], j1 = s[JSD_TILE + tx + 16];
            jsd_add(acc00, i0 + j0, tab);
            jsd_add(acc01, i0 + j1, tab);
            jsd_add(acc10, i1 + j0, tab);
            jsd_add(acc11, i1 + j1, tab);
        }
    }
    const double acc[2][2] = {{acc00, acc01}, {acc10, acc11}};
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const uint32_t i = bi * JSD_TILE + ty + 16 * a, j = bj * JSD_TILE + tx + 16 * b;
            if (i >= n || j > i) continue;
            if (i == j) d_h[i] = acc[a][b];  // H(f_i)
            else dist[uint64_t(i) * n + j] = acc[a][b];  // H(mean), finished below
        }
}

// below the diagonal: H(mean) -> the divergence, clamped to [0, 1] (NaN where a row has no valid k-mer); the mirror
// cell through an LDS transpose; 0 on the diagonal
__global__ __launch_bounds__(JSD_THREADS) void jsd_finish_kernel(const uint32_t *__restrict__ totals,
                                                                 const double *__restrict__ d_h, uint32_t n,
                                                                 double *__restrict__ dist) {
    __shared__ double t[JSD_TILE][JSD_TILE + 1];
    const uint32_t bi = blockIdx.x, bj = blockIdx.y;
    if (bj > bi) return;
    const uint32_t lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (uint32_t q = ly; q < JSD_TILE; q += JSD_THREADS / 32) {
        const uint32_t i = bi * JSD_TILE + q, j = bj * JSD_TILE + lx;
        double d = 0.0;
        if (i < n && j < i) {
            d = dist[uint64_t(i) * n + j] - 0.5 * (d_h[i] + d_h[j]);
            d = d < 0.0 ? 0.0 : d;
            d = d > 1.0 ? 1.0 : d;
            if (totals[i] == 0 || totals[j] == 0) d = NAN;
            dist[uint64_t(i) * n + j] = d;
        } else if (i < n && j == i) {
            dist[uint64_t(i) * n + j] = 0.0;
        }
        t[q][lx] = d;
    }
    __syncthreads();
    for (uint32_t q = ly; q < JSD_TILE; q += JSD_THREADS / 32) {
        const uint32_t j = bj * JSD_TILE + q, i = bi * JSD_TILE + lx;  // cell (j, i) above the diagonal
        if (i < n && j < i) dist[uint64_t(j) * n + i] = t[lx][q];
    }
}

struct PooledBuf {  // a block of the context's cache, handed back on scope exit
    dvs_ctx *ctx;
    void *p = nullptr;
    ~PooledBuf() { dvs_dev_free(ctx, p); }
    template <typename T>
    T *as() { return static_cast<T *>(p); }
};

// both kernels over the rows of m into the device matrix d_dist (every cell, the diagonal included); d_h: n doubles
hipError_t jsd_launch(dvs_ctx *ctx, const dvs_matrix *m, double *d_dist, double *d_h) {
    const uint32_t n = m->nrows, tiles = (n + JSD_TILE - 1) / JSD_TILE;
    const dim3 grid(tiles, tiles);
    dvs_mat_dispatch(m, [&](auto *mp) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(mp)>>;
        hipLaunchKernelGGL((jsd_pairs_kernel<T>), grid, dim3(JSD_THREADS), 0, ctx->stream, mp, m->d_totals, m->nbins, n,
                           d_dist, d_h);
        return 0;
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(jsd_finish_kernel, grid, dim3(JSD_THREADS), 0, ctx->stream, m->d_totals, d_h, n, d_dist);
    return hipGetLastError();
}

// the size limit of dvs_euclidean_distances (eight rows per workgroup, 65 535 workgroups in y)
bool jsd_too_many_rows(uint32_t n) { return (n + 7) / 8 > 65535u; }

}  // namespace

extern "C" int dvs_jsd_distances(dvs_ctx *ctx, const dvs_matrix *m, double *dist) {
    if (!ctx || !m || !dist) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    const uint32_t n = m->nrows;
    if (n == 0) return DVS_OK;
    if (n == 1) {
        dist[0] = 0.0;
        return DVS_OK;
    }
    if (jsd_too_many_rows(n))
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "%u rows: the %u x %u distance matrix is beyond this path", n, n, n);
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    PooledBuf d_dist{ctx}, d_h{ctx};
    int rc = dvs_dev_alloc(ctx, &d_dist.p, size_t(n) * n * 8, "distance matrix");
    if (!rc) rc = dvs_dev_alloc(ctx, &d_h.p, size_t(n) * 8, "row entropies");
    if (rc) return rc;
    hipError_t e = jsd_launch(ctx, m, d_dist.as<double>(), d_h.as<double>());
    if (e == hipSuccess) e = hipMemcpyAsync(dist, d_dist.p, size_t(n) * n * 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t se = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, "jsd distances");
    if (se != hipSuccess) return dvs_hip_fail(ctx, se, "jsd distances");
    return DVS_OK;
}

extern "C" int dvs_matrix_jsd_linkage(dvs_ctx *ctx, const dvs_matrix *m, int method, uint32_t *pairs, double *heights,
                                      uint32_t *sizes) {
    if (!ctx || !m || !pairs || !heights || !sizes) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (int rc = dvs_linkage_check_method(ctx, method)) return rc;
    const uint32_t n = m->nrows;
    if (n < 2) return dvs_set_error(ctx, DVS_ERR_VALUE, "need at least two sequences to build a tree");
    if (jsd_too_many_rows(n))
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "%u rows: the %u x %u distance matrix is beyond this path", n, n, n);
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    PooledBuf d_dist{ctx}, d_h{ctx};
    int rc = dvs_linkage_check_size(ctx, n);
    if (!rc) rc = dvs_dev_alloc(ctx, &d_dist.p, size_t(n) * n * 8, "distance matrix");
    if (!rc) rc = dvs_dev_alloc(ctx, &d_h.p, size_t(n) * 8, "row entropies");
    if (rc) return rc;
    const hipError_t e = jsd_launch(ctx, m, d_dist.as<double>(), d_h.as<double>());
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->stream);
        return dvs_hip_fail(ctx, e, "jsd distances");
    }
    return dvs_linkage_device(ctx, d_dist.as<double>(), n, nullptr, method, pairs, heights, sizes);
}
