// Distances between two collections -- M query rows against N reference rows -- in the three modes of the square
// path (rowdist.hip, mash.hip), and the k nearest references of every query.  No counterpart in the reference, whose
// distance functions fill the N x N matrix of one collection (diverse_seq/distance.py:119-175, 294-336).
//
// A cell is the square path's cell for the same two rows, bit for bit: the Jensen-Shannon kernel keeps the tile of
// jsd_pairs_kernel (32 x 32 pairs per workgroup, 64 bins staged at a time in the 65-double LDS row, a 2 x 2 block of
// pairs per thread, jsd_add per bin in bin order) with the 32 i-rows taken from the queries and the 32 j-rows from the
// references; it has no diagonal tiles and no mirror, so it finishes its cells itself.  The row entropies the square
// kernel reads off its diagonal pairs come from jsd_entropy_kernel: the same expression (mean == f_i + f_i halved
// twice) summed in the same bin order by one thread per row.  The euclidean kernel is euclid_kernel with row i from
// the queries; the mash kernel is another wrapper of the one merge in mash.hip.
//
// The M x N matrix never has to exist whole: a stage (dvs_cross_stage) fills rows [q0, q0 + mq) into a strip, and the
// drivers walk the queries strip by strip -- to the host matrix, through cross_topk_kernel to the kk nearest
// references per query, or (queries = references) through cluster_scores_kernel to the scores of a labelling of the
// rows, or through cophenet_kernel to the correlation of the distances with a tree's cophenetic distances, or through the
// within_* kernels to the list of the cells within a radius and (queries = references) the connected components they
// make.  The strip is CROSS_STRIP_BYTES at most (and a tile row of 32 queries at least).
#include "dvs_internal.h"
#include "rowdist_dev.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <type_traits>
#include <vector>

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr size_t CROSS_STRIP_BYTES = size_t(256) << 20;  // the strip buffer's bound
constexpr uint32_t TOPK_MAX = 64;

// H(f) of the rows rows[p] (NULL: p), p < count, by the pair kernels' own expression and bin order: what
// jsd_pairs_kernel leaves in d_h for a pair on the diagonal.  One wave per 64 rows: a lane stages one bin of the 64
// rows at a time (consecutive lanes, consecutive bins: coalesced) and then sums its own row.
template <typename T>
__global__ __launch_bounds__(64) void jsd_entropy_kernel(const T *__restrict__ mat, const uint32_t *__restrict__ totals,
                                                         const uint32_t *__restrict__ rows, uint32_t count, uint64_t B,
                                                         double *__restrict__ h) {
    __shared__ double2 tab[128];
    __shared__ double s_f[JSD_CHUNK * JSD_LD];
    __shared__ double s_tot[64], s_rt[64];
    __shared__ uint32_t s_row[64];
    const uint32_t tid = threadIdx.x, p = blockIdx.x * 64 + tid;
    log2_tab_fill(tab, int(tid));
    log2_tab_fill(tab, int(tid) + 64);
    {
        const uint32_t row = p < count ? (rows ? rows[p] : p) : NONE;
        const double t = row != NONE ? double(totals[row]) : 0.0;
        s_row[tid] = row;
        s_tot[tid] = t;
        s_rt[tid] = t > 0.0 ? 1.0 / t : 0.0;
    }
    double acc = 0.0;
    for (uint64_t c0 = 0; c0 < B; c0 += JSD_CHUNK) {
        const uint32_t cn = uint32_t(B - c0 < JSD_CHUNK ? B - c0 : JSD_CHUNK);
        __syncthreads();
        if (tid < cn) {
#pragma unroll 8
            for (uint32_t r = 0; r < 64; r++) {
                const uint32_t row = s_row[r];
                const double t = s_tot[r];
                double f = 0.0;
                if (row != NONE && t > 0.0) f = 0.5 * count_freq_x(mat[uint64_t(row) * B + c0 + tid], t, s_rt[r]);
                s_f[tid * JSD_LD + r] = f;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (uint32_t b = 0; b < cn; b++) {
            const double f = s_f[b * JSD_LD + tid];
            jsd_add(acc, f + f, tab);
        }
    }
    if (p < count) h[p] = acc;
}

// Tile (bi, bj): queries q0 + 32 bi .. + 31 of the query list against references 32 bj .. + 31 of the reference list.
// hq[q0 + i], hr[j]: the row entropies above.  Cell (i, j) of the strip (mq x n): the clamped divergence, NaN where
// either row has no valid k-mer.
template <typename T, typename U>
__global__ __launch_bounds__(JSD_THREADS) void jsd_cross_kernel(
    const T *__restrict__ qmat, const uint32_t *__restrict__ qtot, const uint32_t *__restrict__ qrows, uint32_t q0,
    uint32_t mq, const U *__restrict__ rmat, const uint32_t *__restrict__ rtot, const uint32_t *__restrict__ rrows,
    uint32_t n, uint64_t B, const double *__restrict__ hq, const double *__restrict__ hr, double *__restrict__ strip) {
    __shared__ double2 tab[128];
    __shared__ double s_f[JSD_CHUNK * JSD_LD];  // s_f[b * JSD_LD + r]: half the frequency of tile row r in bin b
    __shared__ double s_tot[2 * JSD_TILE], s_rt[2 * JSD_TILE];
    __shared__ uint32_t s_row[2 * JSD_TILE];  // the matrix row behind tile row r (NONE: beyond the strip / the list)
    const uint32_t bi = blockIdx.x, bj = blockIdx.y;
    const uint32_t tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    if (tid < 128) log2_tab_fill(tab, int(tid));
    if (tid < 2 * JSD_TILE) {
        uint32_t row = NONE;
        double t = 0.0;
        if (tid < JSD_TILE) {
            const uint32_t i = bi * JSD_TILE + tid;
            if (i < mq) {
                row = qrows ? qrows[q0 + i] : q0 + i;
                t = double(qtot[row]);
            }
        } else {
            const uint32_t j = bj * JSD_TILE + (tid - JSD_TILE);
            if (j < n) {
                row = rrows ? rrows[j] : j;
                t = double(rtot[row]);
            }
        }
        s_row[tid] = row;
        s_tot[tid] = t;
        s_rt[tid] = t > 0.0 ? 1.0 / t : 0.0;
    }
    double acc00 = 0.0, acc01 = 0.0, acc10 = 0.0, acc11 = 0.0;  // acc[a][b]: rows ty + 16 a and tx + 16 b
    const uint32_t sb = tid & (JSD_CHUNK - 1), sr0 = tid / JSD_CHUNK;  // staging: bin sb of rows sr0, sr0 + 4, ...
    for (uint64_t c0 = 0; c0 < B; c0 += JSD_CHUNK) {
        const uint32_t cn = uint32_t(B - c0 < JSD_CHUNK ? B - c0 : JSD_CHUNK);
        __syncthreads();  // (the table, the rows and the totals the first time; the previous chunk's readers after that)
        if (sb < cn) {
#pragma unroll 4
            for (uint32_t r = sr0; r < JSD_TILE; r += JSD_THREADS / JSD_CHUNK) {  // the query rows
                const uint32_t row = s_row[r];
                const double t = s_tot[r];
                double f = 0.0;
                if (row != NONE && t > 0.0) f = 0.5 * count_freq_x(qmat[uint64_t(row) * B + c0 + sb], t, s_rt[r]);
                s_f[sb * JSD_LD + r] = f;
            }
#pragma unroll 4
            for (uint32_t r = JSD_TILE + sr0; r < 2 * JSD_TILE; r += JSD_THREADS / JSD_CHUNK) {  // the reference rows
                const uint32_t row = s_row[r];
                const double t = s_tot[r];
                double f = 0.0;
                if (row != NONE && t > 0.0) f = 0.5 * count_freq_x(rmat[uint64_t(row) * B + c0 + sb], t, s_rt[r]);
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
            const uint32_t li = ty + 16 * a, lj = tx + 16 * b;
            const uint32_t i = bi * JSD_TILE + li, j = bj * JSD_TILE + lj;
            if (i >= mq || j >= n) continue;
            double d = acc[a][b] - 0.5 * (hq[q0 + i] + hr[j]);  // (jsd_finish_kernel's expression)
            d = d < 0.0 ? 0.0 : d;
            d = d > 1.0 ? 1.0 : d;
            if (s_tot[li] == 0.0 || s_tot[JSD_TILE + lj] == 0.0) d = NAN;
            strip[uint64_t(i) * n + j] = d;
        }
}

// euclid_kernel with row i from the queries: workgroup (i, g) stages query q0 + i in LDS chunk by chunk and its eight
// waves take the references 8 g .. 8 g + 7, one each.
template <typename T, typename U>
__global__ __launch_bounds__(EUC_THREADS) void euclid_cross_kernel(
    const T *__restrict__ qmat, const uint32_t *__restrict__ qtot, const uint32_t *__restrict__ qrows, uint32_t q0,
    const U *__restrict__ rmat, const uint32_t *__restrict__ rtot, const uint32_t *__restrict__ rrows, uint32_t n,
    uint64_t B, double *__restrict__ strip) {
    __shared__ double fi[EUC_CHUNK];
    const uint32_t i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t j = blockIdx.y * (EUC_THREADS / 64) + wave;
    const bool live = j < n;
    const uint32_t qrow = qrows ? qrows[q0 + i] : q0 + i;
    const uint32_t jj = live ? j : 0u, rrow = rrows ? rrows[jj] : jj;
    const T *a = qmat + uint64_t(qrow) * B;
    const U *b = rmat + uint64_t(rrow) * B;
    const double ta = double(qtot[qrow]), tb = double(rtot[rrow]);
    double acc = 0.0;
    for (uint64_t c0 = 0; c0 < B; c0 += EUC_CHUNK) {
        const uint32_t cn = uint32_t(B - c0 < EUC_CHUNK ? B - c0 : EUC_CHUNK);
        __syncthreads();
        for (uint32_t x = threadIdx.x; x < cn; x += EUC_THREADS) fi[x] = double(a[c0 + x]) / ta;
        __syncthreads();
        if (live)
            for (uint32_t x = lane; x < cn; x += 64) {
                const double d = fi[x] - double(b[c0 + x]) / tb;
                acc += d * d;
            }
    }
    acc = dvs_wave_sum(acc);
    if (live && lane == 0) strip[uint64_t(i) * n + j] = sqrt(acc);
}

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

// Gower's add-a-point formula over the rows of a strip (mq x n): include/dvs_hip.h "principal coordinates".  Row r of the
// strip holds a query's distances delta_j to the n fitted rows; out[r][a] = scale[a] * sum_j (delta_j^2 - mu_j) V[j][a],
// scale[a] = -1/2 / sqrt(lambda_a) or 0 (the host's).  A workgroup per (row, eight axes): a thread adds its columns j =
// tid, tid + 256, ... in ascending order, the 256 partials by the fixed tree of dvs_block_sum -- an order n alone fixes,
// so the strip height and the run cannot change a bit.  A NaN cell makes every axis of its row NaN.
constexpr int PROJ_THREADS = 256;
constexpr uint32_t PROJ_AXES = 8;
__global__ __launch_bounds__(PROJ_THREADS) void pcoa_project_kernel(const double *__restrict__ strip, uint32_t n, uint32_t m,
                                                                    const double *__restrict__ V, const double *__restrict__ mu,
                                                                    const double *__restrict__ scale, double *__restrict__ out) {
    __shared__ double scratch[17];
    const uint32_t a0 = blockIdx.y * PROJ_AXES;
    const double *g = strip + uint64_t(blockIdx.x) * n;
    double acc[PROJ_AXES];
#pragma unroll
    for (uint32_t a = 0; a < PROJ_AXES; a++) acc[a] = 0.0;
    for (uint32_t j = threadIdx.x; j < n; j += PROJ_THREADS) {
        const double d = g[j];
        const double t = d * d - mu[j];
#pragma unroll
        for (uint32_t a = 0; a < PROJ_AXES; a++)
            if (a0 + a < m) acc[a] = fma(t, V[size_t(j) * m + a0 + a], acc[a]);
    }
#pragma unroll
    for (uint32_t a = 0; a < PROJ_AXES; a++) {
        const double sum = dvs_block_sum(acc[a], scratch);
        if (threadIdx.x == 0 && a0 + a < m) out[uint64_t(blockIdx.x) * m + a0 + a] = sum * scale[a0 + a];
    }
}

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

// The cells of a strip (mq x n) that lie within a radius, as a list per row in ascending column order (include/dvs_hip.h
// "neighbours within a radius"): three kernels over the strip as the distance kernels left it.  A row is cut into
// segments of WITHIN_SEG columns and one wave takes one (row, segment) item, 64 consecutive columns a step (lane l
// column c + l: coalesced).  A wave and not a workgroup per item because a row of a tall strip is a few cells long
// and a long row has n / WITHIN_SEG items of its own, so that either shape fills the device; the segments' counts
// meet in the scan below, in item order, and not in LDS, which none of the three kernels uses for a row.
//   within_count_kernel  counts[item]: popcount of the ballot of the predicate, summed over the steps
//   within_scan_kernel   offs[item]: the exclusive prefix sum of the counts in item order (row-major: a row's segments
//                        in column order), 64 bits; row_off[r] = base + offs of the row's first item; *total
//   within_write_kernel  the passing cells of an item at offs[item] on: a lane's slot is the running base plus the number
//                        of passing lanes below it (mbcnt of the ballot), the base advances by the ballot's popcount
// The predicate is within_cell, called by both kernels on the same buffer: d <= radius (NaN compares false) over the
// cells the rule lets it read -- every cell, every cell but the row's own position self = q0 + r (WITHIN_NOT_SELF), or
// only the columns above it (WITHIN_ABOVE_SELF: the upper triangle).  A cell the rule excludes is never loaded.  No
// atomics: every position is a function of the strip's bits alone.
constexpr int WITHIN_THREADS = 256;
constexpr uint32_t WITHIN_WAVES = WITHIN_THREADS / 64, WITHIN_SEG = 2048;
constexpr uint32_t WITHIN_ALL = 0, WITHIN_NOT_SELF = 1, WITHIN_ABOVE_SELF = 2;

struct within_seg {
    const double *g;  // the item's strip row
    uint32_t self;    // the row's own position
    uint32_t c0, j1;  // the first step's first column, the end of the segment
};

// item = r * nseg + s: columns [s WITHIN_SEG, min(n, (s + 1) WITHIN_SEG)) of strip row r.  Under WITHIN_ABOVE_SELF the
// steps that lie wholly at or below self hold nothing and are left out (whole steps: a lane keeps its columns)
__device__ __forceinline__ within_seg within_item(const double *strip, uint64_t item, uint32_t n, uint32_t nseg, uint32_t q0,
                                                  uint32_t rule) {
    const uint32_t r = nseg == 1 ? uint32_t(item) : uint32_t(item / nseg);
    const uint32_t j0 = nseg == 1 ? 0u : uint32_t(item % nseg) * WITHIN_SEG;
    within_seg w;
    w.g = strip + uint64_t(r) * n;
    w.self = q0 + r;
    w.j1 = n - j0 < WITHIN_SEG ? n : j0 + WITHIN_SEG;
    w.c0 = j0;
    if (rule == WITHIN_ABOVE_SELF && w.self >= j0) {
        const uint32_t skip = (w.self - j0 + 1) / 64 * 64;
        w.c0 = skip >= w.j1 - j0 ? w.j1 : j0 + skip;
    }
    return w;
}

// whether cell j of the item passes, and its value
__device__ __forceinline__ bool within_cell(const within_seg &w, uint32_t j, uint32_t rule, double radius, double &d) {
    const bool read = j < w.j1 && !(rule == WITHIN_NOT_SELF && j == w.self) && !(rule == WITHIN_ABOVE_SELF && j <= w.self);
    d = read ? w.g[j] : NAN;
    return d <= radius;
}

__global__ __launch_bounds__(WITHIN_THREADS) void within_count_kernel(const double *__restrict__ strip, uint32_t n,
                                                                      uint32_t nseg, uint64_t items, uint32_t q0,
                                                                      uint32_t rule, double radius,
                                                                      uint32_t *__restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t item = uint64_t(blockIdx.x) * WITHIN_WAVES + (threadIdx.x >> 6);
    if (item >= items) return;  // (the whole wave)
    const within_seg w = within_item(strip, item, n, nseg, q0, rule);
    uint32_t count = 0;
    for (uint32_t c = w.c0; c < w.j1; c += 64) {
        double d;
        count += uint32_t(__popcll(__ballot(within_cell(w, c + lane, rule, radius, d))));
    }
    if (lane == 0) counts[item] = count;
}

// One workgroup, looping: SCAN_CHUNK items a turn, SCAN_ITEMS consecutive ones per thread -- a thread over its own, the 64
// lanes by shuffle-up, the waves and the turns before through LDS and a carry every thread keeps.  Integer sums: exact in
// any shape.  items / SCAN_CHUNK turns of a load, one barrier (the waves' sums alternate between two LDS buffers, so a
// turn's readers need no second one) and a store: ~3 000 turns for the tallest strip there is, 11 million rows over 3
// references, and one turn for a strip of up to 4 096 items.
constexpr int SCAN_THREADS = 1024, SCAN_ITEMS = 4;
constexpr uint32_t SCAN_WAVES = SCAN_THREADS / 64, SCAN_CHUNK = SCAN_THREADS * SCAN_ITEMS;
__global__ __launch_bounds__(SCAN_THREADS) void within_scan_kernel(const uint32_t *__restrict__ counts, uint64_t items,
                                                                   uint32_t nseg, uint64_t base, uint64_t *__restrict__ offs,
                                                                   uint64_t *__restrict__ row_off,
                                                                   uint64_t *__restrict__ total) {
    __shared__ uint32_t s_top[2][SCAN_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t carry = 0;  // the sum of the turns before
    uint32_t flip = 0;
    for (uint64_t i0 = 0; i0 < items; i0 += SCAN_CHUNK) {
        const uint64_t t0 = i0 + uint64_t(tid) * SCAN_ITEMS;
        uint32_t c[SCAN_ITEMS];
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; k++) c[k] = t0 + k < items ? counts[t0 + k] : 0u;
        uint32_t mine = 0;  // (a turn's sum stays below 2^32: SCAN_CHUNK x WITHIN_SEG = 2^23)
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; k++) mine += c[k];
        uint32_t incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(incl, o, 64);
            if (lane >= uint32_t(o)) incl += u;
        }
        if (lane == 63) s_top[flip][wave] = incl;
        __syncthreads();  // (two buffers: the writers of the turn after next have passed the next turn's barrier)
        uint32_t before = 0, turn = 0;
#pragma unroll
        for (uint32_t x = 0; x < SCAN_WAVES; x++) {
            const uint32_t top = s_top[flip][x];
            if (x < wave) before += top;
            turn += top;
        }
        flip ^= 1;
        uint64_t at = carry + before + (incl - mine);
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; k++) {
            const uint64_t item = t0 + k;
            if (item < items) {
                offs[item] = at;
                if (nseg == 1)
                    row_off[item] = base + at;
                else if (item % nseg == 0)
                    row_off[item / nseg] = base + at;
            }
            at += c[k];
        }
        carry += turn;
    }
    if (tid == 0) *total = carry;
}

// dist may be NULL (the positions alone: the threshold clusters)
__global__ __launch_bounds__(WITHIN_THREADS) void within_write_kernel(const double *__restrict__ strip, uint32_t n,
                                                                      uint32_t nseg, uint64_t items, uint32_t q0,
                                                                      uint32_t rule, double radius,
                                                                      const uint64_t *__restrict__ offs,
                                                                      uint32_t *__restrict__ col, double *__restrict__ dist) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t item = uint64_t(blockIdx.x) * WITHIN_WAVES + (threadIdx.x >> 6);
    if (item >= items) return;  // (the whole wave)
    const within_seg w = within_item(strip, item, n, nseg, q0, rule);
    uint64_t at = offs[item];
    for (uint32_t c = w.c0; c < w.j1; c += 64) {
        double d;
        const bool pass = within_cell(w, c + lane, rule, radius, d);
        const unsigned long long mask = __ballot(pass);
        if (pass) {
            const uint64_t slot = at + __builtin_amdgcn_mbcnt_hi(uint32_t(mask >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mask), 0u));
            col[slot] = c + lane;
            if (dist) dist[slot] = d;
        }
        at += uint64_t(__popcll(mask));
    }
}

// ---- the two count-matrix modes

// what both of them check: one device, equal bin counts, the row lists, the square path's limit on the columns
int matrix_sides_check(dvs_ctx *ctx, const dvs_matrix *q, const uint32_t *q_rows, uint32_t nq, const dvs_matrix *r,
                       const uint32_t *r_rows, uint32_t nr) {
    if (q->ctx != r->ctx || q->device != ctx->device || r->device != ctx->device)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "the two matrices and the context are not on one device");
    if (q->nbins != r->nbins)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "the query rows have %llu bins, the reference rows %llu",
                             (unsigned long long)q->nbins, (unsigned long long)r->nbins);
    if (int rc = dvs_cross_rows_check(ctx, q_rows, nq, q->nrows, "query")) return rc;
    if (int rc = dvs_cross_rows_check(ctx, r_rows, nr, r->nrows, "reference")) return rc;
    return dvs_rows_check(ctx, nr);
}

// f(typed query rows, typed reference rows) for the two matrices' element types: any of the nine combinations
template <typename F>
void sides_dispatch(const dvs_matrix *q, const dvs_matrix *r, F &&f) {
    dvs_mat_dispatch(q, [&](auto *qp) {
        return dvs_mat_dispatch(r, [&](auto *rp) {
            f(qp, rp);
            return 0;
        });
    });
}

// scratch: the nq + nr row entropies, then the row lists
dvs_cross_stage jsd_cross_stage(dvs_ctx *ctx, const dvs_matrix *q, const uint32_t *q_rows, uint32_t nq, const dvs_matrix *r,
                                const uint32_t *r_rows, uint32_t nr) {
    dvs_cross_stage st{"jsd cross distances", nq, nr};
    const dvs_cross_lists lists{(size_t(nq) + nr) * 8, q_rows, r_rows, nq, nr};
    st.check = [=] { return matrix_sides_check(ctx, q, q_rows, nq, r, r_rows, nr); };
    st.scratch_bytes = lists.bytes();
    st.scratch_what = "row entropies and row lists";
    st.prepare = [=](void *d_scratch) {
        hipError_t e = lists.upload(ctx, d_scratch);
        double *d_hq = static_cast<double *>(d_scratch), *d_hr = d_hq + nq;
        auto entropies = [&](const dvs_matrix *m, const uint32_t *d_rows, uint32_t count, double *d_h) {
            if (e == hipSuccess) e = dvs_jsd_entropies_enqueue(ctx, m, d_rows, count, d_h);
        };
        entropies(q, lists.dq(d_scratch), nq, d_hq);
        entropies(r, lists.dr(d_scratch), nr, d_hr);
        return e;
    };
    st.enqueue = [=](uint32_t q0, uint32_t mq, double *d_strip, void *d_scratch) {
        const double *d_hq = static_cast<const double *>(d_scratch), *d_hr = d_hq + nq;
        const dim3 grid((mq + JSD_TILE - 1) / JSD_TILE, (nr + JSD_TILE - 1) / JSD_TILE);
        sides_dispatch(q, r, [&](auto *qp, auto *rp) {
            using T = std::remove_cv_t<std::remove_pointer_t<decltype(qp)>>;
            using U = std::remove_cv_t<std::remove_pointer_t<decltype(rp)>>;
            hipLaunchKernelGGL((jsd_cross_kernel<T, U>), grid, dim3(JSD_THREADS), 0, ctx->stream, qp, q->d_totals,
                               lists.dq(d_scratch), q0, mq, rp, r->d_totals, lists.dr(d_scratch), nr, q->nbins, d_hq, d_hr,
                               d_strip);
        });
        return hipGetLastError();
    };
    return st;
}

// scratch: the row lists only
dvs_cross_stage euclid_cross_stage(dvs_ctx *ctx, const dvs_matrix *q, const uint32_t *q_rows, uint32_t nq,
                                   const dvs_matrix *r, const uint32_t *r_rows, uint32_t nr,
                                   const uint32_t *d_q_rows = nullptr) {
    dvs_cross_stage st{"euclidean cross distances", nq, nr};
    const dvs_cross_lists lists{0, q_rows, r_rows, nq, nr, d_q_rows};
    st.check = [=] { return matrix_sides_check(ctx, q, q_rows, nq, r, r_rows, nr); };
    st.scratch_bytes = lists.bytes();
    st.scratch_what = "row lists";
    st.prepare = [=](void *d_scratch) { return lists.upload(ctx, d_scratch); };
    st.enqueue = [=](uint32_t q0, uint32_t mq, double *d_strip, void *d_scratch) {
        const dim3 grid(mq, (nr + EUC_THREADS / 64 - 1) / (EUC_THREADS / 64));
        sides_dispatch(q, r, [&](auto *qp, auto *rp) {
            using T = std::remove_cv_t<std::remove_pointer_t<decltype(qp)>>;
            using U = std::remove_cv_t<std::remove_pointer_t<decltype(rp)>>;
            hipLaunchKernelGGL((euclid_cross_kernel<T, U>), grid, dim3(EUC_THREADS), 0, ctx->stream, qp, q->d_totals,
                               lists.dq(d_scratch), q0, rp, r->d_totals, lists.dr(d_scratch), nr, q->nbins, d_strip);
        });
        return hipGetLastError();
    };
    return st;
}

// A caller's own n x n matrix as a stage: rows [q0, q0 + mq) are copied into the strip, from the host or within the
// device; the matrix is only read.
dvs_cross_stage matrix_rows_stage(dvs_ctx *ctx, const double *dist, int dist_on_device, uint32_t n) {
    dvs_cross_stage st{"distance matrix rows", n, n};
    st.check = [=] {
        if (dist_on_device)
            if (int rc = dvs_given_on_device(ctx, nullptr, dist)) return rc;
        return dvs_rows_check(ctx, n);
    };
    st.scratch_bytes = 0;
    st.scratch_what = "";
    st.prepare = [](void *) { return hipSuccess; };
    st.enqueue = [=](uint32_t q0, uint32_t mq, double *d_strip, void *) {
        return hipMemcpyAsync(d_strip, dist + size_t(q0) * n, size_t(mq) * n * 8,
                              dist_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream);
    };
    return st;
}

// ---- the three drivers

// query rows per strip: what CROSS_STRIP_BYTES holds, in whole tile rows and one tile row at least; or the knob
uint32_t strip_rows(const dvs_ctx *ctx, const dvs_cross_stage &st) {
    uint64_t rows = ctx->knobs.cross_strip_rows;
    if (!rows) rows = std::max<uint64_t>(CROSS_STRIP_BYTES / (size_t(st.n) * 8) / JSD_TILE * JSD_TILE, JSD_TILE);
    return uint32_t(std::min<uint64_t>(rows, st.m));
}

// The stage strip by strip on the context's stream, consume(q0, mq, d_strip) enqueued behind each: returns once the
// stream is drained -- whatever consume copied to the host has arrived -- with the stage's zero-division word read.
// stop (may be NULL): set by consume when no further strip is wanted.
template <typename F>
int cross_walk(dvs_ctx *ctx, const dvs_cross_stage &st, uint32_t rows, F &&consume, const bool *stop = nullptr) {
    PooledBuf d_strip{ctx}, d_scratch{ctx};
    int rc = dvs_dev_alloc(ctx, &d_strip.p, size_t(rows) * st.n * 8, "distance strip");
    if (!rc && st.scratch_bytes) rc = dvs_dev_alloc(ctx, &d_scratch.p, st.scratch_bytes, st.scratch_what);
    if (rc) return rc;
    hipError_t e = st.prepare(d_scratch.p);
    for (uint64_t q0 = 0; e == hipSuccess && q0 < st.m && !(stop && *stop); q0 += rows) {
        const uint32_t mq = uint32_t(std::min<uint64_t>(rows, st.m - q0));
        e = st.enqueue(uint32_t(q0), mq, d_strip.as<double>(), d_scratch.p);
        if (e == hipSuccess) e = consume(uint32_t(q0), mq, d_strip.as<double>());
    }
    uint32_t flag = 0;
    if (e == hipSuccess && st.scratch_is_zerodiv)
        e = hipMemcpyAsync(&flag, d_scratch.p, 4, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t se = hipStreamSynchronize(ctx->stream);  // (the blocks go back to the cache behind it)
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, st.label);
    if (se != hipSuccess) return dvs_hip_fail(ctx, se, st.label);
    if (flag) return dvs_set_error(ctx, DVS_ERR_ZERODIV, "division by zero");  // 0 / 0, distance.py:283
    return DVS_OK;
}

// the m x n matrix of a stage into the host array dist
int cross_to_host(dvs_ctx *ctx, const dvs_cross_stage &st, double *dist) {
    if (st.m == 0 || st.n == 0) return DVS_OK;
    if (!dist) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (int rc = st.check()) return rc;
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    return cross_walk(ctx, st, strip_rows(ctx, st), [&](uint32_t q0, uint32_t mq, double *d_strip) {
        return hipMemcpyAsync(dist + size_t(q0) * st.n, d_strip, size_t(mq) * st.n * 8, hipMemcpyDeviceToHost, ctx->stream);
    });
}

// the kk nearest references of every query into the host arrays idx, dist (m x kk)
int cross_to_topk(dvs_ctx *ctx, const dvs_cross_stage &st, uint32_t kk, uint32_t *idx, double *dist) {
    if (kk == 0 || kk > st.n)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "%u nearest of %u references: between 1 and the number of references", kk, st.n);
    if (kk > TOPK_MAX)
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "%u nearest: %u at most (a full ranking takes the matrix)", kk, TOPK_MAX);
    if (st.m == 0) return DVS_OK;
    if (!idx || !dist) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (int rc = st.check()) return rc;
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t rows = strip_rows(ctx, st);
    PooledBuf d_idx{ctx}, d_val{ctx};
    int rc = dvs_dev_alloc(ctx, &d_idx.p, size_t(rows) * kk * 4, "nearest references");
    if (!rc) rc = dvs_dev_alloc(ctx, &d_val.p, size_t(rows) * kk * 8, "nearest distances");
    if (rc) return rc;
    return cross_walk(ctx, st, rows, [&](uint32_t q0, uint32_t mq, double *d_strip) {
        hipLaunchKernelGGL(cross_topk_kernel, dim3(mq), dim3(TOPK_THREADS), 0, ctx->stream, d_strip, st.n, kk,
                           d_idx.as<uint32_t>(), d_val.as<double>());
        hipError_t e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync(idx + size_t(q0) * kk, d_idx.p, size_t(mq) * kk * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(dist + size_t(q0) * kk, d_val.p, size_t(mq) * kk * 8, hipMemcpyDeviceToHost, ctx->stream);
        return e;
    });
}

// the coordinates of every query in a fitted ordination (include/dvs_hip.h "principal coordinates") into the host array
// coords (m x n_axes): the fit's tables uploaded once, pcoa_project_kernel behind each strip's distances
int cross_to_project(dvs_ctx *ctx, const dvs_cross_stage &st, uint32_t n_axes, const double *values, const double *vectors,
                     const double *row_means, double *coords) {
    if (n_axes == 0) return dvs_set_error(ctx, DVS_ERR_VALUE, "principal coordinates: one axis at least");
    if (n_axes > TOPK_MAX)
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "%u axes: %u at most", n_axes, TOPK_MAX);
    if (!values || !vectors || !row_means) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (st.n == 0) return dvs_set_error(ctx, DVS_ERR_VALUE, "a projection needs the fitted rows: no reference rows");
    if (st.m == 0) return DVS_OK;
    if (!coords) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (int rc = st.check()) return rc;
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t rows = strip_rows(ctx, st);
    const size_t nv = size_t(st.n) * n_axes;
    std::vector<double> scale(n_axes);
    for (uint32_t a = 0; a < n_axes; a++) scale[a] = values[a] > 0.0 ? -0.5 / std::sqrt(values[a]) : 0.0;
    PooledBuf d_fit{ctx}, d_out{ctx};  // d_fit: V [n x n_axes], mu [n], scale [n_axes]
    int rc = dvs_dev_alloc(ctx, &d_fit.p, (nv + st.n + n_axes) * 8, "fitted ordination");
    if (!rc) rc = dvs_dev_alloc(ctx, &d_out.p, size_t(rows) * n_axes * 8, "projected coordinates");
    if (rc) return rc;
    double *d_v = d_fit.as<double>(), *d_mu = d_v + nv, *d_scale = d_mu + st.n;
    hipError_t e = hipMemcpyAsync(d_v, vectors, nv * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_mu, row_means, size_t(st.n) * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_scale, scale.data(), size_t(n_axes) * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->stream);
        return dvs_hip_fail(ctx, e, "fitted ordination upload");
    }
    return cross_walk(ctx, st, rows, [&](uint32_t q0, uint32_t mq, double *d_strip) {
        hipLaunchKernelGGL(pcoa_project_kernel, dim3(mq, (n_axes + PROJ_AXES - 1) / PROJ_AXES), dim3(PROJ_THREADS), 0, ctx->stream,
                           d_strip, st.n, n_axes, d_v, d_mu, d_scale, d_out.as<double>());
        hipError_t le = hipGetLastError();
        if (le == hipSuccess)
            le = hipMemcpyAsync(coords + size_t(q0) * n_axes, d_out.p, size_t(mq) * n_axes * 8, hipMemcpyDeviceToHost, ctx->stream);
        return le;
    });
}

// The scores of a labelling (include/dvs_hip.h "flat clusters") over a stage whose queries and references are the same
// n positions: the positions sorted by label once (a stable counting sort: order, start) and uploaded in front of the
// first strip, cluster_scores_kernel behind each strip's distances, its five outputs copied out strip by strip; the
// medoids from the n sums on the host.
int cross_to_cluster_scores(dvs_ctx *ctx, const dvs_cross_stage &st, const uint32_t *labels, uint32_t n_clusters,
                            double *within, double *a, double *b, uint32_t *neighbour, double *silhouette,
                            uint32_t *medoids) {
    const uint32_t n = st.n;
    if (n == 0) return DVS_OK;
    if (!labels || !within) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    for (uint32_t i = 0; i < n; i++)
        if (labels[i] >= n_clusters)
            return dvs_set_error(ctx, DVS_ERR_VALUE, "row %u carries label %u: below the number of clusters (%u)", i,
                                 labels[i], n_clusters);
    if (int rc = st.check()) return rc;
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> start(size_t(n_clusters) + 1, 0), order(n);
    for (uint32_t i = 0; i < n; i++) start[labels[i] + 1]++;
    for (uint32_t c = 0; c < n_clusters; c++) start[c + 1] += start[c];
    {
        std::vector<uint32_t> next(start.begin(), start.end() - 1);
        for (uint32_t i = 0; i < n; i++) order[next[labels[i]]++] = i;
    }
    const uint32_t rows = strip_rows(ctx, st);
    // one block: order [n], start [K + 1], label [n], then per strip row four doubles and the neighbour
    const size_t o_start = size_t(n) * 4, o_label = o_start + (size_t(n_clusters) + 1) * 4;
    const size_t o_out = (o_label + size_t(n) * 4 + 7) / 8 * 8;
    PooledBuf d_buf{ctx};
    int rc = dvs_dev_alloc(ctx, &d_buf.p, o_out + size_t(rows) * 36, "cluster lists and scores");
    if (rc) return rc;
    char *base = d_buf.as<char>();
    uint32_t *d_order = reinterpret_cast<uint32_t *>(base), *d_start = reinterpret_cast<uint32_t *>(base + o_start),
             *d_label = reinterpret_cast<uint32_t *>(base + o_label);
    double *d_within = reinterpret_cast<double *>(base + o_out), *d_a = d_within + rows, *d_b = d_a + rows, *d_sil = d_b + rows;
    uint32_t *d_nb = reinterpret_cast<uint32_t *>(d_sil + rows);
    hipError_t e = hipMemcpyAsync(d_order, order.data(), size_t(n) * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_start, start.data(), start.size() * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_label, labels, size_t(n) * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->stream);
        return dvs_hip_fail(ctx, e, "cluster lists upload");
    }
    rc = cross_walk(ctx, st, rows, [&](uint32_t q0, uint32_t mq, double *d_strip) {
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
    });
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);  // (the uploads read the lists above)
        return rc;
    }
    if (medoids) {
        for (uint32_t c = 0; c < n_clusters; c++) {
            uint32_t best = NONE;
            for (uint32_t p = start[c]; p < start[c + 1]; p++) {  // ascending rows: strict < keeps the lowest of a tie
                const uint32_t i = order[p];
                if (within[i] == within[i] && (best == NONE || within[i] < within[best])) best = i;
            }
            medoids[c] = best;
        }
    }
    return DVS_OK;
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

// The cophenetic correlation of a tree (include/dvs_hip.h "cophenetic distances") over a stage whose queries and
// references are the tree's n leaves: the in-order walk on the host, its three lists and the heights uploaded in front
// of the first strip in one pooled block that also holds the strip's 5 sums per row; cophenet_kernel behind each
// strip's distances, the sums (and, when asked for, the cophenetic rows, from a second strip buffer) copied out strip
// by strip; r from the 5 n sums on the host.
int cross_to_cophenet(dvs_ctx *ctx, const dvs_cross_stage &st, const uint32_t *pairs, const double *heights, double *corr,
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
    if (int rc = st.check()) return rc;
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t rows = strip_rows(ctx, st);
    std::vector<double> own_sums;
    if (!row_sums) {
        own_sums.resize(size_t(5) * n);
        row_sums = own_sums.data();
    }
    PooledBuf d_buf{ctx}, d_coph{ctx};
    int rc = dvs_dev_alloc(ctx, &d_buf.p, o_out + size_t(rows) * 40, "tree lists and row sums");
    if (!rc && coph) rc = dvs_dev_alloc(ctx, &d_coph.p, size_t(rows) * n * 8, "cophenetic strip");
    if (rc) return rc;
    char *base = d_buf.as<char>();
    const uint32_t *d_order = reinterpret_cast<uint32_t *>(base), *d_pos = reinterpret_cast<uint32_t *>(base + o_pos),
                   *d_gap = reinterpret_cast<uint32_t *>(base + o_gap);
    const double *d_heights = reinterpret_cast<double *>(base + o_h);
    double *d_sums = reinterpret_cast<double *>(base + o_out);
    const hipError_t e = hipMemcpyAsync(base, hb, o_out, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->stream);
        return dvs_hip_fail(ctx, e, "tree lists upload");
    }
    rc = cross_walk(ctx, st, rows, [&](uint32_t q0, uint32_t mq, double *d_strip) {
        hipLaunchKernelGGL(cophenet_kernel, dim3(mq), dim3(COPH_THREADS), 0, ctx->stream, d_strip, n, q0, d_order, d_pos,
                           d_gap, d_heights, c_bar, rows, d_sums, d_coph.as<double>());
        hipError_t ce = hipGetLastError();
        for (int a = 0; a < 5 && ce == hipSuccess; a++)
            ce = hipMemcpyAsync(row_sums + size_t(a) * n + q0, d_sums + size_t(a) * rows, size_t(mq) * 8,
                                hipMemcpyDeviceToHost, ctx->stream);
        if (ce == hipSuccess && coph)
            ce = hipMemcpyAsync(coph + size_t(q0) * n, d_coph.p, size_t(mq) * n * 8, hipMemcpyDeviceToHost, ctx->stream);
        return ce;
    });
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);  // (the upload reads the lists above)
        return rc;
    }
    *corr = cophenet_correlation(row_sums, n);
    return DVS_OK;
}

// The cells within `radius` of a stage, strip by strip: the three within_* kernels behind each strip's distances, then
// the strip's number of pairs read back and waited for (the one synchronisation per strip: the host has to know how
// much to take, and whether max_pairs -- 0: no limit -- is passed), then sink(q0, mq, base, count, d_row_off, d_col,
// d_dist) -> DVS_OK or the error it set: the strip's `count` pairs lie at d_col / d_dist (NULL unless want_dist) in row
// order, d_row_off[r] is base plus the pairs in front of strip row r, base the pairs of the strips before.  What sink
// enqueues on the context's stream is done before the next sink is called, and when this returns.  The pair buffers
// hold the worst case of one strip; a negative radius is passed on as NaN, which no cell is within.
template <typename Sink>
int cross_within_walk(dvs_ctx *ctx, const dvs_cross_stage &st, double radius, uint32_t rule, bool want_dist,
                      uint64_t max_pairs, uint64_t *n_pairs, Sink &&sink) {
    const uint32_t n = st.n, rows = strip_rows(ctx, st), nseg = (n + WITHIN_SEG - 1) / WITHIN_SEG;
    const uint64_t max_items = uint64_t(rows) * nseg, cap = uint64_t(rows) * n;
    if ((max_items + WITHIN_WAVES - 1) / WITHIN_WAVES > 0x7FFFFFFFull)
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "a strip of %u rows: more row segments than a grid takes", rows);
    // one block: offs [items], row_off [rows] and the total, 64 bits each, then counts [items]
    PooledBuf d_scan{ctx}, d_col{ctx}, d_dist{ctx};
    int rc = dvs_dev_alloc(ctx, &d_scan.p, size_t(max_items + rows + 1) * 8 + size_t(max_items) * 4, "within counts and offsets");
    if (!rc) rc = dvs_dev_alloc(ctx, &d_col.p, size_t(cap) * 4, "within positions");
    if (!rc && want_dist) rc = dvs_dev_alloc(ctx, &d_dist.p, size_t(cap) * 8, "within distances");
    if (rc) return rc;
    uint64_t *d_offs = d_scan.as<uint64_t>(), *d_row_off = d_offs + max_items, *d_total = d_row_off + rows;
    uint32_t *d_counts = reinterpret_cast<uint32_t *>(d_total + 1);
    const double r_eff = radius < 0.0 ? double(NAN) : radius;
    uint64_t base = 0, over = 0;
    bool stop = false;
    int sink_rc = DVS_OK;
    rc = cross_walk(ctx, st, rows, [&](uint32_t q0, uint32_t mq, double *d_strip) {
        const uint64_t items = uint64_t(mq) * nseg;
        const dim3 grid(uint32_t((items + WITHIN_WAVES - 1) / WITHIN_WAVES));
        hipLaunchKernelGGL(within_count_kernel, grid, dim3(WITHIN_THREADS), 0, ctx->stream, d_strip, n, nseg, items, q0, rule,
                           r_eff, d_counts);
        hipLaunchKernelGGL(within_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, d_counts, items, nseg, base,
                           d_offs, d_row_off, d_total);
        hipLaunchKernelGGL(within_write_kernel, grid, dim3(WITHIN_THREADS), 0, ctx->stream, d_strip, n, nseg, items, q0, rule,
                           r_eff, d_offs, d_col.as<uint32_t>(), d_dist.as<double>());
        hipError_t e = hipGetLastError();
        uint64_t count = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&count, d_total, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return e;
        if (max_pairs && base + count > max_pairs) {
            over = base + count;
            stop = true;
            return hipSuccess;
        }
        sink_rc = sink(q0, mq, base, count, d_row_off, d_col.as<uint32_t>(), d_dist.as<double>());
        stop = sink_rc != DVS_OK;
        base += count;
        return hipSuccess;
    }, &stop);
    if (rc) return rc;
    if (sink_rc) return sink_rc;
    if (over)
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "%llu pairs within the radius so far: more than max_pairs = %llu",
                             (unsigned long long)over, (unsigned long long)max_pairs);
    *n_pairs = base;
    return DVS_OK;
}

}  // namespace

// a CSR list of (query position, reference position, distance) on the host
struct dvs_pairs {
    std::vector<uint64_t> row_start;  // [n_rows + 1]
    std::vector<uint32_t> col;
    std::vector<double> dist;
};

namespace {

constexpr uint32_t WITHIN_FLAGS = DVS_WITHIN_SKIP_SELF;

// the cells within `radius` of a stage into a new dvs_pairs (include/dvs_hip.h "neighbours within a radius")
int cross_to_within(dvs_ctx *ctx, const dvs_cross_stage &st, double radius, uint32_t flags, uint64_t max_pairs,
                    dvs_pairs **out) {
    if (!out) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    *out = nullptr;
    if (radius != radius) return dvs_set_error(ctx, DVS_ERR_VALUE, "the radius cannot be NaN");
    if (flags & ~WITHIN_FLAGS) return dvs_set_error(ctx, DVS_ERR_VALUE, "unknown flag bits 0x%x", flags & ~WITHIN_FLAGS);
    std::unique_ptr<dvs_pairs> p;
    try {
        p.reset(new dvs_pairs);
        p->row_start.assign(size_t(st.m) + 1, 0);
    } catch (const std::exception &) {
        return dvs_set_error(ctx, DVS_ERR_NOMEM, "no host memory for the row starts of %u queries", st.m);
    }
    if (st.m == 0 || st.n == 0) {
        *out = p.release();
        return DVS_OK;
    }
    if (int rc = st.check()) return rc;
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t total = 0;
    const int rc = cross_within_walk(
        ctx, st, radius, flags & DVS_WITHIN_SKIP_SELF ? WITHIN_NOT_SELF : WITHIN_ALL, true, max_pairs, &total,
        [&](uint32_t q0, uint32_t mq, uint64_t base, uint64_t count, const uint64_t *d_row_off, const uint32_t *d_col,
            const double *d_dist) {
            try {  // (nothing is in flight into the vectors: the walk has waited for the copies of the strip before)
                p->col.resize(size_t(base + count));
                p->dist.resize(size_t(base + count));
            } catch (const std::exception &) {
                return dvs_set_error(ctx, DVS_ERR_NOMEM, "no host memory for %llu pairs", (unsigned long long)(base + count));
            }
            hipError_t e = hipMemcpyAsync(p->row_start.data() + q0, d_row_off, size_t(mq) * 8, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess && count)
                e = hipMemcpyAsync(p->col.data() + base, d_col, size_t(count) * 4, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess && count)
                e = hipMemcpyAsync(p->dist.data() + base, d_dist, size_t(count) * 8, hipMemcpyDeviceToHost, ctx->stream);
            return e == hipSuccess ? DVS_OK : dvs_hip_fail(ctx, e, "within pairs read-back");
        });
    if (rc) return rc;
    p->row_start[st.m] = total;
    *out = p.release();
    return DVS_OK;
}

// The connected components of the graph "distance <= radius" over a stage whose queries and references are the same n
// positions (include/dvs_hip.h "threshold clusters"): the edges of the upper triangle strip by strip through a
// union-find on the host (union by lower root index, path halving), a strip's edges dropped before the next strip's
// arrive; the labels by first appearance in position order -- a component's root is its lowest position.
int cross_to_threshold_clusters(dvs_ctx *ctx, const dvs_cross_stage &st, double radius, uint32_t *labels,
                                uint32_t *n_clusters) {
    const uint32_t n = st.n;
    if (n == 0) return DVS_OK;
    if (!labels || !n_clusters) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (radius != radius) return dvs_set_error(ctx, DVS_ERR_VALUE, "the radius cannot be NaN");
    if (int rc = st.check()) return rc;
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> parent, h_col;
    std::vector<uint64_t> h_off;
    try {
        parent.resize(n);
    } catch (const std::exception &) {
        return dvs_set_error(ctx, DVS_ERR_NOMEM, "no host memory for the union-find of %u positions", n);
    }
    for (uint32_t i = 0; i < n; i++) parent[i] = i;
    auto find = [&](uint32_t x) {
        while (parent[x] != x) {
            parent[x] = parent[parent[x]];
            x = parent[x];
        }
        return x;
    };
    uint64_t total = 0;
    const int rc = cross_within_walk(
        ctx, st, radius, WITHIN_ABOVE_SELF, false, 0, &total,
        [&](uint32_t q0, uint32_t mq, uint64_t base, uint64_t count, const uint64_t *d_row_off, const uint32_t *d_col,
            const double *) {
            if (!count) return DVS_OK;
            try {
                h_col.resize(size_t(count));
                h_off.resize(size_t(mq) + 1);
            } catch (const std::exception &) {
                return dvs_set_error(ctx, DVS_ERR_NOMEM, "no host memory for the %llu edges of a strip", (unsigned long long)count);
            }
            hipError_t e = hipMemcpyAsync(h_off.data(), d_row_off, size_t(mq) * 8, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(h_col.data(), d_col, size_t(count) * 4, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) return dvs_hip_fail(ctx, e, "threshold edges read-back");
            h_off[mq] = base + count;
            for (uint32_t r = 0; r < mq; r++)
                for (uint64_t p = h_off[r] - base; p < h_off[r + 1] - base; p++) {
                    const uint32_t a = find(q0 + r), b = find(h_col[size_t(p)]);
                    if (a != b) parent[a > b ? a : b] = a > b ? b : a;
                }
            return DVS_OK;
        });
    if (rc) return rc;
    uint32_t next = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t root = find(i);
        labels[i] = root == i ? next++ : labels[root];  // (root < i: it has its label)
    }
    *n_clusters = next;
    return DVS_OK;
}

}  // namespace

dvs_cross_stage dvs_euclid_cross_stage(dvs_ctx *ctx, const dvs_matrix *q, const uint32_t *q_rows, uint32_t nq,
                                       const dvs_matrix *r, const uint32_t *r_rows, uint32_t nr, const uint32_t *d_q_rows) {
    return euclid_cross_stage(ctx, q, q_rows, nq, r, r_rows, nr, d_q_rows);
}

hipError_t dvs_jsd_entropies_enqueue(dvs_ctx *ctx, const dvs_matrix *m, const uint32_t *d_rows, uint32_t count, double *d_h) {
    dvs_mat_dispatch(m, [&](auto *mp) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(mp)>>;
        hipLaunchKernelGGL((jsd_entropy_kernel<T>), dim3((count + 63) / 64), dim3(64), 0, ctx->stream, mp, m->d_totals, d_rows,
                           count, m->nbins, d_h);
        return 0;
    });
    return hipGetLastError();
}

hipError_t dvs_jsd_cross_row_enqueue(dvs_ctx *ctx, const dvs_matrix *m, const uint32_t *d_q_rows, uint32_t q0, uint32_t n,
                                     const double *d_hq, const double *d_hr, double *d_row) {
    dvs_mat_dispatch(m, [&](auto *mp) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(mp)>>;
        hipLaunchKernelGGL((jsd_cross_kernel<T, T>), dim3(1, (n + JSD_TILE - 1) / JSD_TILE), dim3(JSD_THREADS), 0, ctx->stream,
                           mp, m->d_totals, d_q_rows, q0, 1u, mp, m->d_totals, static_cast<const uint32_t *>(nullptr), n,
                           m->nbins, d_hq, d_hr, d_row);
        return 0;
    });
    return hipGetLastError();
}

int dvs_cross_rows_check(dvs_ctx *ctx, const uint32_t *rows, uint32_t nrows, uint32_t limit, const char *side) {
    if (!rows) {
        if (nrows > limit) return dvs_set_error(ctx, DVS_ERR_VALUE, "%u %s rows of a handle that holds %u", nrows, side, limit);
        return DVS_OK;
    }
    for (uint32_t i = 0; i < nrows; i++)
        if (rows[i] >= limit)
            return dvs_set_error(ctx, DVS_ERR_VALUE, "%s row list: entry %u is row %u of a handle that holds %u", side, i, rows[i], limit);
    return DVS_OK;
}

// ---- the entries: a source or two (include/dvs_hip.h dvs_source), checked, as a stage of the drivers above

// the sides checked by dvs_source_check: of one kind, GIVEN the caller's matrix against itself
static dvs_cross_stage source_cross_stage(dvs_ctx *ctx, const dvs_source *q, const dvs_source *r) {
    switch (q->kind) {
    case DVS_SRC_MASH:
        return dvs_mash_cross_stage(ctx, dvs_src_sketches(q), q->rows, q->n, dvs_src_sketches(r), r->rows, r->n, q->k,
                                    q->sketch_size);
    case DVS_SRC_EUCLIDEAN:
        return euclid_cross_stage(ctx, dvs_src_matrix(q), q->rows, q->n, dvs_src_matrix(r), r->rows, r->n);
    case DVS_SRC_JSD:
        return jsd_cross_stage(ctx, dvs_src_matrix(q), q->rows, q->n, dvs_src_matrix(r), r->rows, r->n);
    default:
        return matrix_rows_stage(ctx, static_cast<const double *>(q->handle), q->on_device, q->n);
    }
}

extern "C" int dvs_cross_distances(dvs_ctx *ctx, const dvs_source *q, const dvs_source *r, double *dist) {
    if (int rc = dvs_source_check(ctx, q, r)) return rc;
    if (q->kind == DVS_SRC_GIVEN) return dvs_source_refuse(ctx, "dvs_cross_distances", q, "the matrix");
    return cross_to_host(ctx, source_cross_stage(ctx, q, r), dist);
}

extern "C" int dvs_nearest(dvs_ctx *ctx, const dvs_source *q, const dvs_source *r, uint32_t kk, uint32_t *idx,
                           double *dist) {
    if (int rc = dvs_source_check(ctx, q, r)) return rc;
    if (q->kind == DVS_SRC_GIVEN) return dvs_source_refuse(ctx, "dvs_nearest", q, "the matrix");
    return cross_to_topk(ctx, source_cross_stage(ctx, q, r), kk, idx, dist);
}

extern "C" int dvs_pcoa_project(dvs_ctx *ctx, const dvs_source *q, const dvs_source *r, uint32_t n_axes, const double *values,
                                const double *vectors, const double *row_means, double *coords) {
    if (int rc = dvs_source_check(ctx, q, r)) return rc;
    if (q->kind == DVS_SRC_GIVEN) return dvs_source_refuse(ctx, "dvs_pcoa_project", q, "the matrix");
    return cross_to_project(ctx, source_cross_stage(ctx, q, r), n_axes, values, vectors, row_means, coords);
}

extern "C" int dvs_cluster_scores(dvs_ctx *ctx, const dvs_source *src, const uint32_t *labels, uint32_t n_clusters,
                                  double *within, double *a, double *b, uint32_t *neighbour, double *silhouette,
                                  uint32_t *medoids) {
    if (int rc = dvs_source_check(ctx, src, src)) return rc;
    return cross_to_cluster_scores(ctx, source_cross_stage(ctx, src, src), labels, n_clusters, within, a, b, neighbour,
                                   silhouette, medoids);
}

extern "C" int dvs_cophenet(dvs_ctx *ctx, const dvs_source *src, const uint32_t *pairs, const double *heights, double *corr,
                            double *row_sums, double *coph) {
    if (int rc = dvs_source_check(ctx, src, src)) return rc;
    return cross_to_cophenet(ctx, source_cross_stage(ctx, src, src), pairs, heights, corr, row_sums, coph);
}

extern "C" int dvs_within(dvs_ctx *ctx, const dvs_source *q, const dvs_source *r, double radius, uint32_t flags,
                          uint64_t max_pairs, dvs_pairs **out) {
    if (out) *out = nullptr;
    if (!r && q && q->kind == DVS_SRC_GIVEN) r = q;  // a caller's matrix is both sides
    if (int rc = dvs_source_check(ctx, q, r)) return rc;
    if (q->kind == DVS_SRC_GIVEN && (r->handle != q->handle || r->n != q->n || r->on_device != q->on_device))
        return dvs_source_refuse(ctx, "dvs_within", q, "another matrix as the references");
    return cross_to_within(ctx, source_cross_stage(ctx, q, r), radius, flags, max_pairs, out);
}

extern "C" void dvs_pairs_destroy(dvs_pairs *p) { delete p; }

extern "C" int dvs_pairs_info(const dvs_pairs *p, uint32_t *n_rows, uint64_t *n_pairs) {
    if (!p) return DVS_ERR_VALUE;
    if (n_rows) *n_rows = uint32_t(p->row_start.size() - 1);
    if (n_pairs) *n_pairs = p->row_start.back();
    return DVS_OK;
}

extern "C" int dvs_pairs_get(const dvs_pairs *p, uint64_t *row_start, uint32_t *col, double *dist) {
    if (!p) return DVS_ERR_VALUE;
    if (row_start) std::copy(p->row_start.begin(), p->row_start.end(), row_start);
    if (col) std::copy(p->col.begin(), p->col.end(), col);
    if (dist) std::copy(p->dist.begin(), p->dist.end(), dist);
    return DVS_OK;
}

extern "C" int dvs_threshold_clusters(dvs_ctx *ctx, const dvs_source *src, double radius, uint32_t *labels,
                                      uint32_t *n_clusters) {
    if (int rc = dvs_source_check(ctx, src, src)) return rc;
    return cross_to_threshold_clusters(ctx, source_cross_stage(ctx, src, src), radius, labels, n_clusters);
}
