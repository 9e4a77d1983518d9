// Distances between two collections -- M query rows against N reference rows -- in the three modes of the square
// path (rowdist.hip, mash.hip), and the driver of everything that reads them.  No counterpart in the reference, whose
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
// strip driver (dvs_strip_run) walks the queries strip by strip with a consumer (dvs_strip_consumer) behind each: the host
// matrix (here), the kk nearest references per query (nearest.hip), the coordinates in a fitted ordination (pcoa.hip),
// or (queries = references) the scores of a labelling of the rows (clusters.hip), the correlation of the distances
// with a tree's cophenetic distances (cophenet.hip), the list of the cells within a radius and the connected
// components they make (within.hip), the minimum spanning tree (mst.hip: one pass of the strips per Boruvka round).  Every C entry of these operations is at the end of this file, as rowdist.hip
// keeps the square ones.  The strip is CROSS_STRIP_BYTES at most (and a tile row of 32 queries at least).
#include "dvs_internal.h"
#include "rowdist_dev.h"

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

namespace {

constexpr uint32_t NONE = DVS_NONE;
constexpr size_t CROSS_STRIP_BYTES = size_t(256) << 20;  // the strip buffer's bound

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

// ---- the strip driver

// query rows per strip: what CROSS_STRIP_BYTES holds, in whole tile rows and one tile row at least; or the knob
uint32_t strip_rows(const dvs_ctx *ctx, const dvs_cross_stage &st) {
    uint64_t rows = ctx->knobs.cross_strip_rows;
    if (!rows) rows = std::max<uint64_t>(CROSS_STRIP_BYTES / (size_t(st.n) * 8) / JSD_TILE * JSD_TILE, JSD_TILE);
    return uint32_t(std::min<uint64_t>(rows, st.m));
}

}  // namespace

// A stage strip by strip on the context's stream, and a consumer (dvs_internal.h dvs_strip_consumer) run over it: the
// stage's own check; the device; the strip and the stage's scratch; the stage's prepare; the consumer's begin; behind
// each strip's distance kernels the consumer's strip, until the queries or the consumer's wish for more (stop) run out.
// From the first enqueue on every path, failed or not, goes through the ONE hipStreamSynchronize below before a block
// goes back to the cache or the caller lets go of the host memory an upload reads; on DVS_OK what the consumer copied
// to the host has arrived.
int dvs_strip_run(dvs_ctx *ctx, const dvs_cross_stage &st, const dvs_strip_consumer &c) {
    if (int rc = st.check()) return rc;
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t rows = strip_rows(ctx, st);
    PooledBuf d_strip{ctx}, d_scratch{ctx};
    int rc = dvs_dev_alloc(ctx, &d_strip.p, size_t(rows) * st.n * 8, "distance strip");
    if (!rc && st.scratch_bytes) rc = dvs_dev_alloc(ctx, &d_scratch.p, st.scratch_bytes, st.scratch_what);
    if (rc) return rc;
    hipError_t e = st.prepare(d_scratch.p);
    if (e == hipSuccess && c.begin) rc = c.begin(rows);
    for (uint64_t q0 = 0; !rc && e == hipSuccess && q0 < st.m && !(c.stop && *c.stop); q0 += rows) {
        const uint32_t mq = uint32_t(std::min<uint64_t>(rows, st.m - q0));
        e = st.enqueue(uint32_t(q0), mq, d_strip.as<double>(), d_scratch.p);
        if (e == hipSuccess) e = c.strip(uint32_t(q0), mq, d_strip.as<double>());
    }
    uint32_t flag = 0;
    if (!rc && e == hipSuccess && st.scratch_is_zerodiv)
        e = hipMemcpyAsync(&flag, d_scratch.p, 4, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t se = hipStreamSynchronize(ctx->stream);
    if (rc) return rc;
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, st.label);
    if (se != hipSuccess) return dvs_hip_fail(ctx, se, st.label);
    if (flag) return dvs_set_error(ctx, DVS_ERR_ZERODIV, "division by zero");  // 0 / 0, distance.py:283
    return DVS_OK;
}

// the m x n matrix of a stage into the host array dist
static int cross_to_host(dvs_ctx *ctx, const dvs_cross_stage &st, double *dist) {
    if (st.m == 0 || st.n == 0) return DVS_OK;
    if (!dist) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    dvs_strip_consumer c{};
    c.strip = [&](uint32_t q0, uint32_t mq, double *d_strip) {
        return hipMemcpyAsync(dist + size_t(q0) * st.n, d_strip, size_t(mq) * st.n * 8, hipMemcpyDeviceToHost, ctx->stream);
    };
    return dvs_strip_run(ctx, st, c);
}

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

// ---- the entries: a source or two (include/dvs_hip.h dvs_source), checked, as a stage of the strip driver above

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
    return dvs_nearest_strips(ctx, source_cross_stage(ctx, q, r), kk, idx, dist);
}

extern "C" int dvs_pcoa_project(dvs_ctx *ctx, const dvs_source *q, const dvs_source *r, uint32_t n_axes, const double *values,
                                const double *vectors, const double *row_means, double *coords) {
    if (int rc = dvs_source_check(ctx, q, r)) return rc;
    if (q->kind == DVS_SRC_GIVEN) return dvs_source_refuse(ctx, "dvs_pcoa_project", q, "the matrix");
    return dvs_pcoa_project_strips(ctx, source_cross_stage(ctx, q, r), n_axes, values, vectors, row_means, coords);
}

extern "C" int dvs_cluster_scores(dvs_ctx *ctx, const dvs_source *src, const uint32_t *labels, uint32_t n_clusters,
                                  double *within, double *a, double *b, uint32_t *neighbour, double *silhouette,
                                  uint32_t *medoids) {
    if (int rc = dvs_source_check(ctx, src, src)) return rc;
    return dvs_cluster_scores_strips(ctx, source_cross_stage(ctx, src, src), labels, n_clusters, within, a, b, neighbour,
                                     silhouette, medoids);
}

extern "C" int dvs_cophenet(dvs_ctx *ctx, const dvs_source *src, const uint32_t *pairs, const double *heights, double *corr,
                            double *row_sums, double *coph) {
    if (int rc = dvs_source_check(ctx, src, src)) return rc;
    return dvs_cophenet_strips(ctx, source_cross_stage(ctx, src, src), pairs, heights, corr, row_sums, coph);
}

extern "C" int dvs_within(dvs_ctx *ctx, const dvs_source *q, const dvs_source *r, double radius, uint32_t flags,
                          uint64_t max_pairs, dvs_pairs **out) {
    if (out) *out = nullptr;
    if (!r && q && q->kind == DVS_SRC_GIVEN) r = q;  // a caller's matrix is both sides
    if (int rc = dvs_source_check(ctx, q, r)) return rc;
    if (q->kind == DVS_SRC_GIVEN && (r->handle != q->handle || r->n != q->n || r->on_device != q->on_device))
        return dvs_source_refuse(ctx, "dvs_within", q, "another matrix as the references");
    return dvs_within_strips(ctx, source_cross_stage(ctx, q, r), radius, flags, max_pairs, out);
}

extern "C" int dvs_threshold_clusters(dvs_ctx *ctx, const dvs_source *src, double radius, uint32_t *labels,
                                      uint32_t *n_clusters) {
    if (int rc = dvs_source_check(ctx, src, src)) return rc;
    return dvs_threshold_clusters_strips(ctx, source_cross_stage(ctx, src, src), radius, labels, n_clusters);
}

extern "C" int dvs_mst(dvs_ctx *ctx, const dvs_source *src, const double *core, uint32_t *edges, double *weights,
                       uint32_t *n_edges, uint32_t *n_rounds) {
    if (int rc = dvs_source_check(ctx, src, src)) return rc;
    return dvs_mst_strips(ctx, source_cross_stage(ctx, src, src), core, edges, weights, n_edges, n_rounds);
}
