// Pairwise distances between the rows of a k-mer matrix -- the Jensen-Shannon divergence and the euclidean distance
// (diverse_seq/distance.py:294-336) -- and the drivers every ctree distance mode goes through: rows of a matrix to a
// host N x N array, and a whole source to a consumer of its N x N matrix (the linkage tree, the neighbour-joining tree,
// the principal coordinates, k-medoids) with the matrix left in HBM.
//
// The Jensen-Shannon divergence:
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
#include "rowdist_dev.h"  // the tile shape and the per-bin term, shared with the rectangular kernels (crossdist.hip)

#include <type_traits>

namespace {

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

// ||f_i - f_j||_2 (diverse_seq/distance.py:335-336), f = counts / total.  Workgroup (i, g) stages row
// i's frequencies in LDS chunk by chunk and its eight waves take the rows j = 8 g .. 8 g + 7 below the
// diagonal, one each: row i is read once per eight pairs, row j streamed by one wave with 16-byte loads
// where the bin count allows.  Only the lower triangle does work; both mirror cells are written.
template <typename T>
__global__ __launch_bounds__(EUC_THREADS) void euclid_kernel(const T *__restrict__ mat,
                                                            const uint32_t *__restrict__ totals, uint64_t B,
                                                            uint32_t n, double *__restrict__ dist) {
    __shared__ double fi[EUC_CHUNK];
    const uint32_t i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t j = blockIdx.y * (EUC_THREADS / 64) + wave;
    if (blockIdx.y * (EUC_THREADS / 64) >= i) return;  // the whole group is on or above the diagonal
    const T *a = mat + uint64_t(i) * B;
    const bool live = j < i;
    const T *b = mat + uint64_t(live ? j : 0) * B;
    const double ta = double(totals[i]), tb = double(totals[live ? j : 0]);
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
    if (live && lane == 0) {
        const double d = sqrt(acc);
        dist[uint64_t(i) * n + j] = d;
        dist[uint64_t(j) * n + i] = d;
    }
}

// ---- the modes over the rows of a matrix (the mash mode: mash.hip dvs_mash_stage)

// both limits of a count-matrix mode: euclid_kernel's grid has a workgroup per EUC_THREADS / 64 rows in y, 65 535 of
// them at most, and the jsd mode keeps the same limit
int rows_check(dvs_ctx *ctx, uint32_t n) {
    if ((n + EUC_THREADS / 64 - 1) / (EUC_THREADS / 64) > 65535u)
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "%u rows: the %u x %u distance matrix is beyond this path", n, n, n);
    return DVS_OK;
}

// the two jsd kernels write every cell, the diagonal included; their scratch is the n row entropies
dvs_dist_stage jsd_stage(dvs_ctx *ctx, const dvs_matrix *m) {
    const uint32_t n = m->nrows;
    dvs_dist_stage st{"jsd distances", n};
    st.check = [=] { return rows_check(ctx, n); };
    st.scratch_bytes = size_t(n) * 8;
    st.scratch_what = "row entropies";
    st.enqueue = [=](double *d_dist, void *d_scratch) {
        double *d_h = static_cast<double *>(d_scratch);
        const uint32_t tiles = (n + JSD_TILE - 1) / JSD_TILE;
        const dim3 grid(tiles, tiles);
        dvs_mat_dispatch(m, [&](auto *mp) {
            using T = std::remove_cv_t<std::remove_pointer_t<decltype(mp)>>;
            hipLaunchKernelGGL((jsd_pairs_kernel<T>), grid, dim3(JSD_THREADS), 0, ctx->stream, mp, m->d_totals, m->nbins,
                               n, d_dist, d_h);
            return 0;
        });
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(jsd_finish_kernel, grid, dim3(JSD_THREADS), 0, ctx->stream, m->d_totals, d_h, n, d_dist);
        return hipGetLastError();
    };
    return st;
}

// euclid_kernel writes every cell off the diagonal and needs no scratch
dvs_dist_stage euclid_stage(dvs_ctx *ctx, const dvs_matrix *m) {
    const uint32_t n = m->nrows;
    dvs_dist_stage st{"euclidean distances", n};
    st.check = [=] { return rows_check(ctx, n); };
    st.zero_diagonal = true;
    st.enqueue = [=](double *d_dist, void *) {
        const dim3 grid(n, (n + EUC_THREADS / 64 - 1) / (EUC_THREADS / 64));
        dvs_mat_dispatch(m, [&](auto *mp) {
            using T = std::remove_cv_t<std::remove_pointer_t<decltype(mp)>>;
            hipLaunchKernelGGL((euclid_kernel<T>), grid, dim3(EUC_THREADS), 0, ctx->stream, mp, m->d_totals, m->nbins, n,
                               d_dist);
            return 0;
        });
        return hipGetLastError();
    };
    return st;
}

// ---- the drivers.  stage_enqueue: what both go through; stage_to_host: a mode's matrix to a host array; square_run
// (behind the sources below, which it takes as they are): a whole matrix, left in HBM, to its consumer

// The matrix and the mode's scratch from the context's cache, then the mode's kernels, behind a zeroed diagonal where
// they leave it alone: DVS_OK with everything enqueued and nothing waited for, or the error (the stream drained, so
// that the caller may let go of the two blocks).
int stage_enqueue(dvs_ctx *ctx, const dvs_dist_stage &st, PooledBuf *d_dist, PooledBuf *d_scratch) {
    const size_t n = st.n;
    int rc = dvs_dev_alloc(ctx, &d_dist->p, n * n * 8, "distance matrix");
    if (!rc && st.scratch_bytes) rc = dvs_dev_alloc(ctx, &d_scratch->p, st.scratch_bytes, st.scratch_what);
    if (rc) return rc;
    hipError_t e = st.zero_diagonal ? hipMemset2DAsync(d_dist->p, (n + 1) * 8, 0, 8, n, ctx->stream) : hipSuccess;
    if (e == hipSuccess) e = st.enqueue(d_dist->as<double>(), d_scratch->p);
    if (e == hipSuccess) return DVS_OK;
    (void)hipStreamSynchronize(ctx->stream);
    return dvs_hip_fail(ctx, e, st.label);
}

// the distances of a count-matrix mode into the host array dist (n x n)
int stage_to_host(dvs_ctx *ctx, const dvs_dist_stage &st, double *dist) {
    if (st.n == 0) return DVS_OK;
    if (st.n == 1) {
        dist[0] = 0.0;
        return DVS_OK;
    }
    if (int rc = st.check()) return rc;
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    PooledBuf d_dist{ctx}, d_scratch{ctx};
    if (int rc = stage_enqueue(ctx, st, &d_dist, &d_scratch)) return rc;
    const hipError_t e = hipMemcpyAsync(dist, d_dist.p, size_t(st.n) * st.n * 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t se = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, st.label);
    if (se != hipSuccess) return dvs_hip_fail(ctx, se, st.label);
    return DVS_OK;
}

}  // namespace

int dvs_rows_check(dvs_ctx *ctx, uint32_t n) { return rows_check(ctx, n); }

// ---- what every operation over a whole n x n matrix shares (dvs_internal.h)

int dvs_square_fits(dvs_ctx *ctx, const char *op, uint32_t n, bool need_matrix, size_t extra_bytes, const char *extra_what) {
    const char *sep = op ? ": " : "";
    if (!op) op = "";
    const uint64_t n2 = uint64_t(n) * n;
    if (n2 > (uint64_t(1) << 58))
        return dvs_set_error(ctx, DVS_ERR_NOMEM, "%s%sa %u x %u distance matrix does not fit in memory", op, sep, n, n);
    const size_t bytes = (need_matrix ? size_t(n2) * 8 : 0) + extra_bytes;
    size_t free_b = 0, total_b = 0;
    DVS_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    if (bytes + (64u << 20) > free_b + ctx->pool_bytes)
        return dvs_set_error(ctx, DVS_ERR_NOMEM, "%s%sa %u x %u distance matrix and %s need %zu bytes of HBM, %zu free", op, sep,
                             n, n, extra_what, bytes, free_b);
    return DVS_OK;
}

int dvs_given_on_device(dvs_ctx *ctx, const char *op, const void *dist) {
    const char *sep = op ? ": " : "";
    if (!op) op = "";
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, dist) != hipSuccess) {
        (void)hipGetLastError();  // clear the sticky error
        return dvs_set_error(ctx, DVS_ERR_VALUE, "%s%sthe distance matrix is not device memory", op, sep);
    }
    if (attr.device != ctx->device)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "%s%sthe distance matrix is on device %d, the context on device %d", op, sep,
                             attr.device, ctx->device);
    return DVS_OK;
}

int dvs_given_upload(dvs_ctx *ctx, const double *dist, uint32_t n, PooledBuf *d_dist) {
    if (int rc = dvs_dev_alloc(ctx, &d_dist->p, size_t(n) * n * 8, "distance matrix")) return rc;
    const hipError_t e = hipMemcpyAsync(d_dist->p, dist, size_t(n) * n * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) return DVS_OK;
    (void)hipStreamSynchronize(ctx->stream);
    return dvs_hip_fail(ctx, e, "distance matrix upload");
}

// ---- a source (include/dvs_hip.h dvs_source): what every entry checks first, and the source as a stage

static const char *const SRC_KIND[] = {"mash", "euclidean", "jsd", "given"};

int dvs_source_check(dvs_ctx *ctx, const dvs_source *q, const dvs_source *r) {
    if (!ctx || !q || !r) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    for (const dvs_source *s : {q, r}) {
        if (s->kind > DVS_SRC_GIVEN) return dvs_set_error(ctx, DVS_ERR_VALUE, "unknown source kind %u", s->kind);
        if (!s->handle && !(s->kind == DVS_SRC_GIVEN && s->n == 0)) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
        if (s->kind == DVS_SRC_GIVEN && s->rows)
            return dvs_set_error(ctx, DVS_ERR_VALUE, "a caller's distance matrix takes no row list");
    }
    if (q->kind != r->kind)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "a %s source against a %s source", SRC_KIND[q->kind], SRC_KIND[r->kind]);
    if (q->kind == DVS_SRC_MASH && (q->k != r->k || q->sketch_size != r->sketch_size))
        return dvs_set_error(ctx, DVS_ERR_VALUE, "sketches of k = %u, sketch size %u against k = %u, sketch size %u", q->k,
                             q->sketch_size, r->k, r->sketch_size);
    return DVS_OK;
}

int dvs_source_refuse(dvs_ctx *ctx, const char *op, const dvs_source *src, const char *what) {
    return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "%s: %s of a %s source", op, what, SRC_KIND[src->kind]);
}

int dvs_source_whole(dvs_ctx *ctx, const char *op, const dvs_source *src) {
    if (src->rows) return dvs_source_refuse(ctx, op, src, "a row list");
    const uint32_t rows = src->kind == DVS_SRC_MASH ? dvs_sketches_nseq(dvs_src_sketches(src))
                          : src->kind == DVS_SRC_GIVEN ? src->n : dvs_src_matrix(src)->nrows;
    if (src->n != rows) return dvs_source_refuse(ctx, op, src, "some of the rows");
    return DVS_OK;
}

// a MASH, EUCLIDEAN or JSD source, whole, as a stage of the drivers above
static dvs_dist_stage source_stage(dvs_ctx *ctx, const dvs_source *src) {
    if (src->kind == DVS_SRC_MASH) return dvs_mash_stage(ctx, dvs_src_sketches(src), src->k, src->sketch_size);
    return src->kind == DVS_SRC_JSD ? jsd_stage(ctx, dvs_src_matrix(src)) : euclid_stage(ctx, dvs_src_matrix(src));
}

extern "C" int dvs_distances(dvs_ctx *ctx, const dvs_source *src, double *dist) {
    if (int rc = dvs_source_check(ctx, src, src)) return rc;
    if (!dist) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (src->kind == DVS_SRC_GIVEN) return dvs_source_refuse(ctx, "dvs_distances", src, "the matrix");
    if (int rc = dvs_source_whole(ctx, "dvs_distances", src)) return rc;
    if (src->kind == DVS_SRC_MASH)  // (the pair kernel on the caller's diagonal, as Sketches.distances always ran it)
        return dvs_sketches_distances(ctx, dvs_src_sketches(src), src->k, src->sketch_size, 0, 1, 1, dist);
    return stage_to_host(ctx, source_stage(ctx, src), dist);
}

// The square driver: a whole source (checked by its entry) brought to the device as an n x n matrix, and a consumer
// run over it (dvs_internal.h dvs_square_consumer: the linkage tree of ctree, diverse_seq/cluster.py:164-188, 216-233,
// and what else reads a whole matrix).  A matrix the library measures never crosses PCIe: the mode's kernels write it
// into a block of the cache and the consumer enqueues behind them.  The checks come in one order whatever the
// consumer: its arguments and n; its early answer and the mode's own check (a MASH, EUCLIDEAN or JSD source); the
// device; the pointer (a caller's device matrix, used where it is); the fit in HBM.
//
// The bringing half, which dvs_mantel goes through twice: a whole source as an n x n matrix in HBM.  The steps in
// front of the fit -- the mode's own check (a MASH, EUCLIDEAN or JSD source), the pointer (a caller's device matrix)
// -- and source_bring behind it, which gives the device pointer, the block it owns (none: a caller's device matrix,
// used where it is) and the zero-division word.
struct SquareBrought {
    dvs_dist_stage st{};  // of a MASH, EUCLIDEAN or JSD source
    PooledBuf d_dist, d_scratch;
    double *dist = nullptr;
    const uint32_t *d_zerodiv = nullptr;
    explicit SquareBrought(dvs_ctx *ctx) : d_dist{ctx}, d_scratch{ctx} {}
    bool owned() const { return d_dist.p != nullptr; }
};
static bool source_needs_block(const dvs_source *src) { return !(src->kind == DVS_SRC_GIVEN && src->on_device); }
static int source_own_check(dvs_ctx *ctx, const dvs_source *src, SquareBrought *b) {
    if (src->kind == DVS_SRC_GIVEN) return DVS_OK;
    b->st = source_stage(ctx, src);
    return b->st.check();
}
static int source_pointer_check(dvs_ctx *ctx, const char *op, const dvs_source *src) {
    return src->kind == DVS_SRC_GIVEN && src->on_device ? dvs_given_on_device(ctx, op, src->handle) : DVS_OK;
}
static int source_bring(dvs_ctx *ctx, const dvs_source *src, SquareBrought *b) {
    b->dist = static_cast<double *>(src->handle);
    if (src->kind != DVS_SRC_GIVEN) {
        if (int rc = stage_enqueue(ctx, b->st, &b->d_dist, &b->d_scratch)) return rc;
        if (b->st.scratch_is_zerodiv) b->d_zerodiv = b->d_scratch.as<uint32_t>();
    } else if (!src->on_device) {
        if (int rc = dvs_given_upload(ctx, b->dist, src->n, &b->d_dist)) return rc;
    }
    if (b->owned()) b->dist = b->d_dist.as<double>();
    return DVS_OK;
}

static int square_run(dvs_ctx *ctx, const dvs_source *src, const dvs_square_consumer &c) {
    if (int rc = c.check()) return rc;
    SquareBrought b(ctx);
    if (src->kind != DVS_SRC_GIVEN && c.early && c.early()) return DVS_OK;
    if (int rc = source_own_check(ctx, src, &b)) return rc;
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = source_pointer_check(ctx, c.name, src)) return rc;
    if (int rc = dvs_square_fits(ctx, c.name, src->n, source_needs_block(src), c.extra_bytes(), c.extra_what)) return rc;
    if (int rc = source_bring(ctx, src, &b)) return rc;
    const int rc = c.run(b.dist, b.d_zerodiv);
    // (the one place that keeps PooledBuf's contract for the matrix: a run that failed may have left the kernels that
    // write it, or its own that read it, queued)
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

extern "C" int dvs_linkage(dvs_ctx *ctx, const dvs_source *src, int method, uint32_t *pairs, double *heights,
                           uint32_t *sizes) {
    if (int rc = dvs_source_check(ctx, src, src)) return rc;
    if (!pairs || !heights || !sizes) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (int rc = dvs_source_whole(ctx, "dvs_linkage", src)) return rc;
    return square_run(ctx, src, dvs_linkage_consumer(ctx, src->n, src->kind == DVS_SRC_GIVEN, method, pairs, heights, sizes));
}

extern "C" int dvs_nj(dvs_ctx *ctx, const dvs_source *src, uint32_t *joins, double *lengths) {
    if (int rc = dvs_source_check(ctx, src, src)) return rc;
    if (!joins || !lengths) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (int rc = dvs_source_whole(ctx, "dvs_nj", src)) return rc;
    return square_run(ctx, src, dvs_nj_consumer(ctx, src->n, joins, lengths));
}

extern "C" int dvs_pcoa(dvs_ctx *ctx, const dvs_source *src, const dvs_pcoa_params *params, double *values, double *vectors,
                        double *residuals, double *row_means, dvs_pcoa_info *info) {
    if (int rc = dvs_source_check(ctx, src, src)) return rc;
    if (!params || !values || !vectors || !residuals || !row_means || !info) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (int rc = dvs_source_whole(ctx, "dvs_pcoa", src)) return rc;
    return square_run(ctx, src, dvs_pcoa_consumer(ctx, src->n, params, values, vectors, residuals, row_means, info));
}

extern "C" int dvs_kmedoids(dvs_ctx *ctx, const dvs_source *src, const dvs_kmedoids_params *params, uint32_t *medoids,
                            uint32_t *labels, double *dist, double *second, uint32_t *swaps, double *td, dvs_kmedoids_info *info) {
    if (!ctx || !src) return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_kmedoids: null argument");
    if (int rc = dvs_source_check(ctx, src, src)) return rc;
    if (!params || !medoids || !labels || !dist || !info) return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_kmedoids: null argument");
    if (int rc = dvs_source_whole(ctx, "dvs_kmedoids", src)) return rc;
    const dvs_kmedoids_out out{medoids, labels, dist, second, swaps, td, info};
    return square_run(ctx, src, dvs_kmedoids_consumer(ctx, src->n, src->kind == DVS_SRC_GIVEN, params, out));
}

extern "C" int dvs_permanova(dvs_ctx *ctx, const dvs_source *src, const uint32_t *labels, uint32_t n_groups,
                             const uint32_t *perm_labels, uint32_t n_perm, double *ss_total, double *ss_within, double *group_ss,
                             dvs_permanova_info *info) {
    if (!ctx || !src) return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_permanova: null argument");
    if (int rc = dvs_source_check(ctx, src, src)) return rc;
    if (int rc = dvs_source_whole(ctx, "dvs_permanova", src)) return rc;
    const dvs_permanova_args args{labels, n_groups, perm_labels, n_perm, ss_total, ss_within, group_ss, info};
    return square_run(ctx, src, dvs_permanova_consumer(ctx, src->n, args));
}

// Two whole sources, of any two kinds, brought side by side (include/dvs_hip.h "Mantel"): the arguments and n, x's own
// check, y's own check, the device, the pointers, ONE fit for both matrices, y's working copy and the state, then x, y
// and the run (mantel.hip).
extern "C" int dvs_mantel(dvs_ctx *ctx, const dvs_source *x, const dvs_source *y, const uint32_t *perms, uint32_t n_perm,
                          double *moments, double *z, dvs_mantel_info *info) {
    const char *op = "dvs_mantel";
    if (!ctx || !x || !y) return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_mantel: null argument");
    if (int rc = dvs_source_check(ctx, x, x)) return rc;
    if (int rc = dvs_source_check(ctx, y, y)) return rc;
    if (!moments || !z || (n_perm != 0) != (perms != nullptr))
        return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_mantel: null argument (perms is NULL exactly when n_perm is 0)");
    if (x->n != y->n) return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_mantel: %u rows against %u rows", x->n, y->n);
    const uint32_t n = x->n;
    if (n < 3) return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_mantel: %u rows: three at least", n);
    if (int rc = dvs_source_whole(ctx, op, x)) return rc;
    if (int rc = dvs_source_whole(ctx, op, y)) return rc;
    SquareBrought bx(ctx), by(ctx);
    if (int rc = source_own_check(ctx, x, &bx)) return rc;
    if (int rc = source_own_check(ctx, y, &by)) return rc;
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = source_pointer_check(ctx, op, x)) return rc;
    if (int rc = source_pointer_check(ctx, op, y)) return rc;
    char what[64];
    snprintf(what, sizeof what, "the second matrix and the sums of %u permutations", n_perm);
    const uint64_t n2 = uint64_t(n) * n;
    if (n2 > (uint64_t(1) << 58)) return dvs_square_fits(ctx, op, n, true, 0, what);  // (its own message)
    if (int rc = dvs_square_fits(ctx, op, n, source_needs_block(x), size_t(n2) * 8 + dvs_mantel_state_bytes(ctx, n, n_perm), what))
        return rc;
    int rc = source_bring(ctx, x, &bx);
    if (!rc) rc = source_bring(ctx, y, &by);
    if (!rc) rc = dvs_mantel_run(ctx, n, bx.dist, by.dist, by.owned(), bx.d_zerodiv, by.d_zerodiv, dvs_mantel_args{perms, n_perm, moments, z, info});
    // (as square_run: a step that failed may have left the kernels that write a matrix, or the run's own, queued)
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}
