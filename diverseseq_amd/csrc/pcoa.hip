// Principal coordinates (PCoA, classical MDS) of an n x n distance matrix on the device: include/dvs_hip.h "principal
// coordinates", DESIGN.md 4.16.  The few algebraically largest eigenpairs of B = J A J, A = -1/2 D o D, J = I - 11^T / n,
// by a block Krylov iteration with full orthogonalisation and Rayleigh-Ritz:
//
//   the basis Q (n x dim, orthonormal, every column orthogonal to 1) and B Q beside it, both column-major in HBM;
//   a step multiplies the newest block by B (pcoa_product_kernel: the one pass over the matrix, which squares the cells
//   as it reads them, then B x = A x - mean(A x) 1 since x is orthogonal to 1), takes the new block column of
//   T = Q^T B Q (pcoa_dots_kernel), solves the small dense problem on the host (pcoa_host.cpp), forms the leading Ritz
//   vectors and their TRUE residuals B v - theta v from Q and B Q (pcoa_ritz_kernel: no further pass over the
//   matrix), and unless they are small enough makes the next block: every column of B Q_new orthogonalised against
//   the whole basis twice (classical Gram-Schmidt, twice: CGS2), centred, normalised.  A column that all but vanishes
//   -- an invariant subspace, a constant matrix, n < 2 b -- is replaced by a fresh hashed vector; the iteration ends
//   only when the leading pairs have converged or the basis has reached its limit (at n - 1 columns it spans the whole
//   complement of 1 and the Ritz pairs are exact).
//
// The matrix is only READ.  Every reduction -- the row dot products, the column means, the Gram products, the norms --
// adds its terms in an order that n and the block shape fix: a lane (thread) its strided terms in ascending order, the
// lanes by the xor-shuffle tree, the waves in wave order.  No float atomics: the same bits on every run.
//
// Further rows are placed in a fitted ordination by pcoa_project_kernel, behind the strip driver (crossdist.hip dvs_strip_run).
#include "dvs_internal.h"
#include "pcoa_host.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr uint32_t PCOA_BLOCK = 16;        // b: columns of a block (DESIGN.md 4.16 has the other shapes' times)
constexpr uint32_t PCOA_ROWS = 4;          // matrix rows a wave of the product kernel carries at once
constexpr uint32_t PCOA_THREADS = 256;
constexpr uint32_t PCOA_WAVES = PCOA_THREADS / 64;
constexpr uint32_t PCOA_MAX_AXES = 64;
constexpr uint32_t PCOA_MAX_BASIS = 512;   // the default limit of the basis (and the most a caller may ask for: 4096)
constexpr uint32_t PCOA_BASIS_CAP = 4096;
constexpr uint32_t PCOA_AXIS_CHUNK = 8;    // Ritz vectors a thread of pcoa_ritz_kernel carries at once
constexpr uint32_t PCOA_TILE = 32;         // the prepare pass's tiles
// a column of the next block whose norm, after the orthogonalisation, is below this fraction of the largest column
// norm of B Q seen so far (the block's own included) is replaced by a hashed vector
constexpr double PCOA_RANK_TOL = 1e-10;
// ... and a hashed vector that keeps less than this fraction of its own norm is dropped for the next one
constexpr double PCOA_HASH_TOL = 1e-6;
// the small problem is solved after every step while the basis has at most this many columns, after every fourth
// step beyond (0.7 s of host time at 512 columns: DESIGN.md 4.16)
constexpr uint32_t PCOA_SOLVE_EVERY_STEP = 256;

constexpr uint32_t PCOA_NONFINITE = 1, PCOA_ASYMMETRIC = 2;

// ---- the prepare pass, one read of the matrix: every off-diagonal entry finite, D[i][j] == D[j][i] bit for bit, and
// the row sums of d^2

// the sum of a value over the 32 lanes of a tile row (half a wave: the xor offsets stay inside it); every lane gets it
__device__ __forceinline__ double pcoa_half_wave_sum(double v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One 32 x 32 tile pair (bi >= bj) per workgroup: the upper tile (bj, bi) goes through LDS and is compared, transposed,
// with the lower tile (bi, bj).  The diagonal is not read.  Every tile also leaves the sums of d^2 over its 32 columns,
// row by row, in partial[tile column][row]: each (tile column, row) has exactly one writer -- the upper pass of
// workgroup (tile column, tile row) on and above the diagonal of tiles, the lower pass of (tile row, tile column)
// below it -- and a sum is the fixed tree over the row's 32 lanes.
__global__ __launch_bounds__(256) void pcoa_check_kernel(const double *__restrict__ D, uint32_t n,
                                                         uint32_t *__restrict__ status, double *__restrict__ partial) {
    __shared__ double s_up[PCOA_TILE][PCOA_TILE + 1];
    const uint32_t bi = blockIdx.x, bj = blockIdx.y;
    if (bj > bi) return;
    const uint32_t tx = threadIdx.x & (PCOA_TILE - 1), ty = threadIdx.x / PCOA_TILE;  // 32 x 8
    bool bad = false, asym = false;
    for (uint32_t r = ty; r < PCOA_TILE; r += 256 / PCOA_TILE) {
        const uint32_t row = bj * PCOA_TILE + r, col = bi * PCOA_TILE + tx;
        double v = 0.0;
        if (row < n && col < n && row != col) {
            v = D[size_t(row) * n + col];
            bad |= !__builtin_isfinite(v);
        }
        s_up[r][tx] = v;
        const double sum = pcoa_half_wave_sum(v * v);
        if (tx == 0 && row < n) partial[size_t(bi) * n + row] = sum;
    }
    __syncthreads();
    if (bi != bj)  // lower entry (bi * 32 + r, bj * 32 + tx) against upper entry (bj * 32 + tx, bi * 32 + r)
        for (uint32_t r = ty; r < PCOA_TILE; r += 256 / PCOA_TILE) {
            const uint32_t row = bi * PCOA_TILE + r, col = bj * PCOA_TILE + tx;
            double v = 0.0;
            if (row < n && col < n) {
                v = D[size_t(row) * n + col];
                bad |= !__builtin_isfinite(v);
                asym |= __double_as_longlong(v) != __double_as_longlong(s_up[tx][r]);
            }
            const double sum = pcoa_half_wave_sum(v * v);
            if (tx == 0 && row < n) partial[size_t(bj) * n + row] = sum;
        }
    else  // a diagonal tile is its own mirror image: the entries below the diagonal against those above
        for (uint32_t r = ty; r < PCOA_TILE; r += 256 / PCOA_TILE)
            if (r > tx) asym |= __double_as_longlong(s_up[r][tx]) != __double_as_longlong(s_up[tx][r]);
    if (bad) atomicOr(status, PCOA_NONFINITE);
    if (asym) atomicOr(status, PCOA_ASYMMETRIC);
}

// rowsum[i] = sum over j != i of D[i][j]^2 from the tiles' partial sums: 32 rows a workgroup, eight threads a row; a
// thread adds the tile columns t = q, q + 8, ... in ascending order, the eight by a fixed pairwise tree
__global__ __launch_bounds__(PCOA_THREADS) void pcoa_rowsum_kernel(const double *__restrict__ partial, uint32_t n,
                                                                   uint32_t tiles, double *__restrict__ rowsum) {
    __shared__ double s_q[8][32];
    const uint32_t rr = threadIdx.x & 31, q = threadIdx.x >> 5, row = blockIdx.x * 32 + rr;
    double acc = 0.0;
    if (row < n)
        for (uint32_t t = q; t < tiles; t += 8) acc += partial[size_t(t) * n + row];
    s_q[q][rr] = acc;
    __syncthreads();
    if (q == 0 && row < n)
        rowsum[row] = ((s_q[0][rr] + s_q[1][rr]) + (s_q[2][rr] + s_q[3][rr])) + ((s_q[4][rr] + s_q[5][rr]) + (s_q[6][rr] + s_q[7][rr]));
}

// ---- the hot kernel: Y[:, c] = (-1/2 D o D) X[:, c] for the nb <= PCOA_BLOCK columns of a block; X and Y column-major,
// n doubles from column to column.  A wave carries PCOA_ROWS rows: per 64 columns of the matrix it reads the block's
// 64 x nb entries once (through L2) and 64 cells of each of its rows (from HBM, coalesced along the row), two multiplies
// and nb fmas per cell.  Cell (i, i) counts as 0 and is not read.
__global__ __launch_bounds__(PCOA_THREADS) void pcoa_product_kernel(const double *__restrict__ D, uint32_t n,
                                                                    const double *__restrict__ X, uint32_t nb,
                                                                    double *__restrict__ Y) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t row0 = (blockIdx.x * PCOA_WAVES + (threadIdx.x >> 6)) * PCOA_ROWS;
    if (row0 >= n) return;  // (the whole wave)
    double acc[PCOA_ROWS][PCOA_BLOCK];
#pragma unroll
    for (uint32_t r = 0; r < PCOA_ROWS; r++)
#pragma unroll
        for (uint32_t c = 0; c < PCOA_BLOCK; c++) acc[r][c] = 0.0;
    const double *g[PCOA_ROWS];
#pragma unroll
    for (uint32_t r = 0; r < PCOA_ROWS; r++) g[r] = D + size_t(row0 + r < n ? row0 + r : n - 1) * n;  // (a row past the end: neither read nor written)
    for (uint32_t j = lane; j < n; j += 64) {
        double x[PCOA_BLOCK];
#pragma unroll
        for (uint32_t c = 0; c < PCOA_BLOCK; c++) x[c] = c < nb ? X[size_t(c) * n + j] : 0.0;
#pragma unroll
        for (uint32_t r = 0; r < PCOA_ROWS; r++) {
            const double d = j == row0 + r || row0 + r >= n ? 0.0 : g[r][j];
            const double a = -0.5 * (d * d);
#pragma unroll
            for (uint32_t c = 0; c < PCOA_BLOCK; c++) acc[r][c] = fma(a, x[c], acc[r][c]);
        }
    }
#pragma unroll
    for (uint32_t r = 0; r < PCOA_ROWS; r++)
#pragma unroll
        for (uint32_t c = 0; c < PCOA_BLOCK; c++) {
            const double s = dvs_wave_sum(acc[r][c]);
            if (lane == 0 && row0 + r < n && c < nb) Y[size_t(c) * n + row0 + r] = s;
        }
}

// a thread's strided part of a sum over the n entries of a column, then the workgroup's
template <typename F>
__device__ __forceinline__ double pcoa_column_sum(uint32_t n, double *scratch, F &&term) {
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += PCOA_THREADS) acc += term(i);
    return dvs_block_sum(acc, scratch);
}

// column c of W (a workgroup each) minus its mean
__global__ __launch_bounds__(PCOA_THREADS) void pcoa_center_kernel(double *__restrict__ W, uint32_t n) {
    __shared__ double scratch[17];
    double *w = W + size_t(blockIdx.x) * n;
    const double mean = pcoa_column_sum(n, scratch, [&](uint32_t i) { return w[i]; }) / double(n);
    for (uint32_t i = threadIdx.x; i < n; i += PCOA_THREADS) w[i] -= mean;
}

// G[r + c * ldg] = Q[:, r] . W[:, c], a workgroup per (r, c)
__global__ __launch_bounds__(PCOA_THREADS) void pcoa_dots_kernel(const double *__restrict__ Q, const double *__restrict__ W,
                                                                 uint32_t n, double *__restrict__ G, uint32_t ldg) {
    __shared__ double scratch[17];
    const double *q = Q + size_t(blockIdx.x) * n, *w = W + size_t(blockIdx.y) * n;
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += PCOA_THREADS) acc = fma(q[i], w[i], acc);
    acc = dvs_block_sum(acc, scratch);
    if (threadIdx.x == 0) G[blockIdx.x + size_t(blockIdx.y) * ldg] = acc;
}

// w -= Q[:, 0 .. nq) h, a thread per entry, the columns in ascending order
__global__ __launch_bounds__(PCOA_THREADS) void pcoa_project_out_kernel(const double *__restrict__ Q, uint32_t nq, uint32_t n,
                                                                        const double *__restrict__ h, double *__restrict__ w) {
    const uint32_t i = blockIdx.x * PCOA_THREADS + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;
    for (uint32_t r = 0; r < nq; r++) acc = fma(h[r], Q[size_t(r) * n + i], acc);
    w[i] -= acc;
}

// out = w / *norm2's square root
__global__ __launch_bounds__(PCOA_THREADS) void pcoa_normalise_kernel(const double *__restrict__ w, uint32_t n,
                                                                      const double *__restrict__ norm2, double *__restrict__ out) {
    const uint32_t i = blockIdx.x * PCOA_THREADS + threadIdx.x;
    if (i < n) out[i] = w[i] / sqrt(*norm2);
}

// The start and replacement vectors: a counter-based hash of (row, column id) -- no generator state, nothing of the
// clock -- as a value in [-1/2, 1/2)
__global__ __launch_bounds__(PCOA_THREADS) void pcoa_hash_kernel(double *__restrict__ w, uint32_t n, uint32_t id) {
    const uint32_t i = blockIdx.x * PCOA_THREADS + threadIdx.x;
    if (i >= n) return;
    uint64_t h = uint64_t(i) * 0x9E3779B97F4A7C15ull + uint64_t(id) * 0xBF58476D1CE4E5B9ull + 1ull;
    h ^= h >> 31;
    h *= 0x94D049BB133111EBull;
    h ^= h >> 29;
    w[i] = double(h >> 11) * 0x1p-53 - 0.5;
}

// The Ritz vectors v_a = Q y_a (into V, n x m row-major) and their residuals B v_a - theta_a v_a = (B Q) y_a - theta_a v_a
// (into R, column-major) for the axes [blockIdx.y * 8, ...): a thread per row, the basis columns in ascending order.
// Y: dim x m column-major.
__global__ __launch_bounds__(PCOA_THREADS) void pcoa_ritz_kernel(const double *__restrict__ Q, const double *__restrict__ BQ,
                                                                 uint32_t n, uint32_t dim, const double *__restrict__ Y,
                                                                 const double *__restrict__ theta, uint32_t m,
                                                                 double *__restrict__ V, double *__restrict__ R) {
    const uint32_t i = blockIdx.x * PCOA_THREADS + threadIdx.x, a0 = blockIdx.y * PCOA_AXIS_CHUNK;
    if (i >= n) return;
    double v[PCOA_AXIS_CHUNK], bv[PCOA_AXIS_CHUNK];
#pragma unroll
    for (uint32_t a = 0; a < PCOA_AXIS_CHUNK; a++) v[a] = bv[a] = 0.0;
    for (uint32_t r = 0; r < dim; r++) {
        const double q = Q[size_t(r) * n + i], bq = BQ[size_t(r) * n + i];
#pragma unroll
        for (uint32_t a = 0; a < PCOA_AXIS_CHUNK; a++) {
            const double y = a0 + a < m ? Y[r + size_t(a0 + a) * dim] : 0.0;
            v[a] = fma(q, y, v[a]);
            bv[a] = fma(bq, y, bv[a]);
        }
    }
#pragma unroll
    for (uint32_t a = 0; a < PCOA_AXIS_CHUNK; a++)
        if (a0 + a < m) {
            V[size_t(i) * m + a0 + a] = v[a];
            R[size_t(a0 + a) * n + i] = bv[a] - theta[a0 + a] * v[a];
        }
}

// out[c] = sum of the squares of column c of W, a workgroup per column
__global__ __launch_bounds__(PCOA_THREADS) void pcoa_norm2_kernel(const double *__restrict__ W, uint32_t n,
                                                                  double *__restrict__ out) {
    __shared__ double scratch[17];
    const double *w = W + size_t(blockIdx.x) * n;
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += PCOA_THREADS) acc = fma(w[i], w[i], acc);
    acc = dvs_block_sum(acc, scratch);
    if (threadIdx.x == 0) out[blockIdx.x] = acc;
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

size_t up8(size_t x) { return (x + 7) & ~size_t(7); }

// the small blocks of a run, one allocation: offsets in bytes
struct PcoaLayout {
    size_t status, rowsum, w, h, g, y, theta, norm2, v, r, partial, bytes;
    PcoaLayout(uint32_t n, uint32_t limit, uint32_t m) {
        status = 0;                                    // uint32 [4]: the prepare pass's bits, the zero-division word
        rowsum = 16;                                   // double [n]
        w = rowsum + size_t(n) * 8;                    // double [n]: the candidate column
        h = w + size_t(n) * 8;                         // double [limit]: its coefficients against the basis
        g = h + size_t(limit) * 8;                     // double [dim x nb], dim entries from column to column: the new block column of T
        y = g + size_t(limit) * PCOA_BLOCK * 8;        // double [limit x m]: the leading eigenvectors of T
        theta = y + size_t(limit) * m * 8;             // double [m]
        norm2 = theta + size_t(m) * 8;                 // double [max(m, b)]
        v = norm2 + size_t(std::max(m, PCOA_BLOCK)) * 8;  // double [n x m] row-major: the Ritz vectors
        r = v + size_t(n) * m * 8;                     // double [n x m] column-major: their residual vectors
        partial = r + size_t(n) * m * 8;               // double [ceil(n / 32) x n]: the prepare pass's per-tile row sums
        bytes = up8(partial + size_t((n + PCOA_TILE - 1) / PCOA_TILE) * n * 8);
    }
};

uint32_t basis_limit(uint32_t n, uint32_t max_basis) {
    return std::min<uint32_t>(max_basis ? max_basis : PCOA_MAX_BASIS, n - 1);
}

}  // namespace

// the arguments and n, before anything else is looked at
static int pcoa_check_args(dvs_ctx *ctx, uint32_t n, const dvs_pcoa_params *p) {
    if (p->n_axes == 0) return dvs_set_error(ctx, DVS_ERR_VALUE, "principal coordinates: one axis at least");
    if (!(p->tol >= 0.0)) return dvs_set_error(ctx, DVS_ERR_VALUE, "tol must be a number >= 0");
    if (p->max_basis && p->max_basis < p->n_axes)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "a basis of %u columns cannot hold %u axes", p->max_basis, p->n_axes);
    if (p->n_axes > PCOA_MAX_AXES)
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "%u axes: %u at most (a full spectrum takes a dense solver)",
                             p->n_axes, PCOA_MAX_AXES);
    if (p->max_basis > PCOA_BASIS_CAP)
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "a basis of %u columns: %u at most", p->max_basis, PCOA_BASIS_CAP);
    if (n < 2) return dvs_set_error(ctx, DVS_ERR_VALUE, "need at least two rows for principal coordinates, not %u", n);
    if (p->n_axes > n - 1)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "%u axes of %u rows: between 1 and n - 1", p->n_axes, n);
    return DVS_OK;
}

// A consumer's run (dvs_internal.h dvs_square_consumer): the principal coordinates of the n x n matrix at d_dist (only
// read).  The prepare pass is enqueued on the context's stream behind whatever wrote the matrix.  Returns when the host
// outputs (dvs_pcoa's) are written.
static int pcoa_run(dvs_ctx *ctx, const double *d_dist, uint32_t n, const uint32_t *d_zerodiv, const dvs_pcoa_params *p,
                    double *values, double *vectors, double *residuals, double *row_means, dvs_pcoa_info *info) {
    const uint32_t m = p->n_axes, limit = basis_limit(n, p->max_basis);
    const PcoaLayout L(n, limit, m);
    PooledBuf basis{ctx}, scratch{ctx};
    int rc = dvs_dev_alloc(ctx, &basis.p, 2 * size_t(n) * limit * 8, "principal-coordinates basis");
    if (!rc) rc = dvs_dev_alloc(ctx, &scratch.p, L.bytes, "principal-coordinates scratch");
    if (rc) return rc;
    double *Q = basis.as<double>(), *BQ = Q + size_t(n) * limit;
    char *base = scratch.as<char>();
    auto f64 = [&](size_t off) { return reinterpret_cast<double *>(base + off); };
    uint32_t *d_status = reinterpret_cast<uint32_t *>(base + L.status);
    const char *what = "principal coordinates";
    const hipStream_t s = ctx->stream;
    const uint32_t row_grid = (n + PCOA_THREADS - 1) / PCOA_THREADS;

    // ---- the prepare pass
    uint32_t st[4] = {0, 0, 0, 0};
    std::vector<double> rowsum(n);
    hipError_t e = dvs_status_begin(ctx, d_status, 16, 1, d_zerodiv);
    if (e == hipSuccess) {
        const uint32_t tiles = (n + PCOA_TILE - 1) / PCOA_TILE;
        hipLaunchKernelGGL(pcoa_check_kernel, dim3(tiles, tiles), dim3(256), 0, s, d_dist, n, d_status, f64(L.partial));
        hipLaunchKernelGGL(pcoa_rowsum_kernel, dim3((n + 31) / 32), dim3(PCOA_THREADS), 0, s, f64(L.partial), n, tiles, f64(L.rowsum));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(st, d_status, 16, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(rowsum.data(), f64(L.rowsum), size_t(n) * 8, hipMemcpyDeviceToHost, s);
    hipError_t se = hipStreamSynchronize(s);
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, what);
    if (se != hipSuccess) return dvs_hip_fail(ctx, se, what);
    if (st[1]) return dvs_set_error(ctx, DVS_ERR_ZERODIV, "division by zero");  // 0 / 0, distance.py:283
    if (st[0] & PCOA_NONFINITE)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "Input contains NaN or infinity: the %u x %u distance matrix", n, n);
    if (st[0] & PCOA_ASYMMETRIC)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "the %u x %u distance matrix is not symmetric", n, n);
    long double total = 0.0L;
    for (uint32_t i = 0; i < n; i++) {
        row_means[i] = rowsum[i] / double(n);
        total += rowsum[i];
    }
    info->trace = double(total / (2.0L * n));

    // ---- the iteration (every helper enqueues on the stream and returns the launch's error)
    uint32_t dim = 0, hash_next = 0;
    double bq_scale = 0.0;  // the largest column norm of B Q so far
    bool failed = false;    // e != hipSuccess somewhere below
    auto ok = [&](hipError_t x) {
        if (x != hipSuccess && e == hipSuccess) e = x;
        failed = e != hipSuccess;
        return !failed;
    };
    auto sync = [&] { return ok(hipStreamSynchronize(s)); };
    // the candidate in w: twice against the basis, centred; -> its squared norm (waits for the stream)
    auto orthogonalise = [&](double *norm2) {
        for (int pass = 0; pass < 2 && dim; pass++) {
            hipLaunchKernelGGL(pcoa_dots_kernel, dim3(dim, 1), dim3(PCOA_THREADS), 0, s, Q, f64(L.w), n, f64(L.h), limit);
            hipLaunchKernelGGL(pcoa_project_out_kernel, dim3(row_grid), dim3(PCOA_THREADS), 0, s, Q, dim, n, f64(L.h), f64(L.w));
        }
        hipLaunchKernelGGL(pcoa_center_kernel, dim3(1), dim3(PCOA_THREADS), 0, s, f64(L.w), n);
        hipLaunchKernelGGL(pcoa_norm2_kernel, dim3(1), dim3(PCOA_THREADS), 0, s, f64(L.w), n, f64(L.norm2));
        if (!ok(hipGetLastError())) return false;
        if (!ok(hipMemcpyAsync(norm2, f64(L.norm2), 8, hipMemcpyDeviceToHost, s))) return false;
        return sync();
    };
    auto append = [&] {  // w / its norm is the basis's next column
        hipLaunchKernelGGL(pcoa_normalise_kernel, dim3(row_grid), dim3(PCOA_THREADS), 0, s, f64(L.w), n, f64(L.norm2),
                           Q + size_t(dim) * n);
        dim++;
        return ok(hipGetLastError());
    };
    // a hashed vector that survives the orthogonalisation becomes the next column; 64 in a row that do not: the basis
    // spans the complement of 1 as far as f64 can tell, and the block ends there
    auto append_hashed = [&] {
        for (int attempt = 0; attempt < 64; attempt++) {
            hipLaunchKernelGGL(pcoa_hash_kernel, dim3(row_grid), dim3(PCOA_THREADS), 0, s, f64(L.w), n, hash_next++);
            hipLaunchKernelGGL(pcoa_center_kernel, dim3(1), dim3(PCOA_THREADS), 0, s, f64(L.w), n);
            hipLaunchKernelGGL(pcoa_norm2_kernel, dim3(1), dim3(PCOA_THREADS), 0, s, f64(L.w), n, f64(L.norm2));
            double before = 0.0, after = 0.0;
            if (!ok(hipMemcpyAsync(&before, f64(L.norm2), 8, hipMemcpyDeviceToHost, s)) || !sync()) return false;
            if (!orthogonalise(&after)) return false;
            if (after > PCOA_HASH_TOL * PCOA_HASH_TOL * before && after > 0.0) return append();
        }
        return false;
    };

    for (uint32_t c = 0; c < PCOA_BLOCK && dim < limit && !failed; c++)
        if (!append_hashed()) break;
    std::vector<double> T(size_t(limit) * limit, 0.0), work, theta(limit), Z, g_host(size_t(limit) * PCOA_BLOCK);
    std::vector<double> y_host(size_t(limit) * m), res2(m), bq2(PCOA_BLOCK);
    uint32_t block0 = 0, steps = 0, converged = 0, since_solve = 0;
    uint64_t products = 0;
    bool have_ritz = false;
    // Rayleigh-Ritz over the basis as it stands: the leading m pairs of T, their vectors and true residuals (waits)
    auto solve = [&] {
        since_solve = 0;
        work.resize(size_t(dim) * dim);
        Z.resize(size_t(dim) * dim);
        for (uint32_t r = 0; r < dim; r++) std::copy_n(&T[size_t(r) * limit], dim, &work[size_t(r) * dim]);
        dvs_symeig_desc(int(dim), work.data(), theta.data(), Z.data());
        for (uint32_t a = 0; a < m; a++) std::copy_n(&Z[size_t(a) * dim], dim, &y_host[size_t(a) * dim]);
        if (!ok(hipMemcpyAsync(f64(L.y), y_host.data(), size_t(dim) * m * 8, hipMemcpyHostToDevice, s))) return false;
        if (!ok(hipMemcpyAsync(f64(L.theta), theta.data(), size_t(m) * 8, hipMemcpyHostToDevice, s))) return false;
        hipLaunchKernelGGL(pcoa_ritz_kernel, dim3(row_grid, (m + PCOA_AXIS_CHUNK - 1) / PCOA_AXIS_CHUNK), dim3(PCOA_THREADS), 0, s,
                           Q, BQ, n, dim, f64(L.y), f64(L.theta), m, f64(L.v), f64(L.r));
        hipLaunchKernelGGL(pcoa_norm2_kernel, dim3(m), dim3(PCOA_THREADS), 0, s, f64(L.r), n, f64(L.norm2));
        if (!ok(hipGetLastError())) return false;
        if (!ok(hipMemcpyAsync(res2.data(), f64(L.norm2), size_t(m) * 8, hipMemcpyDeviceToHost, s))) return false;
        if (!sync()) return false;  // (y_host and theta have been read)
        have_ritz = true;
        const double scale = p->tol * std::max(theta[0], 0.0);
        converged = 0;
        for (uint32_t a = 0; a < m; a++) converged += std::sqrt(res2[a]) <= scale;
        return true;
    };
    while (!failed && dim > block0) {
        const uint32_t nb = dim - block0;
        // 1. B Q_new, kept beside Q
        hipLaunchKernelGGL(pcoa_product_kernel, dim3((n + PCOA_WAVES * PCOA_ROWS - 1) / (PCOA_WAVES * PCOA_ROWS)),
                           dim3(PCOA_THREADS), 0, s, d_dist, n, Q + size_t(block0) * n, nb, BQ + size_t(block0) * n);
        hipLaunchKernelGGL(pcoa_center_kernel, dim3(nb), dim3(PCOA_THREADS), 0, s, BQ + size_t(block0) * n, n);
        // 2. the new block column of T = Q^T B Q, and the block's column norms
        hipLaunchKernelGGL(pcoa_dots_kernel, dim3(dim, nb), dim3(PCOA_THREADS), 0, s, Q, BQ + size_t(block0) * n, n, f64(L.g), dim);
        hipLaunchKernelGGL(pcoa_norm2_kernel, dim3(nb), dim3(PCOA_THREADS), 0, s, BQ + size_t(block0) * n, n, f64(L.norm2));
        if (!ok(hipGetLastError())) break;
        if (!ok(hipMemcpyAsync(g_host.data(), f64(L.g), size_t(dim) * nb * 8, hipMemcpyDeviceToHost, s))) break;
        if (!ok(hipMemcpyAsync(bq2.data(), f64(L.norm2), size_t(nb) * 8, hipMemcpyDeviceToHost, s))) break;
        if (!sync()) break;
        steps++;
        products += nb;
        for (uint32_t c = 0; c < nb; c++) {
            bq_scale = std::max(bq_scale, std::sqrt(bq2[c]));
            for (uint32_t r = 0; r < dim; r++) T[size_t(r) * limit + block0 + c] = g_host[r + size_t(c) * dim];
        }
        // symmetrised: the diagonal block averaged, the rest mirrored
        for (uint32_t c = block0; c < dim; c++)
            for (uint32_t r = 0; r < c; r++) {
                double t = T[size_t(r) * limit + c];
                if (r >= block0) t = 0.5 * (t + T[size_t(c) * limit + r]);
                T[size_t(r) * limit + c] = T[size_t(c) * limit + r] = t;
            }
        // 3. Rayleigh-Ritz, every step or every fourth
        const bool last = dim >= limit;
        since_solve++;
        if (dim >= m && (last || dim <= PCOA_SOLVE_EVERY_STEP || since_solve >= 4)) {
            if (!solve()) break;
            if (converged == m) break;
        }
        if (last) break;
        // 4. the next block: the columns of B Q_new against the whole basis
        const uint32_t from = block0;
        block0 = dim;
        for (uint32_t c = 0; c < nb && dim < limit && !failed; c++) {
            if (!ok(hipMemcpyAsync(f64(L.w), BQ + size_t(from + c) * n, size_t(n) * 8, hipMemcpyDeviceToDevice, s))) break;
            double after = 0.0;
            if (!orthogonalise(&after)) break;
            if (std::sqrt(after) > PCOA_RANK_TOL * bq_scale) {
                if (!append()) break;
            } else if (!append_hashed()) {
                break;  // (no hashed vector survives: the basis spans the complement of 1)
            }
        }
    }
    if (!failed && since_solve && dim >= m) solve();  // (the basis ended between two scheduled solves)
    std::vector<double> v_host(size_t(n) * m);
    if (!failed && have_ritz) ok(hipMemcpyAsync(v_host.data(), f64(L.v), size_t(n) * m * 8, hipMemcpyDeviceToHost, s));
    se = hipStreamSynchronize(s);
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, what);
    if (se != hipSuccess) return dvs_hip_fail(ctx, se, what);
    if (!have_ritz)
        return dvs_set_error(ctx, DVS_ERR_RUNTIME, "principal coordinates: the basis stopped at %u columns, short of %u axes",
                             dim, m);
    // the sign rule: the component of largest magnitude (the lowest index on a tie) is positive
    for (uint32_t a = 0; a < m; a++) {
        values[a] = theta[a];
        residuals[a] = std::sqrt(res2[a]);
        uint32_t top = 0;
        for (uint32_t i = 1; i < n; i++)
            if (std::fabs(v_host[size_t(i) * m + a]) > std::fabs(v_host[size_t(top) * m + a])) top = i;
        const bool flip = v_host[size_t(top) * m + a] < 0.0;
        for (uint32_t i = 0; i < n; i++) vectors[size_t(i) * m + a] = flip ? -v_host[size_t(i) * m + a] : v_host[size_t(i) * m + a];
    }
    info->converged = converged;
    info->basis = dim;
    info->steps = steps;
    info->products = products;
    return DVS_OK;
}

// beside the matrix: the basis with B Q beside it, and the small blocks
dvs_square_consumer dvs_pcoa_consumer(dvs_ctx *ctx, uint32_t n, const dvs_pcoa_params *p, double *values, double *vectors,
                                      double *residuals, double *row_means, dvs_pcoa_info *info) {
    dvs_square_consumer c{"dvs_pcoa"};
    const uint32_t limit = basis_limit(n, p->max_basis);
    c.check = [=] { return pcoa_check_args(ctx, n, p); };
    c.extra_bytes = [=] { return 2 * size_t(n) * limit * 8 + PcoaLayout(n, limit, p->n_axes).bytes; };
    snprintf(c.extra_what, sizeof c.extra_what, "a basis of %u columns", limit);
    c.writes_matrix = false;
    c.run = [=](double *d_dist, const uint32_t *d_zerodiv) {
        return pcoa_run(ctx, d_dist, n, d_zerodiv, p, values, vectors, residuals, row_means, info);
    };
    return c;
}

// the coordinates of every query in a fitted ordination (include/dvs_hip.h "principal coordinates") into the host array
// coords (m x n_axes): the fit's tables uploaded once, pcoa_project_kernel behind each strip's distances
int dvs_pcoa_project_strips(dvs_ctx *ctx, const dvs_cross_stage &st, uint32_t n_axes, const double *values,
                            const double *vectors, const double *row_means, double *coords) {
    if (n_axes == 0) return dvs_set_error(ctx, DVS_ERR_VALUE, "principal coordinates: one axis at least");
    if (n_axes > DVS_TOPK_MAX)
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "%u axes: %u at most", n_axes, DVS_TOPK_MAX);
    if (!values || !vectors || !row_means) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (st.n == 0) return dvs_set_error(ctx, DVS_ERR_VALUE, "a projection needs the fitted rows: no reference rows");
    if (st.m == 0) return DVS_OK;
    if (!coords) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    const size_t nv = size_t(st.n) * n_axes;
    std::vector<double> scale(n_axes);
    for (uint32_t a = 0; a < n_axes; a++) scale[a] = values[a] > 0.0 ? -0.5 / std::sqrt(values[a]) : 0.0;
    PooledBuf d_fit{ctx}, d_out{ctx};  // d_fit: V [n x n_axes], mu [n], scale [n_axes]
    double *d_v, *d_mu, *d_scale;
    dvs_strip_consumer c{};
    c.begin = [&](uint32_t rows) {
        int rc = dvs_dev_alloc(ctx, &d_fit.p, (nv + st.n + n_axes) * 8, "fitted ordination");
        if (!rc) rc = dvs_dev_alloc(ctx, &d_out.p, size_t(rows) * n_axes * 8, "projected coordinates");
        if (rc) return rc;
        d_v = d_fit.as<double>(), d_mu = d_v + nv, d_scale = d_mu + st.n;
        hipError_t e = hipMemcpyAsync(d_v, vectors, nv * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_mu, row_means, size_t(st.n) * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_scale, scale.data(), size_t(n_axes) * 8, hipMemcpyHostToDevice, ctx->stream);
        return e == hipSuccess ? DVS_OK : dvs_hip_fail(ctx, e, "fitted ordination upload");
    };
    c.strip = [&](uint32_t q0, uint32_t mq, double *d_strip) {
        hipLaunchKernelGGL(pcoa_project_kernel, dim3(mq, (n_axes + PROJ_AXES - 1) / PROJ_AXES), dim3(PROJ_THREADS), 0, ctx->stream,
                           d_strip, st.n, n_axes, d_v, d_mu, d_scale, d_out.as<double>());
        hipError_t le = hipGetLastError();
        if (le == hipSuccess)
            le = hipMemcpyAsync(coords + size_t(q0) * n_axes, d_out.p, size_t(mq) * n_axes * 8, hipMemcpyDeviceToHost, ctx->stream);
        return le;
    };
    return dvs_strip_run(ctx, st, c);
}
