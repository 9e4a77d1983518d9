// PERMANOVA (Anderson 2001) over an n x n distance matrix on the device: include/dvs_hip.h "PERMANOVA" pins the
// statistic and the order of every sum, DESIGN.md 4.19 has the measurements.  No counterpart in the reference.
//
// The matrix is only READ, and only above the diagonal.  Device pipeline (one stream; every seam is a launch boundary --
// no grid barrier, no spinning):
//   entry    pv_entry_kernel, a wave per row i: flags a non-finite or negative D[i][j], j > i, and leaves T_i = sum_{j>i}
//            q_ij and, for the observed labels, R_i = sum_{j>i, g_j = g_i} q_ij; the host adds T into SS_T and R into the
//            groups' own terms in item order
//   batch    per batch of up to B label vectors (the observed one first, then the permutations in their order):
//            pv_score_kernel<L, B>, the hot kernel, ONE pass over the upper triangle for all B vectors, and
//            pv_final_kernel, which adds the tiles' partial sums
// pv_score_kernel: a workgroup takes a tile of PV_ROWS rows x PV_COLS columns, a lane ONE column j of it.  The lane
// keeps the B labels of its column in registers, the tile's rows' labels sit in LDS as [row][B] (a row's B labels are
// contiguous: one broadcast read a row, no bank conflict) and go through the scalar unit; the rows' cells are loaded 8
// rows ahead.  Accumulator b of the lane is C_j^b = sum_{i<j, i in the tile, g_i^b = g_j^b} q_ij: a cell that does not
// match, or lies on or below the diagonal (never loaded), adds +0.0 at its place.  Then w[g_j^b] C_j^b, the 64 lanes
// by the xor-shuffle tree, the 4 waves in wave order, and the tile's B sums stored; pv_final_kernel adds a vector's
// tiles, a thread its strided tiles in ascending order, the lanes by the tree, the waves in wave order.  Every order
// is fixed by (n, position): the labels only decide between q and +0.0 and pick w by the group's SIZE.
#include "dvs_internal.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

namespace {

constexpr int PV_THREADS = 256;
constexpr uint32_t PV_WAVES = PV_THREADS / 64;
constexpr uint32_t PV_COLS = PV_THREADS;  // columns of a tile: one per thread
constexpr uint32_t PV_ROWS = 128;         // rows of a tile
constexpr uint32_t PV_UNROLL = 8;         // rows of a tile a lane has in flight
constexpr uint32_t PV_BATCH = 16;         // label vectors a pass serves (DESIGN.md 4.19 has the other lengths' times)
constexpr uint32_t PV_MAX_BATCH = 32;     // the widest instantiation
constexpr uint32_t PV_MAX_GROUPS = 65535;
constexpr size_t PV_LABEL_BYTES = size_t(16) << 20;  // the narrowed labels of the batches uploaded at once, at most
enum { PV_ST_BAD = 0, PV_ST_ZERODIV = 1 };
constexpr uint32_t PV_BAD_NONFINITE = 1, PV_BAD_NEGATIVE = 2;
static_assert(PV_ROWS % PV_UNROLL == 0, "a tile's rows go in whole groups");

// the entry check and the observed labels' row sums: a wave per row x (PV_WAVES rows a workgroup), the cells right of
// the diagonal in chunks of 64 from the 64-aligned column at or below x + 1
__global__ __launch_bounds__(PV_THREADS) void pv_entry_kernel(const double *__restrict__ D, uint32_t n,
                                                              const uint32_t *__restrict__ lab, double *__restrict__ T,
                                                              double *__restrict__ R, uint32_t *status) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t x = blockIdx.x * PV_WAVES + wave;
    if (x >= n) return;
    const uint32_t gx = lab[x];
    const double *row = D + size_t(x) * n;
    double t = 0.0, r = 0.0;
    uint32_t bad = 0;
    for (uint32_t j0 = (x + 1) & ~63u; j0 < n; j0 += 64 * PV_UNROLL) {
        double dv[PV_UNROLL];
        uint32_t gv[PV_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < PV_UNROLL; u++) {
            const uint32_t j = j0 + u * 64 + lane;
            const bool valid = j > x && j < n;
            dv[u] = valid ? row[j] : 0.0;
            gv[u] = valid ? lab[j] : ~gx;
        }
#pragma unroll
        for (uint32_t u = 0; u < PV_UNROLL; u++) {
            const double d = dv[u];
            if (!__builtin_isfinite(d)) bad |= PV_BAD_NONFINITE;
            if (d < 0.0) bad |= PV_BAD_NEGATIVE;
            const double q = d * d;
            t += q;
            r += gv[u] == gx ? q : 0.0;
        }
    }
    if (bad) atomicOr(&status[PV_ST_BAD], bad);
    t = dvs_wave_sum(t);
    r = dvs_wave_sum(r);
    if (lane == 0) {
        T[x] = t;
        R[x] = r;
    }
}

template <typename L>
__device__ __forceinline__ uint32_t pv_label_of(const uint32_t *words, int b) {
    if (sizeof(L) == 1) return (words[b >> 2] >> ((b & 3) * 8)) & 0xFFu;
    return (words[b >> 1] >> ((b & 1) * 16)) & 0xFFFFu;
}

// One pass over the upper triangle for B label vectors (the file's head has the order).  lab: [n][B], item j's B labels
// contiguous; w: [n_groups] 1 / the group's size; part: [tiles][B], tile (rb, cb) at rb * gridDim.x + cb.
template <typename L, int B>
__global__ __launch_bounds__(PV_THREADS) void pv_score_kernel(const double *__restrict__ D, uint32_t n,
                                                              const L *__restrict__ lab, const double *__restrict__ w,
                                                              double *__restrict__ part) {
    constexpr int WORDS = B * int(sizeof(L)) / 4;  // of a row's labels
    __shared__ __attribute__((aligned(16))) uint32_t s_row[PV_ROWS * WORDS];
    __shared__ double s_sum[PV_WAVES][B];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t c0 = blockIdx.x * PV_COLS, r0 = blockIdx.y * PV_ROWS;
    const uint32_t r1 = min(r0 + PV_ROWS, n), c1 = min(c0 + PV_COLS, n);
    double *out = part + (size_t(blockIdx.y) * gridDim.x + blockIdx.x) * B;
    if (r0 + 1 >= c1) {  // no cell of the tile lies above the diagonal (the whole workgroup)
        if (tid < uint32_t(B)) out[tid] = 0.0;
        return;
    }
    {  // the labels of the tile's rows: lab[r0 * B .. r1 * B) as it stands, zeros behind the last row
        const uint32_t *src = reinterpret_cast<const uint32_t *>(lab + size_t(r0) * B);
        const uint32_t have = (r1 - r0) * WORDS;
        for (uint32_t k = tid; k < PV_ROWS * WORDS; k += PV_THREADS) s_row[k] = k < have ? src[k] : 0u;
    }
    const uint32_t j = c0 + wave * 64 + lane;
    const bool col = j < n;
    uint32_t cw[WORDS], cl[B];  // the column's labels: loaded as words, kept one to a register
#pragma unroll
    for (int k = 0; k < WORDS; k++) cw[k] = 0u;
    if (col) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(lab + size_t(j) * B);
#pragma unroll
        for (int k = 0; k < WORDS; k++) cw[k] = src[k];
    }
#pragma unroll
    for (int b = 0; b < B; b++) cl[b] = pv_label_of<L>(cw, b);
    __syncthreads();
    double acc[B];
#pragma unroll
    for (int b = 0; b < B; b++) acc[b] = 0.0;
    // the wave's rows: those above its last column (none for a wave behind the matrix's last column)
    const uint32_t rend = c0 + wave * 64 < n ? min(r1, min(c0 + wave * 64 + 63, n - 1)) : r0;
    for (uint32_t i0 = r0; i0 < rend; i0 += PV_UNROLL) {
        double dv[PV_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < PV_UNROLL; u++) {
            const uint32_t i = i0 + u;
            dv[u] = i < rend && i < j && col ? D[size_t(i) * n + j] : 0.0;
        }
#pragma unroll
        for (uint32_t u = 0; u < PV_UNROLL; u++) {
            const double q = dv[u] * dv[u];
            uint32_t rw[WORDS];  // the row's labels: the same in every lane, through the scalar unit
#pragma unroll
            for (int k = 0; k < WORDS; k++) rw[k] = __builtin_amdgcn_readfirstlane(s_row[(i0 + u - r0) * WORDS + k]);
#pragma unroll
            // (q * 1.0 + acc, rounded once, is q + acc; q * 0.0 + acc is acc: one select of a half word, not two)
            for (int b = 0; b < B; b++) acc[b] = __builtin_fma(q, pv_label_of<L>(rw, b) == cl[b] ? 1.0 : 0.0, acc[b]);
        }
    }
    // w[g_j] C_j, then the B trees of dvs_wave_sum level by level: B independent shuffles in flight, not a chain of 6 B
#pragma unroll
    for (int b = 0; b < B; b++) acc[b] *= w[cl[b]];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int b = 0; b < B; b++) acc[b] += __shfl_xor(acc[b], o, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int b = 0; b < B; b++) s_sum[wave][b] = acc[b];
    }
    __syncthreads();
    if (tid < uint32_t(B)) {
        double v = s_sum[0][tid];
        for (uint32_t k = 1; k < PV_WAVES; k++) v += s_sum[k][tid];
        out[tid] = v;
    }
}

// Behind a scoring pass, workgroup b: the n_tiles partial sums of the batch's vector b (part: [tiles][stride]) added
// into out[b] -- a thread its strided tiles in ascending order, the lanes by the tree, the waves in wave order
__global__ __launch_bounds__(PV_THREADS) void pv_final_kernel(const double *__restrict__ part, uint32_t n_tiles, uint32_t stride,
                                                              double *__restrict__ out) {
    __shared__ double s_w[PV_WAVES];
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    double acc = 0.0;
    for (uint32_t t = tid; t < n_tiles; t += PV_THREADS) acc += part[size_t(t) * stride + b];
    acc = dvs_wave_sum(acc);
    if ((tid & 63) == 0) s_w[tid >> 6] = acc;
    __syncthreads();
    if (tid != 0) return;
    for (uint32_t k = 1; k < PV_WAVES; k++) acc += s_w[k];
    out[b] = acc;
}

size_t up16(size_t x) { return (x + 15) & ~size_t(15); }
uint32_t grid_of(uint32_t n, uint32_t per) { return (n + per - 1) / per; }

// what a run enqueues a pass with: the vectors a pass serves, the instantiation that holds them, the label width
struct PvShape {
    uint32_t batch, cap, lbytes, n_cb, n_rb, n_batches, per_upload;
    PvShape(const dvs_ctx *ctx, uint32_t n, uint32_t n_groups, uint32_t n_perm) {
        const uint32_t knob = ctx->knobs.permanova_batch;
        batch = knob ? std::min(knob, PV_MAX_BATCH) : PV_BATCH;
        cap = batch <= 8 ? 8 : batch <= 16 ? 16 : 32;
        lbytes = n_groups <= 256 ? 1 : 2;
        n_cb = grid_of(n, PV_COLS);
        n_rb = grid_of(n, PV_ROWS);
        n_batches = uint32_t((uint64_t(n_perm) + 1 + batch - 1) / batch);
        const size_t one = size_t(n) * cap * lbytes;
        per_upload = uint32_t(std::min<size_t>(std::max<size_t>(PV_LABEL_BYTES / one, 1), n_batches));
    }
    size_t batch_label_bytes(uint32_t n) const { return size_t(n) * cap * lbytes; }
};

// the state of a run, one allocation: offsets in bytes
struct PvLayout {
    size_t status, T, R, w, ssw, part, lab, labels, bytes;
    PvLayout(uint32_t n, uint32_t n_groups, uint32_t n_perm, const PvShape &sh) {
        status = 0;                                                   // uint32 [8]
        T = 32;                                                       // double [n]
        R = T + size_t(n) * 8;                                        // double [n]
        w = R + size_t(n) * 8;                                        // double [n_groups]
        ssw = w + size_t(n_groups) * 8;                               // double [n_perm + 1]
        part = ssw + (size_t(n_perm) + 1) * 8;                        // double [tiles][cap]
        lab = part + size_t(sh.n_cb) * sh.n_rb * sh.cap * 8;          // uint32 [n]: the observed labels
        labels = up16(lab + size_t(n) * 4);                           // L [per_upload][n][cap]
        bytes = up16(labels + sh.batch_label_bytes(n) * sh.per_upload);
    }
};

template <typename L>
void pv_launch_score(uint32_t cap, dim3 grid, hipStream_t s, const double *D, uint32_t n, const void *lab, const double *w,
                     double *part) {
    const L *l = static_cast<const L *>(lab);
    if (cap == 8) hipLaunchKernelGGL((pv_score_kernel<L, 8>), grid, dim3(PV_THREADS), 0, s, D, n, l, w, part);
    else if (cap == 16) hipLaunchKernelGGL((pv_score_kernel<L, 16>), grid, dim3(PV_THREADS), 0, s, D, n, l, w, part);
    else hipLaunchKernelGGL((pv_score_kernel<L, 32>), grid, dim3(PV_THREADS), 0, s, D, n, l, w, part);
}

}  // namespace

// the arguments and n, before anything else is looked at; counts: the observed group sizes (filled here)
static int permanova_check_args(dvs_ctx *ctx, uint32_t n, const dvs_permanova_args &a, std::vector<uint32_t> *counts) {
    if (!a.labels || !a.ss_total || !a.ss_within || (a.n_perm != 0) != (a.perm_labels != nullptr))
        return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_permanova: null argument (perm_labels is NULL exactly when n_perm is 0)");
    if (n < 3) return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_permanova: %u rows: three at least", n);
    if (a.n_groups < 2 || a.n_groups >= n)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_permanova: %u groups of %u rows: between 2 and %u", a.n_groups, n, n - 1);
    if (a.n_groups > PV_MAX_GROUPS)
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "dvs_permanova: %u groups: %u at most (a label travels in 16 bits)",
                             a.n_groups, PV_MAX_GROUPS);
    counts->assign(a.n_groups, 0);
    for (uint32_t i = 0; i < n; i++) {
        if (a.labels[i] >= a.n_groups)
            return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_permanova: row %u has label %u of %u groups", i, a.labels[i], a.n_groups);
        (*counts)[a.labels[i]]++;
    }
    for (uint32_t g = 0; g < a.n_groups; g++)
        if (!(*counts)[g]) return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_permanova: group %u is empty", g);
    std::vector<uint32_t> c(a.n_groups);
    for (uint32_t p = 0; p < a.n_perm; p++) {
        const uint32_t *row = a.perm_labels + size_t(p) * n;
        std::fill(c.begin(), c.end(), 0u);
        for (uint32_t i = 0; i < n; i++) {
            if (row[i] >= a.n_groups)
                return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_permanova: permutation %u: row %u has label %u of %u groups", p, i,
                                     row[i], a.n_groups);
            c[row[i]]++;
        }
        if (c != *counts)
            return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_permanova: permutation %u changes the sizes of the groups", p);
    }
    return DVS_OK;
}

// the labels of vectors [v0, v0 + count) (vector 0: the observed ones, v >= 1: permutation v - 1) narrowed into dst as
// [n][cap], the slots behind `count` zero: an item's cap labels are written together, from `count` rows read side by side
template <typename L>
static void permanova_narrow(const dvs_permanova_args &a, uint32_t n, uint32_t cap, uint64_t v0, uint32_t count, L *dst) {
    const uint32_t *src[PV_MAX_BATCH];
    for (uint32_t b = 0; b < count; b++) src[b] = v0 + b == 0 ? a.labels : a.perm_labels + size_t(v0 + b - 1) * n;
    for (uint32_t j = 0; j < n; j++) {
        L *d = dst + size_t(j) * cap;
        for (uint32_t b = 0; b < count; b++) d[b] = L(src[b][j]);
        for (uint32_t b = count; b < cap; b++) d[b] = L(0);
    }
}

// A consumer's run (dvs_internal.h dvs_square_consumer): PERMANOVA over the n x n matrix at d_dist (only read), enqueued
// on the context's stream behind whatever wrote the matrix.  Returns when the host outputs (dvs_permanova's) are written.
static int permanova_run(dvs_ctx *ctx, const double *d_dist, uint32_t n, const uint32_t *d_zerodiv, const dvs_permanova_args &a,
                         const std::vector<uint32_t> &counts) {
    const uint32_t ng = a.n_groups, np = a.n_perm;
    const PvShape sh(ctx, n, ng, np);
    const PvLayout L(n, ng, np, sh);
    PooledBuf d_state{ctx};
    if (int rc = dvs_dev_alloc(ctx, &d_state.p, L.bytes, "PERMANOVA state")) return rc;
    char *base = d_state.as<char>();
    auto f64 = [&](size_t off) { return reinterpret_cast<double *>(base + off); };
    uint32_t *d_status = reinterpret_cast<uint32_t *>(base + L.status), *d_lab = reinterpret_cast<uint32_t *>(base + L.lab);
    double *d_T = f64(L.T), *d_R = f64(L.R), *d_w = f64(L.w), *d_ssw = f64(L.ssw), *d_part = f64(L.part);
    const char *what = "PERMANOVA";
    const hipStream_t s = ctx->stream;

    // ---- the entry check with the observed labels' row sums
    std::vector<double> wv(ng), T(n), R(n);
    for (uint32_t g = 0; g < ng; g++) wv[g] = 1.0 / double(counts[g]);
    uint32_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    hipError_t e = dvs_status_begin(ctx, d_status, 32, PV_ST_ZERODIV, d_zerodiv);
    if (e == hipSuccess) e = hipMemcpyAsync(d_lab, a.labels, size_t(n) * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_w, wv.data(), size_t(ng) * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pv_entry_kernel, dim3(grid_of(n, PV_WAVES)), dim3(PV_THREADS), 0, s, d_dist, n, d_lab, d_T, d_R, d_status);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(st, d_status, 32, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(T.data(), d_T, size_t(n) * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(R.data(), d_R, size_t(n) * 8, hipMemcpyDeviceToHost, s);
    hipError_t se = hipStreamSynchronize(s);
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, what);
    if (se != hipSuccess) return dvs_hip_fail(ctx, se, what);
    if (st[PV_ST_ZERODIV]) return dvs_set_error(ctx, DVS_ERR_ZERODIV, "division by zero");  // 0 / 0, distance.py:283
    if (st[PV_ST_BAD] & PV_BAD_NONFINITE)
        return dvs_set_error(ctx, DVS_ERR_VALUE,
                             "Input contains NaN or infinity: the %u x %u distance matrix above its diagonal (dvs_permanova)", n, n);
    if (st[PV_ST_BAD] & PV_BAD_NEGATIVE)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_permanova: the %u x %u distance matrix has a negative entry above its diagonal",
                             n, n);

    // ---- the batches: each one's labels narrowed into its own part of the context's pinned staging block and uploaded
    // from there, then its pass and its sums -- the device works on a batch while the host narrows the next.  After
    // per_upload batches the stream is waited for, and the staging block and its image on the device are written again
    // (every copy out of the block has been waited for when the call returns: no event is left behind).
    if (int rc = dvs_pinned_stage(ctx, sh.batch_label_bytes(n) * sh.per_upload, "pinned staging block of the label vectors")) return rc;
    unsigned char *stage = static_cast<unsigned char *>(ctx->h_pack);
    const dim3 grid(sh.n_cb, sh.n_rb);
    const uint64_t n_vec = uint64_t(np) + 1;
    for (uint32_t k0 = 0; k0 < sh.n_batches && e == hipSuccess && se == hipSuccess; k0 += sh.per_upload) {
        const uint32_t k1 = std::min(k0 + sh.per_upload, sh.n_batches);
        for (uint32_t k = k0; k < k1 && e == hipSuccess; k++) {
            const uint64_t v0 = uint64_t(k) * sh.batch;
            const uint32_t count = uint32_t(std::min<uint64_t>(sh.batch, n_vec - v0));
            const size_t at = sh.batch_label_bytes(n) * (k - k0);
            unsigned char *dst = stage + at;
            if (sh.lbytes == 1) permanova_narrow(a, n, sh.cap, v0, count, dst);
            else permanova_narrow(a, n, sh.cap, v0, count, reinterpret_cast<uint16_t *>(dst));
            const void *d_l = base + L.labels + at;
            e = hipMemcpyAsync(base + L.labels + at, dst, sh.batch_label_bytes(n), hipMemcpyHostToDevice, s);
            if (e != hipSuccess) break;
            if (sh.lbytes == 1) pv_launch_score<uint8_t>(sh.cap, grid, s, d_dist, n, d_l, d_w, d_part);
            else pv_launch_score<uint16_t>(sh.cap, grid, s, d_dist, n, d_l, d_w, d_part);
            hipLaunchKernelGGL(pv_final_kernel, dim3(count), dim3(PV_THREADS), 0, s, d_part, sh.n_cb * sh.n_rb, sh.cap, d_ssw + v0);
            e = hipGetLastError();
        }
        if (e == hipSuccess && k1 == sh.n_batches) e = hipMemcpyAsync(a.ss_within, d_ssw, size_t(n_vec) * 8, hipMemcpyDeviceToHost, s);
        se = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, what);
    if (se != hipSuccess) return dvs_hip_fail(ctx, se, what);

    // ---- SS_T and the groups' own terms from the rows' sums, in item order
    double total = 0.0;
    for (uint32_t i = 0; i < n; i++) total += T[i];
    *a.ss_total = total / double(n);
    if (a.group_ss) {
        std::fill(a.group_ss, a.group_ss + ng, 0.0);
        for (uint32_t i = 0; i < n; i++) a.group_ss[a.labels[i]] += R[i];
        for (uint32_t g = 0; g < ng; g++) a.group_ss[g] *= wv[g];
    }
    if (a.info) {
        uint32_t n_le = 0;
        for (uint32_t p = 1; p <= np; p++) n_le += a.ss_within[p] <= a.ss_within[0];
        *a.info = dvs_permanova_info{n_le, 1 + sh.n_batches, sh.batch};
    }
    return DVS_OK;
}

// beside the matrix: the state
dvs_square_consumer dvs_permanova_consumer(dvs_ctx *ctx, uint32_t n, const dvs_permanova_args &a) {
    dvs_square_consumer c{"dvs_permanova"};
    auto counts = std::make_shared<std::vector<uint32_t>>();
    c.check = [=] { return permanova_check_args(ctx, n, a, counts.get()); };
    c.extra_bytes = [=] { return PvLayout(n, a.n_groups, a.n_perm, PvShape(ctx, n, a.n_groups, a.n_perm)).bytes; };
    snprintf(c.extra_what, sizeof c.extra_what, "the sums of %u permutations", a.n_perm);
    c.writes_matrix = false;
    c.run = [=](double *d_dist, const uint32_t *d_zerodiv) { return permanova_run(ctx, d_dist, n, d_zerodiv, a, *counts); };
    return c;
}
