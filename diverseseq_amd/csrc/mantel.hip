// The Mantel test over two n x n distance matrices on the device: include/dvs_hip.h "Mantel" pins the statistic and the
// order of every sum, DESIGN.md 4.20 has the measurements.  No counterpart in the reference.
//
// X is only READ, and only above the diagonal.  Y is worked on in a block the library owns (a caller's device matrix is
// copied first): the centre pass writes v = y - s_y into both triangles, so that the scoring kernel reads v(a, b) at
// [a][b] whichever of a, b is the smaller.  Device pipeline (one stream; every seam is a launch boundary -- no grid
// barrier, no spinning):
//   entry    mt_entry_kernel over each matrix, a wave per row i: flags a non-finite or negative cell right of the
//            diagonal and leaves the row's sum; the host adds the rows in item order into S and forms the shift
//   centre   mt_centre_kernel<Y>, a wave per row i: the row's sums of u and u * u (of v and v * v); for Y, v written to
//            [i][j] and [j][i].  X is not written: u is formed again on load by the scoring kernel
//   batch    per batch of up to B permutations (the identity first, then the caller's in their order):
//            mt_score_kernel, the hot kernel, a workgroup per (row i of X, permutation b), and mt_final_kernel,
//            which adds a permutation's n partial sums
// mt_score_kernel: thread t of the 256 takes the columns j = 256 floor((i + 1) / 256) + t, + 256, ... right of the
// diagonal in ascending order: u_ij from X's row i (coalesced), pi[j] from the permutation (coalesced), and
// v(pi[i], pi[j]) gathered from row pi[i] of the centred Y in global memory (streaming the row into LDS first and
// gathering there was 1.15 times faster at n = 10 000, less than a second path is worth: DESIGN.md 4.20).  The B jobs
// of a row are neighbours in the grid, so that X's row comes from HBM once per batch.
#include "dvs_internal.h"

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

namespace {

constexpr int MT_THREADS = 256;
constexpr uint32_t MT_WAVES = MT_THREADS / 64;
constexpr uint32_t MT_UNROLL = 4;      // cells a lane has in flight
constexpr uint32_t MT_BATCH = 32;      // permutations a pass serves (DESIGN.md 4.20 has the other lengths' times)
constexpr uint32_t MT_MAX_BATCH = 32;
constexpr size_t MT_PERM_BYTES = size_t(16) << 20;  // the permutations of the batches uploaded at once, at most
enum { MT_ST_BAD_X = 0, MT_ST_BAD_Y = 1, MT_ST_ZERODIV_X = 2, MT_ST_ZERODIV_Y = 3 };
constexpr uint32_t MT_BAD_NONFINITE = 1, MT_BAD_NEGATIVE = 2;

// the entry check and the rows' sums: a wave per row x (MT_WAVES rows a workgroup), the cells right of the diagonal in
// chunks of 64 from the 64-aligned column at or below x + 1
__global__ __launch_bounds__(MT_THREADS) void mt_entry_kernel(const double *__restrict__ D, uint32_t n, double *__restrict__ R,
                                                              uint32_t *bad_word) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t x = blockIdx.x * MT_WAVES + wave;
    if (x >= n) return;
    const double *row = D + size_t(x) * n;
    double t = 0.0;
    uint32_t bad = 0;
    for (uint32_t j0 = (x + 1) & ~63u; j0 < n; j0 += 64 * MT_UNROLL) {
        double dv[MT_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < MT_UNROLL; u++) {
            const uint32_t j = j0 + u * 64 + lane;
            dv[u] = j > x && j < n ? row[j] : 0.0;
        }
#pragma unroll
        for (uint32_t u = 0; u < MT_UNROLL; u++) {
            const double d = dv[u];
            if (!__builtin_isfinite(d)) bad |= MT_BAD_NONFINITE;
            if (d < 0.0) bad |= MT_BAD_NEGATIVE;
            t += d;
        }
    }
    if (bad) atomicOr(bad_word, bad);
    t = dvs_wave_sum(t);
    if (lane == 0) R[x] = t;
}

// the centred cells' sums, rows and chains as above: c = D[x][j] - shift, U[x] = sum c, UU[x] = sum c * c; Y: c is
// written over the cell and over its mirror below the diagonal (a thread reads only the cell it then writes)
template <bool Y>
__global__ __launch_bounds__(MT_THREADS) void mt_centre_kernel(std::conditional_t<Y, double, const double> *__restrict__ D,
                                                               uint32_t n, double shift, double *__restrict__ U,
                                                               double *__restrict__ UU) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t x = blockIdx.x * MT_WAVES + wave;
    if (x >= n) return;
    auto *row = D + size_t(x) * n;
    double t = 0.0, q = 0.0;
    for (uint32_t j0 = (x + 1) & ~63u; j0 < n; j0 += 64 * MT_UNROLL) {
        double dv[MT_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < MT_UNROLL; u++) {
            const uint32_t j = j0 + u * 64 + lane;
            dv[u] = j > x && j < n ? row[j] : shift;
        }
#pragma unroll
        for (uint32_t u = 0; u < MT_UNROLL; u++) {
            const uint32_t j = j0 + u * 64 + lane;
            const bool valid = j > x && j < n;
            const double c = valid ? dv[u] - shift : 0.0;
            t += c;
            q += c * c;
            if constexpr (Y) {
                if (valid) {
                    row[j] = c;
                    D[size_t(j) * n + x] = c;
                }
            }
        }
    }
    t = dvs_wave_sum(t);
    q = dvs_wave_sum(q);
    if (lane == 0) {
        U[x] = t;
        UU[x] = q;
    }
}

// One job a workgroup (the file's head has the order): job = i * count + b, row i of X against permutation b of the
// batch.  perms: [count][n]; zpart: [count][n], job (i, b) at b * n + i.
__global__ __launch_bounds__(MT_THREADS) void mt_score_kernel(const double *__restrict__ X, const double *__restrict__ Yc,
                                                              uint32_t n, double s_x, const uint32_t *__restrict__ perms,
                                                              uint32_t count, double *__restrict__ zpart) {
    __shared__ double s_w[MT_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t i = blockIdx.x / count, b = blockIdx.x - i * count;
    double *out = zpart + size_t(b) * n + i;
    if (i + 1 >= n) {  // the last row has no cell right of the diagonal (the whole workgroup)
        if (tid == 0) *out = 0.0;
        return;
    }
    const uint32_t *pi = perms + size_t(b) * n;
    const double *xrow = X + size_t(i) * n;
    const double *yrow = Yc + size_t(pi[i]) * n;
    double acc = 0.0;
    for (uint32_t j0 = (i + 1) & ~uint32_t(MT_THREADS - 1); j0 < n; j0 += MT_THREADS * MT_UNROLL) {
        double xv[MT_UNROLL], yv[MT_UNROLL];
        uint32_t pj[MT_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < MT_UNROLL; u++) {
            const uint32_t j = j0 + u * MT_THREADS + tid;
            const bool valid = j > i && j < n;
            xv[u] = valid ? xrow[j] : s_x;
            pj[u] = valid ? pi[j] : DVS_NONE;
        }
#pragma unroll
        for (uint32_t u = 0; u < MT_UNROLL; u++) yv[u] = pj[u] == DVS_NONE ? 0.0 : yrow[pj[u]];
#pragma unroll
        for (uint32_t u = 0; u < MT_UNROLL; u++) {
            const double prod = (xv[u] - s_x) * yv[u];  // rounded before it is added (-ffp-contract=off)
            acc += pj[u] == DVS_NONE ? 0.0 : prod;
        }
    }
    acc = dvs_wave_sum(acc);
    if (lane == 0) s_w[wave] = acc;
    __syncthreads();
    if (tid != 0) return;
    for (uint32_t k = 1; k < MT_WAVES; k++) acc += s_w[k];
    *out = acc;
}

// Behind a scoring pass, workgroup b: the n partial sums of the batch's permutation b added into out[b] -- a thread its
// strided rows in ascending order, the lanes by the tree, the waves in wave order
__global__ __launch_bounds__(MT_THREADS) void mt_final_kernel(const double *__restrict__ zpart, uint32_t n, double *__restrict__ out) {
    __shared__ double s_w[MT_WAVES];
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const double *part = zpart + size_t(b) * n;
    double acc = 0.0;
    for (uint32_t t = tid; t < n; t += MT_THREADS) acc += part[t];
    acc = dvs_wave_sum(acc);
    if ((tid & 63) == 0) s_w[tid >> 6] = acc;
    __syncthreads();
    if (tid != 0) return;
    for (uint32_t k = 1; k < MT_WAVES; k++) acc += s_w[k];
    out[b] = acc;
}

size_t up16(size_t x) { return (x + 15) & ~size_t(15); }
uint32_t grid_of(uint32_t n, uint32_t per) { return (n + per - 1) / per; }

// what a run enqueues a pass with: the permutations a pass serves
struct MtShape {
    uint32_t batch, n_batches, per_upload;
    MtShape(const dvs_ctx *ctx, uint32_t n, uint32_t n_perm) {
        const uint32_t knob = ctx->knobs.mantel_batch;
        batch = knob ? std::min(knob, MT_MAX_BATCH) : MT_BATCH;
        n_batches = uint32_t((uint64_t(n_perm) + 1 + batch - 1) / batch);
        per_upload = uint32_t(std::min<size_t>(std::max<size_t>(MT_PERM_BYTES / batch_perm_bytes(n), 1), n_batches));
    }
    size_t batch_perm_bytes(uint32_t n) const { return size_t(n) * batch * 4; }
};

// the state of a run, one allocation: offsets in bytes
struct MtLayout {
    size_t status, Rx, Ry, U, UU, V, VV, z, zpart, perms, bytes;
    MtLayout(uint32_t n, uint32_t n_perm, const MtShape &sh) {
        status = 0;                                   // uint32 [8]
        Rx = 32;                                      // double [n] each: the rows' sums of x and y, of u, u * u, v, v * v
        Ry = Rx + size_t(n) * 8;
        U = Ry + size_t(n) * 8;
        UU = U + size_t(n) * 8;
        V = UU + size_t(n) * 8;
        VV = V + size_t(n) * 8;
        z = VV + size_t(n) * 8;                       // double [n_perm + 1]
        zpart = z + (size_t(n_perm) + 1) * 8;         // double [batch][n]
        perms = up16(zpart + size_t(sh.batch) * n * 8);  // uint32 [per_upload][batch][n]
        bytes = up16(perms + sh.batch_perm_bytes(n) * sh.per_upload);
    }
};

// row `row` of the caller's permutations into dst, unless it is not a permutation of 0 .. n - 1 (seen: n stamps, one
// value a row)
bool mantel_stage_row(const uint32_t *row, uint32_t n, std::vector<uint32_t> &seen, uint32_t stamp, uint32_t *dst) {
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t a = row[i];
        if (a >= n || seen[a] == stamp) return false;
        seen[a] = stamp;
        dst[i] = a;
    }
    return true;
}

double sum_in_order(const std::vector<double> &v) {
    double t = 0.0;
    for (double x : v) t += x;
    return t;
}

}  // namespace

size_t dvs_mantel_state_bytes(const dvs_ctx *ctx, uint32_t n, uint32_t n_perm) {
    return MtLayout(n, n_perm, MtShape(ctx, n, n_perm)).bytes;
}

// The Mantel sums over X at d_x (only read) and Y at d_y, both enqueued or resident on the context's stream; y_owned: d_y
// is a block of the library's and is centred in place, otherwise it is copied first.  Returns when the host outputs are
// written; on an error work may still be queued (the entry drains the stream).
int dvs_mantel_run(dvs_ctx *ctx, uint32_t n, const double *d_x, double *d_y, bool y_owned, const uint32_t *d_zerodiv_x,
                   const uint32_t *d_zerodiv_y, const dvs_mantel_args &a) {
    const uint32_t np = a.n_perm;
    const MtShape sh(ctx, n, np);
    const MtLayout L(n, np, sh);
    const char *what = "Mantel test";
    const hipStream_t s = ctx->stream;
    PooledBuf d_copy{ctx}, d_state{ctx};
    hipError_t e = hipSuccess;
    if (!y_owned) {
        if (int rc = dvs_dev_alloc(ctx, &d_copy.p, size_t(n) * n * 8, "Mantel working copy of the second matrix")) return rc;
        e = hipMemcpyAsync(d_copy.p, d_y, size_t(n) * n * 8, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return dvs_hip_fail(ctx, e, what);
        d_y = d_copy.as<double>();
    }
    if (int rc = dvs_dev_alloc(ctx, &d_state.p, L.bytes, "Mantel state")) return rc;
    char *base = d_state.as<char>();
    auto f64 = [&](size_t off) { return reinterpret_cast<double *>(base + off); };
    uint32_t *d_status = reinterpret_cast<uint32_t *>(base + L.status);
    double *d_z = f64(L.z), *d_zpart = f64(L.zpart);

    // ---- the entry pass: the flags, the zero-division words and the rows' sums; the shifts
    std::vector<double> Rx(n), Ry(n);
    uint32_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const dim3 rows_grid(grid_of(n, MT_WAVES)), block(MT_THREADS);
    e = dvs_status_begin(ctx, d_status, 32, MT_ST_ZERODIV_X, d_zerodiv_x);
    if (e == hipSuccess && d_zerodiv_y) e = hipMemcpyAsync(d_status + MT_ST_ZERODIV_Y, d_zerodiv_y, 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mt_entry_kernel, rows_grid, block, 0, s, d_x, n, f64(L.Rx), d_status + MT_ST_BAD_X);
        hipLaunchKernelGGL(mt_entry_kernel, rows_grid, block, 0, s, static_cast<const double *>(d_y), n, f64(L.Ry),
                           d_status + MT_ST_BAD_Y);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(st, d_status, 32, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(Rx.data(), f64(L.Rx), size_t(n) * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(Ry.data(), f64(L.Ry), size_t(n) * 8, hipMemcpyDeviceToHost, s);
    hipError_t se = hipStreamSynchronize(s);
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, what);
    if (se != hipSuccess) return dvs_hip_fail(ctx, se, what);
    if (st[MT_ST_ZERODIV_X] || st[MT_ST_ZERODIV_Y]) return dvs_set_error(ctx, DVS_ERR_ZERODIV, "division by zero");  // 0 / 0, distance.py:283
    for (int side = 0; side < 2; side++) {
        const char *which = side ? "second" : "first";
        const uint32_t bad = st[side ? MT_ST_BAD_Y : MT_ST_BAD_X];
        if (bad & MT_BAD_NONFINITE)
            return dvs_set_error(ctx, DVS_ERR_VALUE,
                                 "Input contains NaN or infinity: the %s %u x %u distance matrix above its diagonal (dvs_mantel)", which,
                                 n, n);
        if (bad & MT_BAD_NEGATIVE)
            return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_mantel: the %s %u x %u distance matrix has a negative entry above its diagonal",
                                 which, n, n);
    }
    const double m = double(uint64_t(n) * (n - 1) / 2);
    const double s_x = sum_in_order(Rx) / m, s_y = sum_in_order(Ry) / m;

    // ---- the centre pass, not waited for: its rows' sums come back with the z
    std::vector<double> U(n), UU(n), V(n), VV(n);
    hipLaunchKernelGGL((mt_centre_kernel<false>), rows_grid, block, 0, s, d_x, n, s_x, f64(L.U), f64(L.UU));
    hipLaunchKernelGGL((mt_centre_kernel<true>), rows_grid, block, 0, s, d_y, n, s_y, f64(L.V), f64(L.VV));
    e = hipGetLastError();
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, what);

    // ---- the batches: each one's permutations checked and written into its own part of the context's pinned staging
    // block and uploaded from there, then its pass and its sums -- the device works on a batch while the host checks
    // and stages the next.  After per_upload batches the stream is waited for, and the staging block and its image on
    // the device are written again (every copy out of the block has been waited for when the call returns).
    if (int rc = dvs_pinned_stage(ctx, sh.batch_perm_bytes(n) * sh.per_upload, "pinned staging block of the permutations")) return rc;
    unsigned char *stage = static_cast<unsigned char *>(ctx->h_pack);
    std::vector<uint32_t> seen(n, 0u);
    const uint64_t n_vec = uint64_t(np) + 1;
    bool bad = false;  // a row that is no permutation: nothing further is enqueued
    uint64_t bad_at = 0;
    for (uint32_t k0 = 0; k0 < sh.n_batches && e == hipSuccess && se == hipSuccess && !bad; k0 += sh.per_upload) {
        const uint32_t k1 = std::min(k0 + sh.per_upload, sh.n_batches);
        for (uint32_t k = k0; k < k1 && e == hipSuccess; k++) {
            const uint64_t v0 = uint64_t(k) * sh.batch;
            const uint32_t count = uint32_t(std::min<uint64_t>(sh.batch, n_vec - v0));
            const size_t at = sh.batch_perm_bytes(n) * (k - k0);
            uint32_t *dst = reinterpret_cast<uint32_t *>(stage + at);
            for (uint32_t b = 0; b < count && !bad; b++) {
                const uint64_t v = v0 + b;
                uint32_t *row = dst + size_t(b) * n;
                if (v == 0) {
                    for (uint32_t i = 0; i < n; i++) row[i] = i;
                } else if (!mantel_stage_row(a.perms + size_t(v - 1) * n, n, seen, uint32_t(v), row)) {
                    bad = true;
                    bad_at = v - 1;
                }
            }
            if (bad) break;
            const uint32_t *d_p = reinterpret_cast<const uint32_t *>(base + L.perms + at);
            e = hipMemcpyAsync(base + L.perms + at, dst, size_t(count) * n * 4, hipMemcpyHostToDevice, s);
            if (e != hipSuccess) break;
            const dim3 grid(n * count);
            hipLaunchKernelGGL(mt_score_kernel, grid, block, 0, s, d_x, static_cast<const double *>(d_y), n, s_x, d_p, count, d_zpart);
            hipLaunchKernelGGL(mt_final_kernel, dim3(count), block, 0, s, static_cast<const double *>(d_zpart), n, d_z + v0);
            e = hipGetLastError();
        }
        if (e == hipSuccess && !bad && k1 == sh.n_batches) {
            e = hipMemcpyAsync(a.z, d_z, size_t(n_vec) * 8, hipMemcpyDeviceToHost, s);
            const std::pair<std::vector<double> *, size_t> back[] = {{&U, L.U}, {&UU, L.UU}, {&V, L.V}, {&VV, L.VV}};
            for (const auto &bk : back)
                if (e == hipSuccess) e = hipMemcpyAsync(bk.first->data(), f64(bk.second), size_t(n) * 8, hipMemcpyDeviceToHost, s);
        }
        se = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, what);
    if (se != hipSuccess) return dvs_hip_fail(ctx, se, what);
    if (bad)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_mantel: permutation %llu is not a permutation of 0 .. %u",
                             static_cast<unsigned long long>(bad_at), n - 1);

    // ---- the invariant moments from the rows' sums, in item order; the counts on Z
    const double A = sum_in_order(U), B = sum_in_order(V);
    const double out[6] = {s_x, s_y, A, B, sum_in_order(UU), sum_in_order(VV)};
    std::copy(out, out + 6, a.moments);
    if (a.info) {
        const double c0 = (A * B) / m, z0 = a.z[0], d0 = std::fabs(z0 - c0);
        dvs_mantel_info info{0, 0, 0, 2 + sh.n_batches, sh.batch};
        for (uint32_t p = 1; p <= np; p++) {
            info.n_ge += a.z[p] >= z0;
            info.n_le += a.z[p] <= z0;
            info.n_abs_ge += std::fabs(a.z[p] - c0) >= d0;
        }
        *a.info = info;
    }
    return DVS_OK;
}
