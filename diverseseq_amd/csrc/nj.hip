// Neighbour-joining tree of a precomputed N x N distance matrix: the other tree stage of ctree, for distances that are
// (approximately) additive, as the mash distance is.  No counterpart in the reference, whose one tree is average linkage.
//
// Canonical Saitou-Nei / Studier-Keppler neighbour joining on the mirrored upper triangle of the matrix (only D[i][j],
// i < j, counts; the diagonal counts as 0), n >= 3, in f64 with no fma (-ffp-contract=off) and real divisions:
//   * slots 0 .. n - 1; leaf i starts in slot i as node i; r active slots; R[s] = sum over the other active t of D[s][t];
//   * while r > 3: Q(i, j) = double(r - 2) * D[i][j] - R[i] - R[j] over active i < j; the least Q wins, equal values go to
//     the lowest (i, j) in lexicographic slot order; record t joins node[i] and node[j] with the branch lengths
//       li = D[i][j] / 2 + (R[i] - R[j]) / (2 * double(r - 2)),   lj = D[i][j] - li;
//     the new node n + t takes slot i, slot j is retired; for every other active k
//       du = (D[i][k] + D[j][k] - D[i][j]) / 2,   R[k] = R[k] - D[i][k] - D[j][k] + du,   D[i][k] = D[k][i] = du,
//     and R[i] is summed afresh over the new row (in any order: the initial row sums too);
//   * at r = 3 (slots x < y < z) the last record joins the three nodes with
//       (Dxy + Dxz - Dyz) / 2,   (Dxy + Dyz - Dxz) / 2,   (Dxz + Dyz - Dxy) / 2.
// The tree is unrooted: n - 2 records, 2 n - 3 edges; a negative length is neighbour joining's answer on input that is
// not additive and is returned as it is.
//
// Device pipeline (one stream, every launch enqueued up front: the step count is known, nothing is read back in between):
//   1. linkage.hip's prepare pass: every entry checked (NaN / +-inf anywhere -> DVS_ERR_VALUE), the upper triangle
//      copied over the lower one; nj_rowsum_kernel: R, a wave per row.
//   2. per step nj_scan_kernel over the grid and nj_join_kernel in one workgroup, a launch boundary between them (no
//      grid barrier inside a launch: a boundary is cheaper).  The scan hands the active rows to the
//      waves of the grid (an ascending list of the active slots, dealt in alternating direction so that every wave
//      gets the same share of the triangle), streams each row's columns behind the diagonal and leaves one candidate
//      (Q, i << 32 | j) per workgroup.  A retired slot has R = NaN: its Q is NaN in every row and never the least.  The
//      join reduces the candidates by the tie rule, writes the record, updates row and column i and every R, and drops
//      slot j from the list.
//   3. nj_repack_kernel whenever r has fallen below half the matrix's current stride: the active slots move to a dense
//      leading block of another buffer in ascending slot order (the tie rule is untouched), so dead columns are not
//      streamed for ever; the buffers alternate between the matrix itself and a block a quarter of its size.
//   4. nj_final_kernel: the last record.
// A status word ends the loop early: every kernel returns at once when it is set (by the prepare pass, or by a join that
// found no pair: a matrix whose arithmetic overflowed).  No kernel spins.
//
// At the end of the file, host only: dvs_nj_patristic, the path lengths between the leaves of such a tree.
#include "dvs_internal.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int NJ_SCAN_THREADS = 256;
constexpr int NJ_SCAN_WAVES = NJ_SCAN_THREADS / 64;
constexpr int NJ_JOIN_THREADS = 1024;
constexpr int NJ_JOIN_WAVES = NJ_JOIN_THREADS / 64;
constexpr int NJ_UNROLL = 4;            // independent loads in flight per thread and pass
constexpr uint32_t NJ_MAX_GRID = 2048;  // workgroups of a scan: 8 per CU; the rows beyond that are strided over
constexpr uint32_t NJ_NONE = 0xFFFFFFFFu;
constexpr uint64_t NJ_NOKEY = ~uint64_t(0);

// status words (device): [0] prepare / loop outcome, [1] the distance kernel's zero-division flag
enum : uint32_t { NJ_OK = 0, NJ_NONFINITE = DVS_LNK_NONFINITE, NJ_NO_PAIR = 2 };

__device__ __forceinline__ bool nj_better(double v, uint64_t k, double bv, uint64_t bk) {
    return v < bv || (v == bv && k < bk);
}

__device__ __forceinline__ void nj_wave_argmin(double &bv, uint64_t &bk) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const uint64_t ok = __shfl_xor(bk, o, 64);
        if (nj_better(ov, ok, bv, bk)) {
            bv = ov;
            bk = ok;
        }
    }
}

// R[s] = sum of row s without its diagonal cell, a wave per row; the identity lists of the first step
__global__ __launch_bounds__(NJ_SCAN_THREADS) void nj_rowsum_kernel(const double *__restrict__ D, uint32_t n,
                                                                   double *__restrict__ R, uint32_t *__restrict__ node,
                                                                   uint32_t *__restrict__ act) {
    const uint32_t lane = threadIdx.x & 63, s = blockIdx.x * NJ_SCAN_WAVES + (threadIdx.x >> 6);
    if (s >= n) return;
    const double *row = D + size_t(s) * n;
    double sum = 0.0;
    for (uint32_t c = lane; c < n; c += 64)
        if (c != s) sum += row[c];
    sum = dvs_wave_sum(sum);
    if (lane == 0) {
        R[s] = sum;
        node[s] = s;
        act[s] = s;
    }
}

// The least Q(i, j), j > i, over the active rows of this workgroup's waves -> cand[blockIdx.x].  D: m slots, ld doubles
// from row to row; act: the r active slots, ascending.  Wave w of W takes the list positions w, 2 W - 1 - w, 2 W + w, ...
__global__ __launch_bounds__(NJ_SCAN_THREADS) void nj_scan_kernel(const double *__restrict__ D, uint32_t ld, uint32_t m,
                                                                 uint32_t r, const double *__restrict__ R,
                                                                 const uint32_t *__restrict__ act,
                                                                 double *__restrict__ cand_q, uint64_t *__restrict__ cand_k,
                                                                 const uint32_t *__restrict__ status) {
    __shared__ double s_q[NJ_SCAN_WAVES];
    __shared__ uint64_t s_k[NJ_SCAN_WAVES];
    if (status[0] != NJ_OK) return;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t W = gridDim.x * NJ_SCAN_WAVES, w = blockIdx.x * NJ_SCAN_WAVES + wave;
    const double rm2 = double(r - 2);
    double bq = __builtin_inf();
    uint64_t bk = NJ_NOKEY;
    for (uint32_t base = 0, pass = 0; base < r; base += W, pass++) {
        const uint32_t a = base + ((pass & 1u) ? W - 1u - w : w);
        if (a >= r) continue;
        const uint32_t s = act[a];
        const double Rs = R[s];
        const double *row = D + size_t(s) * ld;
        const uint64_t hi = uint64_t(s) << 32;
        for (uint32_t c0 = s + 1u + lane; c0 < m; c0 += 64u * NJ_UNROLL) {
            double d[NJ_UNROLL], rc[NJ_UNROLL];
#pragma unroll
            for (int u = 0; u < NJ_UNROLL; u++) {
                const uint32_t c = c0 + 64u * u;
                d[u] = c < m ? row[c] : 0.0;
                rc[u] = c < m ? R[c] : __builtin_nan("");
            }
#pragma unroll
            for (int u = 0; u < NJ_UNROLL; u++) {
                const double q = rm2 * d[u] - Rs - rc[u];  // (NaN for a retired column: never the least)
                const uint64_t key = hi | (c0 + 64u * u);
                if (nj_better(q, key, bq, bk)) {
                    bq = q;
                    bk = key;
                }
            }
        }
    }
    nj_wave_argmin(bq, bk);
    if (lane == 0) {
        s_q[wave] = bq;
        s_k[wave] = bk;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int x = 1; x < NJ_SCAN_WAVES; x++)
            if (nj_better(s_q[x], s_k[x], bq, bk)) {
                bq = s_q[x];
                bk = s_k[x];
            }
        cand_q[blockIdx.x] = bq;
        cand_k[blockIdx.x] = bk;
    }
}

// One workgroup: the least candidate by the tie rule, record t, the new row / column i, every R, the list without j.
__global__ __launch_bounds__(NJ_JOIN_THREADS) void nj_join_kernel(
    double *__restrict__ D, uint32_t ld, uint32_t r, uint32_t t, uint32_t n, double *__restrict__ R,
    uint32_t *__restrict__ node, const uint32_t *__restrict__ act, uint32_t *__restrict__ act_next,
    const double *__restrict__ cand_q, const uint64_t *__restrict__ cand_k, uint32_t ncand,
    uint32_t *__restrict__ rec_child, double *__restrict__ rec_len, uint32_t *__restrict__ status) {
    __shared__ double s_q[NJ_JOIN_WAVES];
    __shared__ uint64_t s_k[NJ_JOIN_WAVES];
    __shared__ double s_sum[NJ_JOIN_WAVES + 1];
    __shared__ uint32_t s_pos;  // position of the retired slot in the list
    if (status[0] != NJ_OK) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double bq = __builtin_inf();
    uint64_t bk = NJ_NOKEY;
    for (uint32_t c = tid; c < ncand; c += NJ_JOIN_THREADS) {
        const double q = cand_q[c];
        const uint64_t k = cand_k[c];
        if (nj_better(q, k, bq, bk)) {
            bq = q;
            bk = k;
        }
    }
    nj_wave_argmin(bq, bk);
    if (lane == 0) {
        s_q[wave] = bq;
        s_k[wave] = bk;
    }
    __syncthreads();
    bq = s_q[0];
    bk = s_k[0];
#pragma unroll
    for (int x = 1; x < NJ_JOIN_WAVES; x++)
        if (nj_better(s_q[x], s_k[x], bq, bk)) {
            bq = s_q[x];
            bk = s_k[x];
        }
    const uint32_t i = uint32_t(bk >> 32), j = uint32_t(bk);
    if (bk == NJ_NOKEY || i >= ld || j >= ld) {  // (no comparable Q: the arithmetic overflowed; never index by such a key)
        if (tid == 0) status[0] = NJ_NO_PAIR;
        return;
    }
    double *ri = D + size_t(i) * ld;
    const double *rj = D + size_t(j) * ld;
    const double dij = ri[j];
    double sum = 0.0;
    for (uint32_t t0 = tid; t0 < r; t0 += NJ_UNROLL * NJ_JOIN_THREADS) {
        uint32_t kk[NJ_UNROLL];
        double dik[NJ_UNROLL], djk[NJ_UNROLL], rk[NJ_UNROLL];
#pragma unroll
        for (int u = 0; u < NJ_UNROLL; u++) {
            const uint32_t p = t0 + u * NJ_JOIN_THREADS;
            kk[u] = p < r ? act[p] : NJ_NONE;
            if (kk[u] == j) s_pos = p;
            if (kk[u] == i || kk[u] == j) kk[u] = NJ_NONE;
        }
#pragma unroll
        for (int u = 0; u < NJ_UNROLL; u++) {
            dik[u] = kk[u] != NJ_NONE ? ri[kk[u]] : 0.0;
            djk[u] = kk[u] != NJ_NONE ? rj[kk[u]] : 0.0;
            rk[u] = kk[u] != NJ_NONE ? R[kk[u]] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < NJ_UNROLL; u++)
            if (kk[u] != NJ_NONE) {
                const double du = (dik[u] + djk[u] - dij) / 2.0;
                R[kk[u]] = rk[u] - dik[u] - djk[u] + du;
                ri[kk[u]] = du;
                D[size_t(kk[u]) * ld + i] = du;
                sum += du;
            }
    }
    sum = dvs_block_sum(sum, s_sum);  // (its barriers: s_pos is set, every thread has read its R and list entries)
    const uint32_t pos = s_pos;
    for (uint32_t p = tid; p < r; p += NJ_JOIN_THREADS)
        if (p != pos) act_next[p - (p > pos ? 1u : 0u)] = act[p];
    if (tid == 0) {
        const double Ri = R[i], Rj = R[j];
        const double li = dij / 2.0 + (Ri - Rj) / (2.0 * double(r - 2));
        rec_child[3 * size_t(t)] = node[i];
        rec_child[3 * size_t(t) + 1] = node[j];
        rec_child[3 * size_t(t) + 2] = NJ_NONE;
        rec_len[3 * size_t(t)] = li;
        rec_len[3 * size_t(t) + 1] = dij - li;
        rec_len[3 * size_t(t) + 2] = 0.0;
        R[i] = sum;
        R[j] = __builtin_nan("");  // retired
        node[i] = n + t;
    }
}

// The r active slots into the dense leading block of dst (ld_d doubles from row to row), in list order; their R and
// node ids to the front of the other copies; the list becomes the identity.  Grid (ceil(r / 256), rows strided over y).
__global__ __launch_bounds__(NJ_SCAN_THREADS) void nj_repack_kernel(
    const double *__restrict__ src, uint32_t ld_s, double *__restrict__ dst, uint32_t ld_d, uint32_t r,
    const uint32_t *__restrict__ act, uint32_t *__restrict__ act_next, const double *__restrict__ R,
    double *__restrict__ R_next, const uint32_t *__restrict__ node, uint32_t *__restrict__ node_next,
    const uint32_t *__restrict__ status) {
    if (status[0] != NJ_OK) return;
    const uint32_t q = blockIdx.x * NJ_SCAN_THREADS + threadIdx.x;
    if (q >= r) return;
    const uint32_t sq = act[q];
    for (uint32_t p = blockIdx.y; p < r; p += gridDim.y)
        dst[size_t(p) * ld_d + q] = src[size_t(act[p]) * ld_s + sq];
    if (blockIdx.y == 0) {
        R_next[q] = R[sq];
        node_next[q] = node[sq];
        act_next[q] = q;
    }
}

// the last record: the three slots that are left
__global__ void nj_final_kernel(const double *__restrict__ D, uint32_t ld, uint32_t t, const uint32_t *__restrict__ node,
                                const uint32_t *__restrict__ act, uint32_t *__restrict__ rec_child,
                                double *__restrict__ rec_len, const uint32_t *__restrict__ status) {
    if (status[0] != NJ_OK || threadIdx.x != 0) return;
    const uint32_t x = act[0], y = act[1], z = act[2];
    const double dxy = D[size_t(x) * ld + y], dxz = D[size_t(x) * ld + z], dyz = D[size_t(y) * ld + z];
    rec_child[3 * size_t(t)] = node[x];
    rec_child[3 * size_t(t) + 1] = node[y];
    rec_child[3 * size_t(t) + 2] = node[z];
    rec_len[3 * size_t(t)] = (dxy + dxz - dyz) / 2.0;
    rec_len[3 * size_t(t) + 1] = (dxy + dyz - dxz) / 2.0;
    rec_len[3 * size_t(t) + 2] = (dxz + dyz - dxy) / 2.0;
}

// byte offsets of the scratch block: what is copied back first, then what stays on the device.  R, node and act exist
// twice: a join writes the next list beside the one it reads, a repack the next of all three.
struct NjLayout {
    size_t status, rec_len, rec_child, out_bytes, R[2], node[2], act[2], cand_q, cand_k, bytes;
    explicit NjLayout(uint32_t n) {
        auto up8 = [](size_t v) { return (v + 7) & ~size_t(7); };
        const size_t recs = 3 * (size_t(n) - 2);
        status = 0;
        rec_len = 16;
        rec_child = rec_len + recs * 8;
        out_bytes = up8(rec_child + recs * 4);
        R[0] = out_bytes;
        R[1] = R[0] + size_t(n) * 8;
        cand_q = R[1] + size_t(n) * 8;
        cand_k = cand_q + size_t(NJ_MAX_GRID) * 8;
        node[0] = cand_k + size_t(NJ_MAX_GRID) * 8;
        node[1] = node[0] + size_t(n) * 4;
        act[0] = node[1] + size_t(n) * 4;
        act[1] = act[0] + size_t(n) * 4;
        bytes = up8(act[1] + size_t(n) * 4);
    }
};

// doubles of the second matrix buffer: the first repack moves r < n / 2 slots into it, every later one fewer
size_t nj_pack_elems(uint32_t n) {
    const size_t h = (size_t(n) - 1) / 2;
    return h * h + 1;
}

}  // namespace

// A consumer's run (dvs_internal.h dvs_square_consumer): the neighbour-joining tree of the n x n matrix at d_dist (a
// working buffer: overwritten), n >= 3, enqueued on the context's stream behind whatever wrote the matrix.  Returns
// when the host outputs (dvs_nj's) are written.
static int nj_run(dvs_ctx *ctx, double *d_dist, uint32_t n, const uint32_t *d_zerodiv, uint32_t *joins, double *lengths) {
    const NjLayout L(n);
    PooledBuf scratch{ctx}, pack{ctx};
    int rc = dvs_dev_alloc(ctx, &scratch.p, L.bytes, "neighbour-joining scratch");
    if (!rc) rc = dvs_dev_alloc(ctx, &pack.p, nj_pack_elems(n) * 8, "neighbour-joining repack buffer");
    if (rc) return rc;
    char *base = scratch.as<char>();
    auto u32 = [&](size_t off) { return reinterpret_cast<uint32_t *>(base + off); };
    auto f64 = [&](size_t off) { return reinterpret_cast<double *>(base + off); };
    uint32_t *d_status = u32(L.status);
    std::vector<uint64_t> host((L.out_bytes + 7) / 8);
    const char *what = "neighbour joining";
    hipError_t e = dvs_status_begin(ctx, d_status, 16, 1, d_zerodiv);
    if (e == hipSuccess) e = dvs_linkage_enqueue_prepare(ctx, d_dist, n, false, d_status);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(nj_rowsum_kernel, dim3((n + NJ_SCAN_WAVES - 1) / NJ_SCAN_WAVES), dim3(NJ_SCAN_THREADS), 0,
                           ctx->stream, d_dist, n, f64(L.R[0]), u32(L.node[0]), u32(L.act[0]));
        e = hipGetLastError();
    }
    // cur / other: the buffer that holds the matrix (m slots, ld doubles from row to row) and the one the next repack fills
    double *cur = d_dist, *other = pack.as<double>();
    uint32_t m = n, ld = n, r = n;
    int ia = 0, iv = 0;  // which copy of act / of R and node is current
    for (uint32_t t = 0; e == hipSuccess && r > 3; t++, r--) {
        if (2 * uint64_t(r) < m) {
            const dim3 grid((r + NJ_SCAN_THREADS - 1) / NJ_SCAN_THREADS, std::min<uint32_t>(r, 1024u));
            hipLaunchKernelGGL(nj_repack_kernel, grid, dim3(NJ_SCAN_THREADS), 0, ctx->stream, cur, ld, other, r, r,
                               u32(L.act[ia]), u32(L.act[ia ^ 1]), f64(L.R[iv]), f64(L.R[iv ^ 1]), u32(L.node[iv]),
                               u32(L.node[iv ^ 1]), d_status);
            std::swap(cur, other);
            m = ld = r;
            ia ^= 1;
            iv ^= 1;
        }
        const uint32_t grid = std::min<uint32_t>(NJ_MAX_GRID, (r + NJ_SCAN_WAVES - 1) / NJ_SCAN_WAVES);
        hipLaunchKernelGGL(nj_scan_kernel, dim3(grid), dim3(NJ_SCAN_THREADS), 0, ctx->stream, cur, ld, m, r, f64(L.R[iv]),
                           u32(L.act[ia]), f64(L.cand_q), reinterpret_cast<uint64_t *>(base + L.cand_k), d_status);
        hipLaunchKernelGGL(nj_join_kernel, dim3(1), dim3(NJ_JOIN_THREADS), 0, ctx->stream, cur, ld, r, t, n, f64(L.R[iv]),
                           u32(L.node[iv]), u32(L.act[ia]), u32(L.act[ia ^ 1]), f64(L.cand_q),
                           reinterpret_cast<const uint64_t *>(base + L.cand_k), grid, u32(L.rec_child), f64(L.rec_len),
                           d_status);
        ia ^= 1;
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(nj_final_kernel, dim3(1), dim3(64), 0, ctx->stream, cur, ld, n - 3, u32(L.node[iv]),
                           u32(L.act[ia]), u32(L.rec_child), f64(L.rec_len), d_status);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), base, L.out_bytes, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t se = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, what);
    if (se != hipSuccess) return dvs_hip_fail(ctx, se, what);
    const char *hb = reinterpret_cast<const char *>(host.data());
    const uint32_t *st = reinterpret_cast<const uint32_t *>(hb + L.status);
    if (st[1]) return dvs_set_error(ctx, DVS_ERR_ZERODIV, "division by zero");  // 0 / 0, distance.py:283
    if (st[0] & NJ_NONFINITE)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "Input contains NaN or infinity: the %u x %u distance matrix", n, n);
    if (st[0] != NJ_OK)
        return dvs_set_error(ctx, DVS_ERR_RUNTIME, "neighbour joining: no pair to join (the distances overflow in f64)");
    const size_t recs = 3 * (size_t(n) - 2);
    std::copy_n(reinterpret_cast<const uint32_t *>(hb + L.rec_child), recs, joins);
    std::copy_n(reinterpret_cast<const double *>(hb + L.rec_len), recs, lengths);
    return DVS_OK;
}

// beside the matrix: the second buffer and the loop's scratch
dvs_square_consumer dvs_nj_consumer(dvs_ctx *ctx, uint32_t n, uint32_t *joins, double *lengths) {
    dvs_square_consumer c{"dvs_nj"};
    c.check = [=] {
        if (n < 3) return dvs_set_error(ctx, DVS_ERR_VALUE, "need at least three sequences for a neighbour-joining tree");
        return int(DVS_OK);
    };
    c.extra_bytes = [=] { return nj_pack_elems(n) * 8 + NjLayout(n).bytes; };
    snprintf(c.extra_what, sizeof c.extra_what, "its neighbour-joining tree");
    c.writes_matrix = true;
    c.run = [=](double *d_dist, const uint32_t *d_zerodiv) { return nj_run(ctx, d_dist, n, d_zerodiv, joins, lengths); };
    return c;
}

// The path lengths between the leaves (host only).  A record's children were made before it, so rooted at the last
// record a parent's id is above its children's: sizes bottom-up, then top-down every node's leaves as one range of a
// leaf order; bottom-up again, h[leaf] grows to the leaf's distance from the node at hand, and two leaves below
// different children of that node are h[a] + h[b] apart.  Every pair meets once: O(n^2) additions for the cells, and
// one per leaf and ancestor for h.
extern "C" int dvs_nj_patristic(dvs_ctx *ctx, uint32_t n, const uint32_t *joins, const double *lengths, double *out) {
    if (!joins || !lengths || !out) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (n < 3) return dvs_set_error(ctx, DVS_ERR_VALUE, "a neighbour-joining tree has three leaves at least, not %u", n);
    if (n > 0x40000000u) return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "a tree of %u leaves: 2^30 at most", n);
    const uint32_t nrec = n - 2, nnode = 2 * n - 2;
    std::vector<uint32_t> size(nnode, 1u), lo(nnode, 0u);
    std::vector<bool> used(nnode, false);
    for (uint32_t t = 0; t < nrec; t++) {
        const uint32_t kids = t + 1 == nrec ? 3u : 2u;
        if (kids == 2 && joins[3 * size_t(t) + 2] != NJ_NONE)
            return dvs_set_error(ctx, DVS_ERR_VALUE, "record %u: only the last record has a third child", t);
        uint32_t s = 0;
        for (uint32_t c = 0; c < kids; c++) {
            const uint32_t v = joins[3 * size_t(t) + c];
            if (v >= n + t || used[v])
                return dvs_set_error(ctx, DVS_ERR_VALUE, "record %u joins node %u: not a node that exists and is free at "
                                     "that point", t, v);
            used[v] = true;
            s += size[v];
        }
        size[n + t] = s;
    }
    for (uint32_t t = nrec; t-- > 0;) {  // (the root's range starts at 0)
        const uint32_t kids = t + 1 == nrec ? 3u : 2u;
        uint32_t at = lo[n + t];
        for (uint32_t c = 0; c < kids; c++) {
            const uint32_t v = joins[3 * size_t(t) + c];
            lo[v] = at;
            at += size[v];
        }
    }
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[lo[i]] = i;
    std::vector<double> h(n, 0.0);  // by position in `order`
    for (uint32_t i = 0; i < n; i++) out[size_t(i) * n + i] = 0.0;
    for (uint32_t t = 0; t < nrec; t++) {
        const uint32_t kids = t + 1 == nrec ? 3u : 2u;
        for (uint32_t c = 0; c < kids; c++) {
            const uint32_t v = joins[3 * size_t(t) + c];
            const double len = lengths[3 * size_t(t) + c];
            for (uint32_t p = lo[v]; p < lo[v] + size[v]; p++) h[p] += len;
        }
        for (uint32_t c = 0; c < kids; c++)
            for (uint32_t d = c + 1; d < kids; d++) {
                const uint32_t v = joins[3 * size_t(t) + c], w = joins[3 * size_t(t) + d];
                for (uint32_t p = lo[v]; p < lo[v] + size[v]; p++)
                    for (uint32_t q = lo[w]; q < lo[w] + size[w]; q++) {
                        const double x = h[p] + h[q];
                        out[size_t(order[p]) * n + order[q]] = x;
                        out[size_t(order[q]) * n + order[p]] = x;
                    }
            }
    }
    return DVS_OK;
}
