// Farthest-first (max-min) selection of representatives by distance: include/dvs_hip.h "farthest-first selection" pins
// the algorithm.  No counterpart in the reference, whose selection is by delta-JSD (records.rs) and whose distances fill
// the N x N matrix of one collection.
//
// A pick costs one row of distances, never the matrix.  Device pipeline (one stream; steps are enqueued a batch ahead
// and nothing is read back inside a batch):
//   per step t (the row of pick t, whose index every kernel reads from the device pick list):
//     1. the distances of pick t to every item and the update of mind / owner / flag by the pinned rule, which leaves
//        one candidate (the largest mind of a live item, the lowest item of equal values) per workgroup:
//          jsd        jsd_row_kernel: a lane per pair, the cell of jsd_cross_kernel bit for bit, the update in its
//                     epilogue -- no N-length row is written
//          mash       mash_pairs_kernel<true> (mash.hip) with the pick list as its query list, q0 = t, one query row
//          euclidean  euclid_cross_kernel (crossdist.hip) likewise
//          a matrix   nothing: row picks[t] of the matrix is the row
//        the last three followed by (for the matrix: consisting of) maxmin_update_kernel over the N-length row;
//     2. maxmin_pick_kernel, one workgroup behind a launch boundary (no grid barrier, no spinning: DESIGN.md 4.12 item
//        3): the candidates reduced by the tie rule in a fixed tree, the stop rules, pick t + 1 written and marked.
//   A status word ends the traversal: every kernel of this file returns at once when it is set (the reused distance
//   kernels know no such word: behind the end they fill a row nobody reads, of a query the init kernel made valid).
//   Between two batches
//   (DVS_MAXMIN_BATCH steps, 64 by default) the host reads the status word, so a min_distance run that ends after a few
//   picks does not enqueue n_select empty steps.
#include "dvs_internal.h"
#include "rowdist_dev.h"

#include <algorithm>
#include <cmath>
#include <type_traits>


namespace {

constexpr uint32_t MM_NONE = 0xFFFFFFFFu;
constexpr uint32_t MM_ROW_PAIRS = 64;  // jsd_row_kernel: pairs per workgroup, a lane each ...
constexpr int MM_ROW_WAVES = 16;       // ... in every one of its waves, which share out the bins of a chunk
constexpr int MM_ROW_THREADS = 64 * MM_ROW_WAVES;
constexpr uint32_t MM_ROW_BINS = JSD_CHUNK / MM_ROW_WAVES;  // bins per wave and chunk
constexpr int MM_UPD_THREADS = 256;
constexpr int MM_PICK_THREADS = 1024;
constexpr uint32_t MM_BATCH = 64;
enum : uint8_t { MM_LIVE = 0, MM_TAKEN = 1, MM_OUT = 2 };
// the status block (device, uint32): [0] set when the traversal has ended, [1] the number of picks, [2] a visited
// mash pair divides by zero (the word mash_pairs_kernel itself sets also speaks for the pick's own cell, which is not a
// pair: it stays in the stage's scratch and is not looked at)
enum { MM_ST_DONE = 0, MM_ST_NPICKED = 1, MM_ST_ZERODIV = 2 };

struct MaxminState {
    double *mind;      // [n] distance to the nearest pick
    uint32_t *owner;   // [n] its position in the pick list
    uint8_t *flag;     // [n] MM_LIVE / MM_TAKEN / MM_OUT
    uint32_t *picks;   // [n_select] rows in pick order; the seeds are there from the start
    double *radius;    // [n_select]
    uint32_t *status;  // the status block
    double *cover;
    double *cand_v;    // per workgroup of step 1: the best live (mind, item); item MM_NONE: none
    uint32_t *cand_j;
};

// the tie rule: the larger value, then the lower item; an entry without an item loses to any with one
__device__ __forceinline__ bool mm_better(double v, uint32_t j, double bv, uint32_t bj) {
    return j != MM_NONE && (bj == MM_NONE || v > bv || (v == bv && j < bj));
}

__device__ __forceinline__ void mm_wave_best(double &bv, uint32_t &bj) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const uint32_t oj = __shfl_xor(bj, o, 64);
        if (mm_better(ov, oj, bv, bj)) {
            bv = ov;
            bj = oj;
        }
    }
}

// take(p, .)'s rule for item j, c = d(p, j): the item's candidate afterwards (cj = MM_NONE: it is not live).  `zerodiv`
// (mash only): a NaN cell of a visited pair is 0 / 0 between two empty sketches.
__device__ __forceinline__ void mm_apply(const MaxminState &S, uint32_t j, uint32_t n, uint32_t p, uint32_t t, double c,
                                         bool mash, double &cv, uint32_t &cj) {
    cv = 0.0;
    cj = MM_NONE;
    if (j >= n || j == p || S.flag[j] != MM_LIVE) return;
    double m = S.mind[j];
    if (c != c) {
        S.flag[j] = MM_OUT;
        S.mind[j] = c;
        S.owner[j] = MM_NONE;
        if (mash) S.status[MM_ST_ZERODIV] = 1u;
        return;
    }
    if (c < m) {
        S.mind[j] = m = c;
        S.owner[j] = t;
    }
    cv = m;
    cj = j;
}

// One query row -- pick t -- against the n rows of the same matrix: the cell of jsd_cross_kernel (half frequencies by
// count_freq_x, one accumulator per pair, jsd_add per bin in ascending bin order, its finish expression, clamp and NaN
// rule; h: jsd_entropy_kernel's row entropies), then the update rule on the cell.  A workgroup takes 64 consecutive rows,
// a lane per pair -- in each of its 16 waves.  jsd_add is acc = fma(-m, log2_tab(max(m, 2^-1000)), acc): only that last
// fma depends on the bin before, so per chunk of 64 bins wave w works out m and its logarithm for bins 4 w .. 4 w + 3 of
// all 64 pairs (a lane reads its own row: the 16 waves share the row's cache line) and leaves them in LDS, and wave 0
// then runs the 64 fmas of each pair in bin order: the same operations on the same values in the same order, so the same
// bits, with the logarithms -- nine tenths of the arithmetic -- spread over 16 times as many waves as a lane per pair
// alone would give (at N = 10 000 that is 2 512 waves instead of 157 on 1 024 SIMDs).  A workgroup without a live item
// has nothing to compute.
template <typename T>
__global__ __launch_bounds__(MM_ROW_THREADS) void jsd_row_kernel(const T *__restrict__ mat, const uint32_t *__restrict__ totals,
                                                                 uint32_t n, uint64_t B, const double *__restrict__ h,
                                                                 uint32_t t, MaxminState S) {
    __shared__ double2 tab[128];
    __shared__ double s_m[JSD_CHUNK * MM_ROW_PAIRS], s_l[JSD_CHUNK * MM_ROW_PAIRS];  // [bin of the chunk][pair]
    if (S.status[MM_ST_DONE]) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t j0 = blockIdx.x * MM_ROW_PAIRS, j = j0 + lane;
    const uint32_t p = S.picks[t];
    // (every wave sees the same 64 flags: wave 0 writes them behind the last barrier only)
    const bool live = j < n && j != p && S.flag[j] == MM_LIVE;
    if (!__any(live)) {
        if (tid == 0) S.cand_j[blockIdx.x] = MM_NONE;
        return;
    }
    if (tid < 128) log2_tab_fill(tab, int(tid));
    const double tq = double(totals[p]), rq = tq > 0.0 ? 1.0 / tq : 0.0;
    const double tj = j < n ? double(totals[j]) : 0.0, rj = tj > 0.0 ? 1.0 / tj : 0.0;
    const T *qrow = mat + uint64_t(p) * B, *rrow = mat + uint64_t(j < n ? j : 0u) * B;
    double acc = 0.0;
    __syncthreads();
    for (uint64_t c0 = 0; c0 < B; c0 += JSD_CHUNK) {
        const uint32_t cn = uint32_t(B - c0 < JSD_CHUNK ? B - c0 : JSD_CHUNK);
#pragma unroll
        for (uint32_t u = 0; u < MM_ROW_BINS; u++) {
            const uint32_t b = wave * MM_ROW_BINS + u;
            if (b < cn) {
                const double q = tq > 0.0 ? 0.5 * count_freq_x(qrow[c0 + b], tq, rq) : 0.0;
                const double f = tj > 0.0 ? 0.5 * count_freq_x(rrow[c0 + b], tj, rj) : 0.0;
                const double m = q + f;
                s_m[b * MM_ROW_PAIRS + lane] = m;
                s_l[b * MM_ROW_PAIRS + lane] = log2_tab(fmax(m, 0x1p-1000), tab);
            }
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll 8
            for (uint32_t b = 0; b < cn; b++) acc = fma(-s_m[b * MM_ROW_PAIRS + lane], s_l[b * MM_ROW_PAIRS + lane], acc);  // (jsd_add)
        }
        __syncthreads();
    }
    if (wave != 0) return;
    double d = NAN;
    if (j < n) {
        d = acc - 0.5 * (h[p] + h[j]);  // (jsd_cross_kernel's finish)
        d = d < 0.0 ? 0.0 : d;
        d = d > 1.0 ? 1.0 : d;
        if (tq == 0.0 || tj == 0.0) d = NAN;
    }
    double cv;
    uint32_t cj;
    mm_apply(S, j, n, p, t, d, false, cv, cj);
    mm_wave_best(cv, cj);
    if (tid == 0) {
        S.cand_v[blockIdx.x] = cv;
        S.cand_j[blockIdx.x] = cj;
    }
}

// The update rule over an N-length row of distances from pick t: row = base + picks[t] * ld (ld = 0: the row a distance
// kernel has just written; ld = n: the caller's matrix).
__global__ __launch_bounds__(MM_UPD_THREADS) void maxmin_update_kernel(const double *__restrict__ base, uint64_t ld, uint32_t n,
                                                                       uint32_t t, int mash, MaxminState S) {
    __shared__ double s_v[MM_UPD_THREADS / 64];
    __shared__ uint32_t s_j[MM_UPD_THREADS / 64];
    if (S.status[MM_ST_DONE]) return;
    const uint32_t j = blockIdx.x * MM_UPD_THREADS + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t p = S.picks[t];
    const double *row = base + uint64_t(p) * ld;
    double cv;
    uint32_t cj;
    mm_apply(S, j, n, p, t, j < n && j != p ? row[j] : 0.0, mash != 0, cv, cj);
    mm_wave_best(cv, cj);
    if (lane == 0) {
        s_v[wave] = cv;
        s_j[wave] = cj;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < MM_UPD_THREADS / 64; w++)
            if (mm_better(s_v[w], s_j[w], cv, cj)) {
                cv = s_v[w];
                cj = s_j[w];
            }
        S.cand_v[blockIdx.x] = cv;
        S.cand_j[blockIdx.x] = cj;
    }
}

// hq[t] = h[picks[t]]: the query's entropy where jsd_cross_kernel looks for it (the A/B mode, DVS_MAXMIN_JSD_CROSS)
__global__ void maxmin_query_entropy_kernel(const double *__restrict__ h, double *__restrict__ hq, uint32_t t, MaxminState S) {
    if (threadIdx.x == 0 && blockIdx.x == 0) hq[t] = h[S.picks[t]];
}

// every item live and unowned, the first seed taken, the seeds' radii NaN.  The pick list behind the seeds starts as
// the first seed: the distance kernels of mash.hip and crossdist.hip know no status word and read their query from the
// list even in a step enqueued behind the traversal's end -- a row nobody looks at, but of a row that exists.
__global__ __launch_bounds__(MM_UPD_THREADS) void maxmin_init_kernel(uint32_t n, uint32_t n_seeds, uint32_t n_select,
                                                                     MaxminState S) {
    const uint32_t j = blockIdx.x * MM_UPD_THREADS + threadIdx.x;
    const uint32_t p = S.picks[0];
    if (j < n) {
        S.mind[j] = j == p ? 0.0 : __builtin_inf();
        S.owner[j] = j == p ? 0u : MM_NONE;
        S.flag[j] = j == p ? MM_TAKEN : MM_LIVE;
    }
    if (j < n_seeds) S.radius[j] = __builtin_nan("");
    if (j >= n_seeds && j < n_select) S.picks[j] = p;
    if (j == 0) {
        S.status[MM_ST_DONE] = 0u;
        S.status[MM_ST_NPICKED] = 1u;
        S.status[MM_ST_ZERODIV] = 0u;
        S.cover[0] = 0.0;
    }
}

// One workgroup behind step t's update: the next seed, or the best candidate by the tie rule under the stop rules, is
// pick t + 1; behind the last step (t + 1 == n_select) and at a stop the covering radius instead, and the status word.
__global__ __launch_bounds__(MM_PICK_THREADS) void maxmin_pick_kernel(uint32_t ncand, uint32_t t, uint32_t n_seeds,
                                                                      uint32_t n_select, int use_min, double min_distance,
                                                                      MaxminState S) {
    __shared__ double s_v[MM_PICK_THREADS / 64];
    __shared__ uint32_t s_j[MM_PICK_THREADS / 64];
    if (S.status[MM_ST_DONE]) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (t + 1 < n_seeds) {
        if (tid == 0) {
            const uint32_t p = S.picks[t + 1];
            S.flag[p] = MM_TAKEN;
            S.mind[p] = 0.0;
            S.owner[p] = t + 1;
            S.status[MM_ST_NPICKED] = t + 2;
        }
        return;
    }
    double bv = 0.0;
    uint32_t bj = MM_NONE;
    for (uint32_t c = tid; c < ncand; c += MM_PICK_THREADS) {
        const uint32_t j = S.cand_j[c];
        const double v = j != MM_NONE ? S.cand_v[c] : 0.0;
        if (mm_better(v, j, bv, bj)) {
            bv = v;
            bj = j;
        }
    }
    mm_wave_best(bv, bj);
    if (lane == 0) {
        s_v[wave] = bv;
        s_j[wave] = bj;
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 1; w < MM_PICK_THREADS / 64; w++)
        if (mm_better(s_v[w], s_j[w], bv, bj)) {
            bv = s_v[w];
            bj = s_j[w];
        }
    if (t + 1 >= n_select || bj == MM_NONE || (use_min && !(bv > min_distance))) {
        S.cover[0] = bj == MM_NONE ? 0.0 : bv;
        S.status[MM_ST_DONE] = 1u;
        return;
    }
    S.picks[t + 1] = bj;
    S.radius[t + 1] = bv;
    S.flag[bj] = MM_TAKEN;
    S.mind[bj] = 0.0;
    S.owner[bj] = t + 1;
    S.status[MM_ST_NPICKED] = t + 2;
}

struct MaxminArgs {
    uint32_t n;
    const uint32_t *seeds;
    uint32_t n_seeds, n_select;
    int use_min_distance;
    double min_distance;
    uint32_t *picks;
    double *radius;
    uint32_t *n_picked, *owner;
    double *dist_to_owner, *cover;
};

// what every entry checks before any device work
int maxmin_check(dvs_ctx *ctx, const MaxminArgs &a) {
    if (!a.seeds || !a.picks || !a.radius || !a.n_picked || !a.owner || !a.dist_to_owner || !a.cover)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (a.n_seeds == 0) return dvs_set_error(ctx, DVS_ERR_VALUE, "farthest-first selection needs at least one seed");
    if (a.n_select < a.n_seeds || a.n_select > a.n)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "n_select = %u: between the number of seeds (%u) and the number of rows (%u)",
                             a.n_select, a.n_seeds, a.n);
    std::vector<bool> seen(a.n, false);
    for (uint32_t i = 0; i < a.n_seeds; i++) {
        if (a.seeds[i] >= a.n) return dvs_set_error(ctx, DVS_ERR_VALUE, "seed %u is row %u of %u", i, a.seeds[i], a.n);
        if (seen[a.seeds[i]]) return dvs_set_error(ctx, DVS_ERR_VALUE, "row %u is a seed more than once", a.seeds[i]);
        seen[a.seeds[i]] = true;
    }
    if (a.use_min_distance && a.min_distance != a.min_distance)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "min_distance is NaN");
    return DVS_OK;
}

// What a mode adds to the traversal: `extra` bytes of device scratch of its own (`what` in an allocation error), set up
// once by prepare(d_extra); step(t, d_extra, d_row, S) enqueues the distances of pick t and the update behind them and
// leaves `ncand` candidates.  with_row: the mode's kernels write an N-length row.
struct MaxminMode {
    const char *label;
    size_t extra;
    const char *what;
    bool with_row;
    uint32_t ncand;
    std::function<hipError_t(void *d_extra, const MaxminState &S)> prepare;
    std::function<hipError_t(uint32_t t, void *d_extra, double *d_row, const MaxminState &S)> step;
};

uint32_t upd_blocks(uint32_t n) { return (n + MM_UPD_THREADS - 1) / MM_UPD_THREADS; }

hipError_t enqueue_update(dvs_ctx *ctx, const double *base, uint64_t ld, uint32_t n, uint32_t t, int mash, const MaxminState &S) {
    hipLaunchKernelGGL(maxmin_update_kernel, dim3(upd_blocks(n)), dim3(MM_UPD_THREADS), 0, ctx->stream, base, ld, n, t, mash, S);
    return hipGetLastError();
}

// byte offsets of the state, one block: what is copied back first (status, cover, radius, picks), then owner, mind,
// then the rest
struct MaxminLayout {
    size_t cover, radius, picks, owner, mind, flag, cv, cj, row, bytes;
    MaxminLayout(uint32_t n, uint32_t ns) {
        auto up8 = [](size_t v) { return (v + 7) & ~size_t(7); };
        const uint32_t max_cand = (n + 63) / 64;
        cover = 16, radius = cover + 8, picks = radius + size_t(ns) * 8, owner = up8(picks + size_t(ns) * 4);
        mind = up8(owner + size_t(n) * 4), flag = mind + size_t(n) * 8;
        cv = up8(flag + n), cj = cv + size_t(max_cand) * 8, row = up8(cj + size_t(max_cand) * 4);
        bytes = row + size_t(n) * 8;
    }
};

// The traversal over a mode (the arguments checked, the device set).  make(S) builds the mode around the device state:
// its query list is S.picks.
template <typename F>
int maxmin_run(dvs_ctx *ctx, const MaxminArgs &a, F &&make) {
    const uint32_t n = a.n, ns = a.n_select;
    const MaxminLayout L(n, ns);
    PooledBuf d_buf{ctx}, d_extra{ctx};
    int rc = dvs_dev_alloc(ctx, &d_buf.p, L.bytes, "farthest-first state");
    if (rc) return rc;
    char *base = d_buf.as<char>();
    MaxminState S;
    S.status = reinterpret_cast<uint32_t *>(base);
    S.cover = reinterpret_cast<double *>(base + L.cover);
    S.radius = reinterpret_cast<double *>(base + L.radius);
    S.picks = reinterpret_cast<uint32_t *>(base + L.picks);
    S.owner = reinterpret_cast<uint32_t *>(base + L.owner);
    S.mind = reinterpret_cast<double *>(base + L.mind);
    S.flag = reinterpret_cast<uint8_t *>(base + L.flag);
    S.cand_v = reinterpret_cast<double *>(base + L.cv);
    S.cand_j = reinterpret_cast<uint32_t *>(base + L.cj);
    double *d_row = reinterpret_cast<double *>(base + L.row);
    const MaxminMode mode = make(S);
    if (mode.extra) {
        rc = dvs_dev_alloc(ctx, &d_extra.p, mode.extra, mode.what);
        if (rc) return rc;
    }
    hipError_t e = hipMemcpyAsync(S.picks, a.seeds, size_t(a.n_seeds) * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(maxmin_init_kernel, dim3(upd_blocks(std::max(n, a.n_seeds))), dim3(MM_UPD_THREADS), 0, ctx->stream, n,
                           a.n_seeds, ns, S);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = mode.prepare(d_extra.p, S);
    const uint32_t batch = ctx->knobs.maxmin_batch ? ctx->knobs.maxmin_batch : MM_BATCH;
    uint32_t status[4] = {0, 0, 0, 0};
    hipError_t se = hipSuccess;
    for (uint32_t t0 = 0; e == hipSuccess && se == hipSuccess && t0 < ns && !status[MM_ST_DONE] && !status[MM_ST_ZERODIV];) {
        const uint32_t t1 = uint32_t(std::min<uint64_t>(uint64_t(t0) + batch, ns));
        for (uint32_t t = t0; e == hipSuccess && t < t1; t++) {
            e = mode.step(t, d_extra.p, d_row, S);
            if (e != hipSuccess) break;
            hipLaunchKernelGGL(maxmin_pick_kernel, dim3(1), dim3(MM_PICK_THREADS), 0, ctx->stream, mode.ncand, t, a.n_seeds, ns,
                               a.use_min_distance, a.min_distance, S);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(status, S.status, 16, hipMemcpyDeviceToHost, ctx->stream);
        se = hipStreamSynchronize(ctx->stream);
        t0 = t1;
    }
    std::vector<uint64_t> head;
    if (e == hipSuccess && se == hipSuccess && !status[MM_ST_ZERODIV]) {
        const uint32_t np = std::min(status[MM_ST_NPICKED], ns);
        head.resize(L.owner / 8);
        e = hipMemcpyAsync(head.data(), base, L.owner, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(a.owner, S.owner, size_t(n) * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(a.dist_to_owner, S.mind, size_t(n) * 8, hipMemcpyDeviceToHost, ctx->stream);
        se = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess && se == hipSuccess) {
            const char *hb = reinterpret_cast<const char *>(head.data());
            *a.n_picked = np;
            *a.cover = *reinterpret_cast<const double *>(hb + L.cover);
            std::copy_n(reinterpret_cast<const double *>(hb + L.radius), np, a.radius);
            std::copy_n(reinterpret_cast<const uint32_t *>(hb + L.picks), np, a.picks);
        }
    } else if (se == hipSuccess) {
        se = hipStreamSynchronize(ctx->stream);  // (the blocks go back to the cache behind it)
    }
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, mode.label);
    if (se != hipSuccess) return dvs_hip_fail(ctx, se, mode.label);
    if (status[MM_ST_ZERODIV]) return dvs_set_error(ctx, DVS_ERR_ZERODIV, "division by zero");  // 0 / 0, distance.py:283
    return DVS_OK;
}

// n == 1: the seed and nothing to measure
int maxmin_single(const MaxminArgs &a) {
    a.picks[0] = 0;
    a.radius[0] = NAN;
    *a.n_picked = 1;
    a.owner[0] = 0;
    a.dist_to_owner[0] = 0.0;
    *a.cover = 0.0;
    return DVS_OK;
}

int matrix_check(dvs_ctx *ctx, const dvs_matrix *m, uint32_t n) {
    if (m->device != ctx->device) return dvs_set_error(ctx, DVS_ERR_VALUE, "the matrix and the context are not on one device");
    if (n > m->nrows) return dvs_set_error(ctx, DVS_ERR_VALUE, "%u rows of a handle that holds %u", n, m->nrows);
    return DVS_OK;
}

// a mode whose distance kernels are a rectangular stage's, run on one query row: the stage's query list is the pick
// list, q0 the step
MaxminMode stage_mode(dvs_ctx *ctx, const dvs_cross_stage &st, uint32_t n, bool mash) {
    MaxminMode mode{st.label, st.scratch_bytes, st.scratch_what, true, upd_blocks(n)};
    mode.prepare = [=](void *d_extra, const MaxminState &) { return st.prepare(d_extra); };
    mode.step = [=](uint32_t t, void *d_extra, double *d_row, const MaxminState &S) {
        hipError_t e = st.enqueue(t, 1u, d_row, d_extra);
        if (e == hipSuccess) e = enqueue_update(ctx, d_row, 0, n, t, mash, S);
        return e;
    };
    return mode;
}

// ---- the traversal over each kind of source: the arguments checked by maxmin_check

int maxmin_given(dvs_ctx *ctx, const MaxminArgs &a, const double *dist, int dist_on_device) {
    const uint32_t n = a.n;
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    PooledBuf d_dist{ctx};
    const double *d_mat = dist;
    int rc = dist_on_device ? dvs_given_on_device(ctx, nullptr, dist) : DVS_OK;
    if (!rc) rc = dvs_square_fits(ctx, nullptr, n, !dist_on_device, MaxminLayout(n, a.n_select).bytes, "the farthest-first state");
    if (!rc && !dist_on_device) rc = dvs_given_upload(ctx, dist, n, &d_dist);
    if (rc) return rc;
    if (!dist_on_device) d_mat = d_dist.as<double>();
    return maxmin_run(ctx, a, [&](const MaxminState &) {
        MaxminMode mode{"farthest-first selection", 0, "", false, upd_blocks(n)};
        mode.prepare = [](void *, const MaxminState &) { return hipSuccess; };
        mode.step = [=](uint32_t t, void *, double *, const MaxminState &S) { return enqueue_update(ctx, d_mat, n, n, t, 0, S); };
        return mode;
    });
}

int maxmin_mash(dvs_ctx *ctx, const MaxminArgs &a, const dvs_sketches *sk, uint32_t k, uint32_t sketch_size) {
    const uint32_t n = a.n;
    if (n > dvs_sketches_nseq(sk))
        return dvs_set_error(ctx, DVS_ERR_VALUE, "%u rows of a handle that holds %u", n, dvs_sketches_nseq(sk));
    if (n == 1) return maxmin_single(a);
    if (k == 0) return dvs_set_error(ctx, DVS_ERR_ZERODIV, "float division by zero");
    if (!dvs_sketches_dev(sk)) return dvs_set_error(ctx, DVS_ERR_ZERODIV, "division by zero");  // every sketch empty
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    return maxmin_run(ctx, a, [&](const MaxminState &S) {
        return stage_mode(ctx, dvs_mash_cross_stage(ctx, sk, nullptr, a.n_select, sk, nullptr, n, k, sketch_size, S.picks), n, true);
    });
}

int maxmin_euclidean(dvs_ctx *ctx, const MaxminArgs &a, const dvs_matrix *m) {
    const uint32_t n = a.n;
    if (int rc = matrix_check(ctx, m, n)) return rc;
    if ((n + EUC_THREADS / 64 - 1) / (EUC_THREADS / 64) > 65535u)  // (euclid_cross_kernel's grid, a workgroup per 8 rows in y)
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "%u rows: beyond the euclidean kernel's grid", n);
    if (n == 1) return maxmin_single(a);
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    return maxmin_run(ctx, a, [&](const MaxminState &S) {
        return stage_mode(ctx, dvs_euclid_cross_stage(ctx, m, nullptr, a.n_select, m, nullptr, n, S.picks), n, false);
    });
}

int maxmin_jsd(dvs_ctx *ctx, const MaxminArgs &a, const dvs_matrix *m) {
    const uint32_t n = a.n, n_select = a.n_select;
    if (int rc = matrix_check(ctx, m, n)) return rc;
    if (n == 1) return maxmin_single(a);
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->knobs.maxmin_jsd_cross)  // the A/B of DESIGN.md 4.13: the tile kernel on one query row, then the update
        return maxmin_run(ctx, a, [&](const MaxminState &) {
            MaxminMode mode{"jsd farthest-first selection (cross kernel)", (size_t(n) + n_select) * 8, "row entropies", true,
                            upd_blocks(n)};
            mode.prepare = [=](void *d_h, const MaxminState &) {
                return dvs_jsd_entropies_enqueue(ctx, m, nullptr, n, static_cast<double *>(d_h));
            };
            mode.step = [=](uint32_t t, void *d_h, double *d_row, const MaxminState &S) {
                double *h = static_cast<double *>(d_h), *hq = h + n;
                hipLaunchKernelGGL(maxmin_query_entropy_kernel, dim3(1), dim3(64), 0, ctx->stream, h, hq, t, S);
                hipError_t e = hipGetLastError();
                if (e == hipSuccess) e = dvs_jsd_cross_row_enqueue(ctx, m, S.picks, t, n, hq, h, d_row);
                if (e == hipSuccess) e = enqueue_update(ctx, d_row, 0, n, t, 0, S);
                return e;
            };
            return mode;
        });
    return maxmin_run(ctx, a, [&](const MaxminState &) {
        const uint32_t blocks = (n + MM_ROW_PAIRS - 1) / MM_ROW_PAIRS;
        MaxminMode mode{"jsd farthest-first selection", size_t(n) * 8, "row entropies", false, blocks};
        mode.prepare = [=](void *d_h, const MaxminState &) {
            return dvs_jsd_entropies_enqueue(ctx, m, nullptr, n, static_cast<double *>(d_h));
        };
        mode.step = [=](uint32_t t, void *d_h, double *, const MaxminState &S) {
            dvs_mat_dispatch(m, [&](auto *mp) {
                using T = std::remove_cv_t<std::remove_pointer_t<decltype(mp)>>;
                hipLaunchKernelGGL((jsd_row_kernel<T>), dim3(blocks), dim3(MM_ROW_THREADS), 0, ctx->stream, mp, m->d_totals, n,
                                   m->nbins, static_cast<const double *>(d_h), t, S);
                return 0;
            });
            return hipGetLastError();
        };
        return mode;
    });
}

}  // namespace

extern "C" int dvs_maxmin(dvs_ctx *ctx, const dvs_source *src, const uint32_t *seeds, uint32_t n_seeds, uint32_t n_select,
                          int use_min_distance, double min_distance, uint32_t *picks, double *radius, uint32_t *n_picked,
                          uint32_t *owner, double *dist_to_owner, double *cover) {
    if (int rc = dvs_source_check(ctx, src, src)) return rc;
    if (src->rows) return dvs_source_refuse(ctx, "dvs_maxmin", src, "a row list");
    const MaxminArgs a{src->n, seeds, n_seeds, n_select, use_min_distance, min_distance, picks, radius, n_picked, owner, dist_to_owner, cover};
    if (int rc = maxmin_check(ctx, a)) return rc;
    switch (src->kind) {
    case DVS_SRC_MASH: return maxmin_mash(ctx, a, dvs_src_sketches(src), src->k, src->sketch_size);
    case DVS_SRC_EUCLIDEAN: return maxmin_euclidean(ctx, a, dvs_src_matrix(src));
    case DVS_SRC_JSD: return maxmin_jsd(ctx, a, dvs_src_matrix(src));
    default: return maxmin_given(ctx, a, static_cast<const double *>(src->handle), src->on_device);
    }
}
