// k-medoids (PAM) over an n x n distance matrix on the device: include/dvs_hip.h "k-medoids" pins the algorithm,
// DESIGN.md 4.17 has the measurements.  No counterpart in the reference, whose selection is by delta-JSD (records.rs).
//
// The matrix is only READ.  Device pipeline (one stream; the launches of a batch of rounds are enqueued ahead and
// nothing is read back inside a batch; every seam is a launch boundary -- no grid barrier, no spinning, DESIGN.md 4.12
// item 3):
//   entry    kmed_score_kernel<KM_ROWSUM>: one pass that flags a non-finite or negative entry off the diagonal and
//            leaves every row's sum, which is BUILD's score for slot 0, and its largest entry, from which
//            kmed_noise_kernel takes the noise level of a Delta; kmed_pick_kernel ends the run on a flag
//   BUILD    per further slot: kmed_build_update_kernel (dn = min(dn, the new medoid's row)), kmed_score_kernel<KM_GAIN>,
//            kmed_pick_kernel
//   state    kmed_assign_kernel: per item the k cells D[med[l]][o] in slot order -> near, dn, ds;
//            kmed_sums_kernel: R[l] by one wave per slot in item order, td by one wave more
//   round    kmed_score_kernel<KM_SWAPK> (k <= 16: <KM_SWAPL>, k = 1: <KM_SWAP1>), the hot kernel: a wave per candidate row x streams
//            D[x][.] from HBM beside dn, ds and near (20 n bytes, L2-resident), keeps shared_x in registers and
//            C_x[0 .. k) in LDS and leaves the best (Delta, slot) of its row; kmed_pick_kernel reduces the rows by the
//            tie rule, decides stop or exchange and writes the status word and the exchange record; then the state
//            kernels again
//   A status word ends the search: every kernel of this file returns at once when it is set.  Between two batches
//   (DVS_KMEDOIDS_BATCH rounds, 8 by default) the host reads the status block.
//
// Every sum is added in a fixed order: a lane its strided terms in ascending order, the lanes by the xor-shuffle tree
// (whose two partners add the same two values, so every lane holds the same bits).  The adds into a bucket C_x[l] are
// ordered too: per chunk of 64 items, the distinct slots among the contributing lanes are taken in the order of their
// first lane, the terms of one slot summed by the same tree and added by lane 0; chunks run in ascending order (up to
// 16 medoids a lane keeps buckets of its own instead, which meet in one tree per slot at the end).  No floating-point
// atomic anywhere.
#include "dvs_internal.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr uint32_t KM_NONE = 0xFFFFFFFFu;
constexpr uint32_t KM_MAX_K = 1024;       // C_x[0 .. k) of a wave in LDS: 8 KB a wave at most
constexpr uint32_t KM_MAX_SWAPS = 65535;
constexpr uint32_t KM_BATCH = 8;          // DESIGN.md 4.17 has the other lengths' times
constexpr int KM_THREADS = 256;
constexpr uint32_t KM_WAVES = KM_THREADS / 64;
constexpr uint32_t KM_UNROLL = 8;         // chunks of 64 cells a wave has in flight
constexpr int KM_PICK_THREADS = 1024;
// the status block (device, uint32 [8])
enum { KM_ST_DONE = 0, KM_ST_NSWAPS = 1, KM_ST_BAD = 2, KM_ST_ZERODIV = 3, KM_ST_STOP = 4, KM_ST_NOCAND = 5 };
constexpr uint32_t KM_BAD_NONFINITE = 1, KM_BAD_NEGATIVE = 2;
enum { KM_ROWSUM = 0, KM_GAIN = 1, KM_SWAP1 = 2, KM_SWAPK = 3, KM_SWAPL = 4 };
constexpr uint32_t KM_LANE_K = 16;        // up to this k a lane keeps buckets of its own (KM_SWAPL): 8 KB a wave at most
enum { KM_PICK_CHECK = 0, KM_PICK_BUILD = 1, KM_PICK_SWAP = 2 };

struct KmedState {
    uint32_t *status;
    double *noise;      // [1] what a Delta may be off by (include/dvs_hip.h): 4 (n + 8) 2^-52 n d_max
    double *td_hist;    // [max_swaps + 1]
    double *dn, *ds;    // [n]
    double *R;          // [k]
    double *rec_v;      // [n] per candidate row: its score (the least is picked) ...
    uint32_t *rec_l;    // [n] ... and slot; KM_NONE: not a candidate
    uint32_t *med;      // [k]
    uint32_t *swaps;    // [2 max_swaps]
    uint32_t *near;     // [n]
    uint32_t *slot_of;  // [n] the slot an item is the medoid of, KM_NONE for the others
};

__device__ __forceinline__ double km_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the tie rule of a reduction: the lesser value, then the lower index; an entry without an index loses to any with one
__device__ __forceinline__ bool km_better(double v, uint32_t i, double bv, uint32_t bi) {
    return i != KM_NONE && (bi == KM_NONE || v < bv || (v == bv && i < bi));
}

// One pass over the matrix, a wave per row x (KM_WAVES rows a workgroup): the row's score by MODE.
//   KM_ROWSUM  sum_{o != x} D[x][o], every row; a non-finite or negative entry sets its bit in the status block
//   KM_GAIN    -(sum_o max(dn[o] - d, 0)) for a non-medoid x (the least is the largest gain)
//   KM_SWAP1   sum_o (d - dn[o]), k = 1
//   KM_SWAPK   min over l of (R[l] + C_x[l]) + shared_x, with that l; s_c holds C_x of the workgroup's waves
//   KM_SWAPL   the same for k <= KM_LANE_K, where most chunks hold several items of every slot and the ordered adds
//              of KM_SWAPK cost a shuffle tree per slot and chunk: every lane adds its own terms, in ascending item
//              order, into buckets of its own (s_c: [wave][slot][lane]), and the 64 buckets of a slot meet in one
//              tree at the end
// d = D[x][o], 0 for o = x (the diagonal is not read).
template <int MODE>
__global__ __launch_bounds__(KM_THREADS) void kmed_score_kernel(const double *__restrict__ D, uint32_t n, uint32_t k, KmedState S) {
    extern __shared__ double s_c[];
    if (S.status[KM_ST_DONE]) return;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t x = blockIdx.x * KM_WAVES + wave;
    const bool active = x < n && (MODE == KM_ROWSUM || S.slot_of[x] == KM_NONE);
    double *C = s_c + size_t(wave) * k;
    double *CL = s_c + size_t(wave) * k * 64 + lane;  // (KM_SWAPL: this lane's bucket of slot l is CL[l * 64])
    if (MODE == KM_SWAPK) {
        for (uint32_t l = lane; l < k; l += 64) C[l] = 0.0;
        __syncthreads();
    }
    if (MODE == KM_SWAPL)
        for (uint32_t l = 0; l < k; l++) CL[l * 64] = 0.0;
    double acc = 0.0, row_max = 0.0;
    uint32_t bad = 0;
    if (active) {
        const double *row = D + size_t(x) * n;
        for (uint32_t j0 = 0; j0 < n; j0 += 64 * KM_UNROLL) {
            double dv[KM_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < KM_UNROLL; u++) {
                const uint32_t j = j0 + u * 64 + lane;
                dv[u] = j < n && j != x ? row[j] : 0.0;
            }
#pragma unroll
            for (uint32_t u = 0; u < KM_UNROLL; u++) {
                const uint32_t j = j0 + u * 64 + lane;
                const bool valid = j < n;
                const double d = dv[u];
                if (MODE == KM_ROWSUM) {
                    if (!__builtin_isfinite(d)) bad |= KM_BAD_NONFINITE;
                    if (d < 0.0) bad |= KM_BAD_NEGATIVE;
                    acc += d;
                    row_max = d > row_max ? d : row_max;
                } else if (MODE == KM_GAIN) {
                    const double t = valid ? S.dn[j] - d : 0.0;
                    acc += t > 0.0 ? t : 0.0;
                } else if (MODE == KM_SWAP1) {
                    acc += valid ? d - S.dn[j] : 0.0;
                } else if (MODE == KM_SWAPL) {
                    const double dnj = valid ? S.dn[j] : 0.0, dsj = valid ? S.ds[j] : 0.0;
                    const double t = d - dnj;
                    acc += t < 0.0 ? t : 0.0;
                    if (valid && d < dsj) CL[S.near[j] * 64] += d < dnj ? dnj - dsj : d - dsj;
                } else {
                    const double dnj = valid ? S.dn[j] : 0.0, dsj = valid ? S.ds[j] : 0.0;
                    const uint32_t nj = valid ? S.near[j] : 0u;
                    const double t = d - dnj;
                    acc += t < 0.0 ? t : 0.0;
                    const bool contrib = valid && d < dsj;
                    const double c = d < dnj ? dnj - dsj : d - dsj;
                    uint64_t mask = __ballot(contrib);
                    while (mask) {  // (wave-uniform)
                        const int leader = __ffsll(static_cast<long long>(mask)) - 1;
                        const uint32_t slot = __shfl(nj, leader, 64);
                        const bool mine = contrib && nj == slot;
                        const uint64_t same = __ballot(mine);
                        // (one lane: the tree would add 63 zeros to its term, the same bits)
                        const double v = (same & (same - 1)) ? km_wave_sum(mine ? c : 0.0) : __shfl(c, leader, 64);
                        if (lane == 0) C[slot] += v;
                        mask &= ~same;
                    }
                }
            }
        }
    }
    if (MODE == KM_SWAPL) {  // (no lane has touched another's buckets: nothing to wait for)
        if (x >= n) return;
        if (!active) {
            if (lane == 0) S.rec_l[x] = KM_NONE;
            return;
        }
        const double shared = km_wave_sum(acc);
        double bv = 0.0;
        uint32_t bl = KM_NONE;
        for (uint32_t l = 0; l < k; l++) {
            const double v = (S.R[l] + km_wave_sum(CL[l * 64])) + shared;
            if (km_better(v, l, bv, bl)) {
                bv = v;
                bl = l;
            }
        }
        if (lane == 0) {
            S.rec_v[x] = bv;
            S.rec_l[x] = bl;
        }
        return;
    }
    if (MODE == KM_SWAPK) {
        __syncthreads();
        if (x >= n) return;
        if (!active) {
            if (lane == 0) S.rec_l[x] = KM_NONE;
            return;
        }
        const double shared = km_wave_sum(acc);
        double bv = 0.0;
        uint32_t bl = KM_NONE;
        for (uint32_t l = lane; l < k; l += 64) {
            const double v = (S.R[l] + C[l]) + shared;
            if (km_better(v, l, bv, bl)) {
                bv = v;
                bl = l;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o, 64);
            const uint32_t ol = __shfl_xor(bl, o, 64);
            if (km_better(ov, ol, bv, bl)) {
                bv = ov;
                bl = ol;
            }
        }
        if (lane == 0) {
            S.rec_v[x] = bv;
            S.rec_l[x] = bl;
        }
        return;
    }
    if (x >= n) return;
    if (MODE == KM_ROWSUM && bad) atomicOr(&S.status[KM_ST_BAD], bad);
    const double sum = km_wave_sum(acc);
    if (MODE == KM_ROWSUM) {  // the row's largest entry, where the second distances will be: nothing reads those yet
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double other = __shfl_xor(row_max, o, 64);
            row_max = other > row_max ? other : row_max;
        }
        if (lane == 0) S.ds[x] = row_max;
    }
    if (lane == 0) {
        S.rec_v[x] = MODE == KM_GAIN ? -sum : sum;
        S.rec_l[x] = active ? 0u : KM_NONE;
    }
}

// Behind the entry check, one workgroup: d_max, the largest entry off the diagonal, from the rows' maxima (a maximum
// is the same in every order) and with it the noise level of a Delta
__global__ __launch_bounds__(KM_PICK_THREADS) void kmed_noise_kernel(uint32_t n, KmedState S) {
    __shared__ double s_m[KM_PICK_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double m = 0.0;
    for (uint32_t c = tid; c < n; c += KM_PICK_THREADS) m = S.ds[c] > m ? S.ds[c] : m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(m, o, 64);
        m = other > m ? other : m;
    }
    if (lane == 0) s_m[wave] = m;
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < KM_PICK_THREADS / 64; w++) m = s_m[w] > m ? s_m[w] : m;
    S.noise[0] = 4.0 * (double(n) + 8.0) * double(n) * 0x1p-52 * m;
}

// no item a medoid yet
__global__ __launch_bounds__(KM_THREADS) void kmed_clear_kernel(uint32_t n, KmedState S) {
    const uint32_t j = blockIdx.x * KM_THREADS + threadIdx.x;
    if (j < n) S.slot_of[j] = KM_NONE;
}

// INIT_GIVEN: the caller's medoids (distinct and < n: kmedoids_check_args) marked
__global__ __launch_bounds__(KM_THREADS) void kmed_mark_kernel(uint32_t k, KmedState S) {
    const uint32_t l = blockIdx.x * KM_THREADS + threadIdx.x;
    if (l < k) S.slot_of[S.med[l]] = l;
}

// One workgroup behind a scoring pass: the rows' records reduced by the tie rule (the least score, the lowest x; the
// slot of a row is already its lowest) in a fixed tree, then by `mode`
//   KM_PICK_CHECK  nothing is picked (INIT_GIVEN behind the entry check)
//   KM_PICK_BUILD  med[t] = x
//   KM_PICK_SWAP   round t: no candidate or a Delta that is not below minus the noise level ends the search (stop =
//                  1), else med[l] = x and the exchange is recorded
// Behind the entry check (t == 0 of the first two modes) a flagged entry ends the run before anything is picked.
__global__ __launch_bounds__(KM_PICK_THREADS) void kmed_pick_kernel(uint32_t n, int mode, uint32_t t, KmedState S) {
    __shared__ double s_v[KM_PICK_THREADS / 64];
    __shared__ uint32_t s_x[KM_PICK_THREADS / 64];
    if (S.status[KM_ST_DONE]) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (mode != KM_PICK_SWAP && t == 0 && (S.status[KM_ST_BAD] || S.status[KM_ST_ZERODIV])) {
        if (tid == 0) S.status[KM_ST_DONE] = 1u;
        return;
    }
    if (mode == KM_PICK_CHECK) return;
    double bv = 0.0;
    uint32_t bx = KM_NONE;
    for (uint32_t c = tid; c < n; c += KM_PICK_THREADS) {
        const uint32_t xi = S.rec_l[c] != KM_NONE ? c : KM_NONE;
        const double v = xi != KM_NONE ? S.rec_v[c] : 0.0;
        if (km_better(v, xi, bv, bx)) {
            bv = v;
            bx = xi;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const uint32_t ox = __shfl_xor(bx, o, 64);
        if (km_better(ov, ox, bv, bx)) {
            bv = ov;
            bx = ox;
        }
    }
    if (lane == 0) {
        s_v[wave] = bv;
        s_x[wave] = bx;
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 1; w < KM_PICK_THREADS / 64; w++)
        if (km_better(s_v[w], s_x[w], bv, bx)) {
            bv = s_v[w];
            bx = s_x[w];
        }
    if (mode == KM_PICK_BUILD) {
        if (bx == KM_NONE) {  // (k <= n leaves a non-medoid for every slot: not reached)
            S.status[KM_ST_NOCAND] = 1u;
            S.status[KM_ST_DONE] = 1u;
            return;
        }
        S.med[t] = bx;
        S.slot_of[bx] = t;
        return;
    }
    if (bx == KM_NONE || !(bv < -S.noise[0])) {
        S.status[KM_ST_STOP] = 1u;
        S.status[KM_ST_DONE] = 1u;
        return;
    }
    const uint32_t l = S.rec_l[bx];
    S.slot_of[S.med[l]] = KM_NONE;
    S.med[l] = bx;
    S.slot_of[bx] = l;
    S.swaps[2 * size_t(t)] = bx;
    S.swaps[2 * size_t(t) + 1] = l;
    S.status[KM_ST_NSWAPS] = t + 1;
}

// BUILD, behind the pick of slot m: dn against the new medoid's row (first: there is no dn yet); a medoid's own is 0
__global__ __launch_bounds__(KM_THREADS) void kmed_build_update_kernel(const double *__restrict__ D, uint32_t n, uint32_t m,
                                                                       KmedState S) {
    if (S.status[KM_ST_DONE]) return;
    const uint32_t j = blockIdx.x * KM_THREADS + threadIdx.x;
    if (j >= n) return;
    if (S.slot_of[j] != KM_NONE) {
        S.dn[j] = 0.0;
        return;
    }
    const double d = D[size_t(S.med[m]) * n + j];
    const double old = m ? S.dn[j] : d;
    S.dn[j] = d < old ? d : old;
}

// The state from the k medoid rows: per item o the cells D[med[l]][o] in slot order (coalesced along each row), four
// in flight.
__global__ __launch_bounds__(KM_THREADS) void kmed_assign_kernel(const double *__restrict__ D, uint32_t n, uint32_t k, KmedState S) {
    __shared__ uint32_t s_med[KM_MAX_K];
    if (S.status[KM_ST_DONE]) return;
    for (uint32_t l = threadIdx.x; l < k; l += KM_THREADS) s_med[l] = S.med[l];
    __syncthreads();
    const uint32_t o = blockIdx.x * KM_THREADS + threadIdx.x;
    if (o >= n) return;
    const uint32_t own = S.slot_of[o];
    double b1 = __builtin_inf(), b2 = __builtin_inf();
    uint32_t nl = 0;
    for (uint32_t l0 = 0; l0 < k; l0 += 4) {
        double dv[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            const uint32_t l = l0 + u;
            dv[u] = l < k && l != own ? D[size_t(s_med[l]) * n + o] : 0.0;
        }
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            const uint32_t l = l0 + u;
            const double d = dv[u];
            if (l >= k || l == own) continue;
            if (own != KM_NONE) {
                b2 = d < b2 ? d : b2;
            } else if (d < b1) {
                b2 = b1;
                b1 = d;
                nl = l;
            } else if (d < b2) {
                b2 = d;
            }
        }
    }
    S.near[o] = own != KM_NONE ? own : nl;
    S.dn[o] = own != KM_NONE ? 0.0 : b1;
    S.ds[o] = b2;
}

// Behind the assign: workgroup l < n_r leaves R[l] = sum_{near[o] = l} (ds[o] - dn[o]), the last one td = sum dn, as
// entry [the exchanges so far] of the history.  A thread adds its strided items in ascending order, a wave by the
// tree, the waves in wave order.
__global__ __launch_bounds__(KM_THREADS) void kmed_sums_kernel(uint32_t n, uint32_t n_r, KmedState S) {
    __shared__ double s_w[KM_WAVES];
    if (S.status[KM_ST_DONE]) return;
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    double acc = 0.0;
    if (b < n_r) {
        for (uint32_t j = tid; j < n; j += KM_THREADS) acc += S.near[j] == b ? S.ds[j] - S.dn[j] : 0.0;
    } else {
        for (uint32_t j = tid; j < n; j += KM_THREADS) acc += S.dn[j];
    }
    acc = km_wave_sum(acc);
    if ((tid & 63) == 0) s_w[tid >> 6] = acc;
    __syncthreads();
    if (tid != 0) return;
    for (uint32_t w = 1; w < KM_WAVES; w++) acc += s_w[w];
    if (b < n_r) S.R[b] = acc;
    else S.td_hist[S.status[KM_ST_NSWAPS]] = acc;
}

size_t up8(size_t x) { return (x + 7) & ~size_t(7); }

// the state of a run, one allocation: offsets in bytes
struct KmedLayout {
    size_t status, noise, td_hist, dn, ds, R, rec_v, med, swaps, near, slot_of, rec_l, bytes;
    KmedLayout(uint32_t n, uint32_t k, uint32_t ms) {
        status = 0;                             // uint32 [8]
        noise = 32;                             // double [1]
        td_hist = 40;                           // double [ms + 1]
        dn = td_hist + (size_t(ms) + 1) * 8;    // double [n]
        ds = dn + size_t(n) * 8;                // double [n]
        R = ds + size_t(n) * 8;                 // double [k]
        rec_v = R + size_t(k) * 8;              // double [n]
        med = rec_v + size_t(n) * 8;            // uint32 [k]
        swaps = med + size_t(k) * 4;            // uint32 [2 ms]
        near = swaps + size_t(ms) * 8;          // uint32 [n]
        slot_of = near + size_t(n) * 4;         // uint32 [n]
        rec_l = slot_of + size_t(n) * 4;        // uint32 [n]
        bytes = up8(rec_l + size_t(n) * 4);
    }
};

uint32_t grid_of(uint32_t n, uint32_t per) { return (n + per - 1) / per; }

}  // namespace

// the arguments and n, before anything else is looked at
static int kmedoids_check_args(dvs_ctx *ctx, uint32_t n, const dvs_kmedoids_params *p, const uint32_t *medoids) {
    if (p->flags) return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_kmedoids: flags = %u: no flag is defined", p->flags);
    if (p->init != DVS_KMEDOIDS_INIT_BUILD && p->init != DVS_KMEDOIDS_INIT_GIVEN)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_kmedoids: unknown init %u", p->init);
    if (p->k == 0) return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_kmedoids: one medoid at least");
    if (n == 0) return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_kmedoids: no rows");
    if (p->k > n) return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_kmedoids: %u medoids of %u rows", p->k, n);
    if (p->k > KM_MAX_K)
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "dvs_kmedoids: %u medoids: %u at most (the accumulators of a candidate live in LDS)",
                             p->k, KM_MAX_K);
    if (p->max_swaps > KM_MAX_SWAPS)
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "dvs_kmedoids: max_swaps = %u: %u at most", p->max_swaps, KM_MAX_SWAPS);
    if (p->init == DVS_KMEDOIDS_INIT_GIVEN) {
        std::vector<bool> seen(n, false);
        for (uint32_t l = 0; l < p->k; l++) {
            if (medoids[l] >= n)
                return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_kmedoids: initial medoid %u is row %u of %u", l, medoids[l], n);
            if (seen[medoids[l]])
                return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_kmedoids: row %u is an initial medoid more than once", medoids[l]);
            seen[medoids[l]] = true;
        }
    }
    return DVS_OK;
}

// A consumer's run (dvs_internal.h dvs_square_consumer): k-medoids over the n x n matrix at d_dist (only read), enqueued
// on the context's stream behind whatever wrote the matrix.  Returns when the host outputs (dvs_kmedoids's) are written.
static int kmedoids_run(dvs_ctx *ctx, const double *d_dist, uint32_t n, const uint32_t *d_zerodiv,
                        const dvs_kmedoids_params *p, const dvs_kmedoids_out &out) {
    const uint32_t k = p->k, ms = p->max_swaps;
    const bool given = p->init == DVS_KMEDOIDS_INIT_GIVEN;
    const KmedLayout L(n, k, ms);
    PooledBuf d_state{ctx};
    if (int rc = dvs_dev_alloc(ctx, &d_state.p, L.bytes, "k-medoids state")) return rc;
    char *base = d_state.as<char>();
    auto f64 = [&](size_t off) { return reinterpret_cast<double *>(base + off); };
    auto u32 = [&](size_t off) { return reinterpret_cast<uint32_t *>(base + off); };
    const KmedState S{u32(L.status), f64(L.noise), f64(L.td_hist), f64(L.dn), f64(L.ds), f64(L.R), f64(L.rec_v), u32(L.rec_l), u32(L.med),
                      u32(L.swaps), u32(L.near), u32(L.slot_of)};
    const char *what = "k-medoids";
    const hipStream_t s = ctx->stream;
    const dim3 rows(grid_of(n, KM_WAVES)), items(grid_of(n, KM_THREADS)), thr(KM_THREADS);
    const uint32_t n_r = k >= 2 ? k : 0;

    // ---- the entry check, the initial medoids and their state
    hipError_t e = dvs_status_begin(ctx, S.status, 32, KM_ST_ZERODIV, d_zerodiv);
    if (e == hipSuccess && given) e = hipMemcpyAsync(S.med, out.medoids, size_t(k) * 4, hipMemcpyHostToDevice, s);
    auto assign = [&] {
        hipLaunchKernelGGL(kmed_assign_kernel, items, thr, 0, s, d_dist, n, k, S);
        hipLaunchKernelGGL(kmed_sums_kernel, dim3(n_r + 1), thr, 0, s, n, n_r, S);
    };
    if (e == hipSuccess) {
        hipLaunchKernelGGL(kmed_clear_kernel, items, thr, 0, s, n, S);
        if (given) hipLaunchKernelGGL(kmed_mark_kernel, dim3(grid_of(k, KM_THREADS)), thr, 0, s, k, S);
        hipLaunchKernelGGL(kmed_score_kernel<KM_ROWSUM>, rows, thr, 0, s, d_dist, n, k, S);
        hipLaunchKernelGGL(kmed_noise_kernel, dim3(1), dim3(KM_PICK_THREADS), 0, s, n, S);
        hipLaunchKernelGGL(kmed_pick_kernel, dim3(1), dim3(KM_PICK_THREADS), 0, s, n, given ? KM_PICK_CHECK : KM_PICK_BUILD, 0u, S);
        for (uint32_t m = 0; !given && m + 1 < k; m++) {
            hipLaunchKernelGGL(kmed_build_update_kernel, items, thr, 0, s, d_dist, n, m, S);
            hipLaunchKernelGGL(kmed_score_kernel<KM_GAIN>, rows, thr, 0, s, d_dist, n, k, S);
            hipLaunchKernelGGL(kmed_pick_kernel, dim3(1), dim3(KM_PICK_THREADS), 0, s, n, KM_PICK_BUILD, m + 1, S);
        }
        assign();
        e = hipGetLastError();
    }
    uint32_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(st, S.status, 32, hipMemcpyDeviceToHost, s);
    hipError_t se = hipStreamSynchronize(s);
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, what);
    if (se != hipSuccess) return dvs_hip_fail(ctx, se, what);
    if (st[KM_ST_ZERODIV]) return dvs_set_error(ctx, DVS_ERR_ZERODIV, "division by zero");  // 0 / 0, distance.py:283
    if (st[KM_ST_BAD] & KM_BAD_NONFINITE)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "Input contains NaN or infinity: the %u x %u distance matrix (dvs_kmedoids)", n, n);
    if (st[KM_ST_BAD] & KM_BAD_NEGATIVE)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "dvs_kmedoids: the %u x %u distance matrix has a negative entry", n, n);
    if (st[KM_ST_NOCAND]) return dvs_set_error(ctx, DVS_ERR_RUNTIME, "dvs_kmedoids: BUILD found no candidate");

    // ---- the swap phase: rounds enqueued a batch ahead
    const uint32_t batch = ctx->knobs.kmedoids_batch ? ctx->knobs.kmedoids_batch : KM_BATCH;
    const size_t lds = size_t(KM_WAVES) * k * 8 * (k <= KM_LANE_K ? 64 : 1);
    if (k == n) st[KM_ST_DONE] = st[KM_ST_STOP] = 1;  // every item a medoid: no candidate
    for (uint32_t t0 = 0; e == hipSuccess && se == hipSuccess && t0 < ms && !st[KM_ST_DONE];) {
        const uint32_t t1 = uint32_t(std::min<uint64_t>(uint64_t(t0) + batch, ms));
        for (uint32_t t = t0; t < t1; t++) {
            if (k > KM_LANE_K) hipLaunchKernelGGL(kmed_score_kernel<KM_SWAPK>, rows, thr, lds, s, d_dist, n, k, S);
            else if (k >= 2) hipLaunchKernelGGL(kmed_score_kernel<KM_SWAPL>, rows, thr, lds, s, d_dist, n, k, S);
            else hipLaunchKernelGGL(kmed_score_kernel<KM_SWAP1>, rows, thr, 0, s, d_dist, n, k, S);
            hipLaunchKernelGGL(kmed_pick_kernel, dim3(1), dim3(KM_PICK_THREADS), 0, s, n, KM_PICK_SWAP, t, S);
            assign();
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(st, S.status, 32, hipMemcpyDeviceToHost, s);
        se = hipStreamSynchronize(s);
        t0 = t1;
    }

    // ---- the results
    const uint32_t ns = std::min(st[KM_ST_NSWAPS], ms);
    std::vector<double> hist(size_t(ns) + 1);
    auto back = [&](void *dst, const void *src, size_t bytes) {
        if (e == hipSuccess && se == hipSuccess && dst && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s);
    };
    back(hist.data(), S.td_hist, hist.size() * 8);
    back(out.medoids, S.med, size_t(k) * 4);
    back(out.labels, S.near, size_t(n) * 4);
    back(out.dist, S.dn, size_t(n) * 8);
    back(out.second, S.ds, size_t(n) * 8);
    back(out.swaps, S.swaps, size_t(ns) * 8);
    if (se == hipSuccess) se = hipStreamSynchronize(s);
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, what);
    if (se != hipSuccess) return dvs_hip_fail(ctx, se, what);
    if (out.td) std::copy(hist.begin(), hist.end(), out.td);
    out.info->td_init = hist.front();
    out.info->td = hist.back();
    out.info->n_swaps = ns;
    out.info->stop = st[KM_ST_STOP];
    out.info->passes = 1 + (given ? 0 : k - 1) + ns + (st[KM_ST_STOP] && k < n ? 1 : 0);
    return DVS_OK;
}

// beside the matrix: the state.  A source of one row the library measures itself (not given) is answered at once: the
// one item its own medoid, there is no cell to compute or to check.
dvs_square_consumer dvs_kmedoids_consumer(dvs_ctx *ctx, uint32_t n, bool given, const dvs_kmedoids_params *p,
                                          const dvs_kmedoids_out &out) {
    dvs_square_consumer c{"dvs_kmedoids"};
    c.check = [=] { return kmedoids_check_args(ctx, n, p, out.medoids); };
    if (!given)
        c.early = [=] {
            if (n != 1) return false;
            out.medoids[0] = out.labels[0] = 0;
            out.dist[0] = 0.0;
            if (out.second) out.second[0] = HUGE_VAL;
            if (out.td) out.td[0] = 0.0;
            *out.info = dvs_kmedoids_info{0.0, 0.0, 0, 1, 1};
            return true;
        };
    c.extra_bytes = [=] { return KmedLayout(n, p->k, p->max_swaps).bytes; };
    snprintf(c.extra_what, sizeof c.extra_what, "the state of %u medoids", p->k);
    c.writes_matrix = false;
    c.run = [=](double *d_dist, const uint32_t *d_zerodiv) { return kmedoids_run(ctx, d_dist, n, d_zerodiv, p, out); };
    return c;
}
