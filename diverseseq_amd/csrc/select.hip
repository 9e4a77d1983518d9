// Greedy delta-JSD selection over the N x B count matrix, entirely on the GPU.
//
// Replaces SummedRecords and the selectors of the reference (src/records.rs):
//   delta_jsd :70-84, increases_jsd :86-92, drop_lowest :94-109, replace_lowest
//   :111-118, push :120-147, stats :153-172, clone :182-189 (= new, :27-68),
//   get_lowest_record_index :220-252, updated_mean_freqs :276-286,
//   select_nmost_divergent :311-342, select_max_divergent :390-454 and the
//   *_final merges :363-382 / :456-507.
//
// The reference walks the candidates one by one; candidate i is tested against
// the set as modified by every accepted j < i.  Here a WINDOW of candidates is
// scored in parallel against the current state (scan_kernel, the HBM-bound hot
// kernel: one wavefront per 4^k-bin row), the FIRST position whose score clears
// the threshold is the only one acted on, and the scan restarts right after it:
// every candidate before it was rejected under exactly the state the sequential
// code would have used, so the selected ids are the reference's.  The state
// update (resolve -> leave-one-out -> finalize kernels) runs on the device too;
// the cursor, window and event live in device memory, so the host enqueues
// launch batches blindly and only polls the control block between batches.
//
// Decisions the device cannot separate from the reference's own rounding noise
// (|jsd - threshold| <= band, band ~ 4 B eps H) are handed to the host tie
// arbiter (exact_set.cpp), which replays the event log in the reference's exact
// f64 operation order.
//
// This file is the scan and state kernels and the host driver.  The persistent engine (persist.hip), the stepwise
// mode (stepwise.hip) and the MODE_MAX batch pair (maxbatch.hip) are files of their own behind select.h.
#include "dvs_internal.h"
#include "select.h"
#include "select_dev.h"

#include <algorithm>
#include <chrono>
#include <type_traits>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <memory>

namespace {

constexpr int SCAN_THREADS = 512;   // 8 waves share one LDS copy of the state vector

// Hot row loop of one wave: identity order, unique ids, B a multiple of 256 * SCAN_CH
// bins.  A row is consumed in batches of SCAN_CH chunks of 1 KiB per wave instruction,
// each batch requested in one burst before any of it is consumed.
template <typename T>
__device__ __forceinline__ void scan_rows_hot(SelCtl *ctl, const T *__restrict__ mat,
                                              const uint32_t *__restrict__ totals,
                                              const double *__restrict__ rowH, const double *bvec,
                                              uint64_t B, const ScanState &st, uint64_t first,
                                              uint64_t stride, uint32_t lane, uint32_t &nread,
                                              uint32_t &nprecise) {
    for (uint64_t r = first; r < st.nrows; r += stride) {
        const uint64_t p = st.cursor + r;
        const T *rp = mat + p * B;
        // the event word and the row's total / entropy in one round trip
        const unsigned long long ev =
            __hip_atomic_load(&ctl->event_pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t tot = totals[p];
        const double hrow = rowH[p];
        if (ev < p) break;       // an earlier event already ends this window: later rows are void
        if (tot == 0) continue;  // "No valid k-mers": skipped (src/records.rs:332-335)
        const double rinv = 1.0 / (double(tot) * st.dsize);
        const double mean_entropy = (st.he_base + hrow) / st.dsize;
        nread++;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, xmin = 0.0;
        for (uint64_t i0 = 0; i0 < B; i0 += 256 * SCAN_CH) {
            // SCAN_CH chunks (1 KiB per wave instruction each) requested before any is consumed
            Raw4<T> raw[SCAN_CH];
#pragma unroll
            for (int j = 0; j < SCAN_CH; j++) raw[j].load(rp + i0 + uint64_t(j) * 256 + lane * 4);
#pragma unroll
            for (int j = 0; j < SCAN_CH; j++) {
                const uint64_t i = i0 + uint64_t(j) * 256 + lane * 4;
                const double2 b01 = *reinterpret_cast<const double2 *>(bvec + i);
                const double2 b23 = *reinterpret_cast<const double2 *>(bvec + i + 2);
                double v0, v1, v2, v3;
                raw[j].get(v0, v1, v2, v3);
                fast4(b01, b23, v0, v1, v2, v3, rinv, a0, a1, a2, a3, xmin);
            }
        }
        const double hf = dvs_wave_sum((a0 + a1) + (a2 + a3));
        const double mn = dvs_wave_min(xmin);
        // a negative bin is NaN in the reference (rejected); else compare with margin
        const double jf = hf - mean_entropy;
        if (!(mn < 0.0) && jf > st.thr_fast) {
            bool hit = jf > st.thr_sure;  // above the threshold by more than the fast tier's error
            if (!hit) {                   // only the +-FAST_BAND zone pays for the f64 tier
                nprecise++;
                hit = precise_row(rp, bvec, B, rinv, mean_entropy, st.thr_lo, lane);
            }
            if (hit && lane == 0) atomicMin(&ctl->event_pos, (unsigned long long)p);
        }
    }
}

// General row loop (explicit order / labels, any B): correctness first.
template <typename T>
__device__ __forceinline__ void scan_rows_general(SelCtl *ctl, const T *__restrict__ mat,
                                               const uint32_t *__restrict__ totals,
                                               const double *__restrict__ rowH,
                                               const uint32_t *__restrict__ order,
                                               const uint32_t *__restrict__ labels,
                                               const uint8_t *__restrict__ inset, uint32_t nlabels,
                                               const double *bvec, uint64_t B, const ScanState &st,
                                               uint64_t first, uint64_t stride, uint32_t lane,
                                               uint32_t &nread, uint32_t &nprecise) {
    for (uint64_t r = first; r < st.nrows; r += stride) {
        const uint64_t p = st.cursor + r;
        if (__hip_atomic_load(&ctl->event_pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < p) break;
        const uint32_t row = order ? order[p] : uint32_t(p);
        if (row == DVS_ROW_REMOTE) continue;  // another rank scores this position
        const uint32_t tot = totals[row];
        if (tot == 0) continue;
        if (labels) {  // ids can only repeat when the caller passed labels (records.rs:87-89)
            const uint32_t lab = labels[p];
            if (lab < nlabels && inset[lab]) continue;
        }
        const T *rp = mat + uint64_t(row) * B;
        const double rinv = 1.0 / (double(tot) * st.dsize);
        const double mean_entropy = (st.he_base + rowH[row]) / st.dsize;
        nread++;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, xmin = 0.0;
        if ((B & 255) == 0) {
            for (uint64_t i0 = 0; i0 < B; i0 += 256) {
                const uint64_t i = i0 + lane * 4;
                double v0, v1, v2, v3;
                load4(rp, i, v0, v1, v2, v3);
                const double2 b01 = *reinterpret_cast<const double2 *>(bvec + i);
                const double2 b23 = *reinterpret_cast<const double2 *>(bvec + i + 2);
                fast4(b01, b23, v0, v1, v2, v3, rinv, a0, a1, a2, a3, xmin);
            }
        } else {
            for (uint64_t i = lane; i < B; i += 64) {
                const double x = fma(row_value(rp, i), rinv, bvec[i]);
                a0 += fast_neg_xlog2x(x);
                xmin = fmin(xmin, x);
            }
        }
        const double hf = dvs_wave_sum((a0 + a1) + (a2 + a3));
        const double mn = dvs_wave_min(xmin);
        if (mn < 0.0) continue;
        const double jf = hf - mean_entropy;
        if (!(jf > st.thr_fast)) continue;
        bool hit = jf > st.thr_sure;
        if (!hit) {
            nprecise++;
            hit = precise_row(rp, bvec, B, rinv, mean_entropy, st.thr_lo, lane);
        }
        if (hit && lane == 0) atomicMin(&ctl->event_pos, (unsigned long long)p);
    }
}

// HOT: identity order, unique ids, B a multiple of 256 * SCAN_CH (host-checked)
template <typename T, bool HOT>
__device__ __forceinline__ void scan_body(
    SelCtl *__restrict__ ctl, const T *__restrict__ mat, const uint32_t *__restrict__ totals,
    const double *__restrict__ rowH, const uint32_t *__restrict__ order,
    const uint32_t *__restrict__ labels, const uint8_t *__restrict__ inset, uint32_t nlabels,
    const double *__restrict__ base, uint32_t *__restrict__ wg_rows, uint64_t B, int base_in_lds,
    unsigned char *smem) {
    uint32_t *s_rows = reinterpret_cast<uint32_t *>(smem);  // 16 B header
    double *sb = reinterpret_cast<double *>(smem + 16);
    if (ctl->status != SEL_RUN) return;
    ScanState st;
    st.cursor = ctl->cursor;
    const uint64_t end = umin64(st.cursor + uint64_t(ctl->window), ctl->npos);
    if (st.cursor >= end) return;
    st.nrows = end - st.cursor;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t wpb = SCAN_THREADS / 64;
    if (uint64_t(blockIdx.x) * wpb >= st.nrows) return;  // whole workgroup idle
    st.thr_lo = ctl->thr - ctl->band;
    st.thr_fast = st.thr_lo - FAST_BAND;
    st.thr_sure = ctl->thr + ctl->band + FAST_BAND;
    st.he_base = ctl->he_base;
    st.dsize = double(ctl->size);
    const double *bvec = base;
    if (threadIdx.x < 2) s_rows[threadIdx.x] = 0;
    if (base_in_lds) {
        if ((B & 1) == 0) {
            const double2 *s2 = reinterpret_cast<const double2 *>(base);
            double2 *d2 = reinterpret_cast<double2 *>(sb);
            for (uint64_t i = threadIdx.x; i < B / 2; i += SCAN_THREADS) d2[i] = s2[i];
        } else {
            for (uint64_t i = threadIdx.x; i < B; i += SCAN_THREADS) sb[i] = base[i];
        }
        bvec = sb;
    }
    __syncthreads();
    const uint64_t first = uint64_t(blockIdx.x) * wpb + wave;
    const uint64_t stride = uint64_t(gridDim.x) * wpb;
    uint32_t nread = 0, nprecise = 0;
    if (HOT)
        scan_rows_hot<T>(ctl, mat, totals, rowH, bvec, B, st, first, stride, lane, nread, nprecise);
    else
        scan_rows_general<T>(ctl, mat, totals, rowH, order, labels, inset, nlabels, bvec, B, st, first,
                             stride, lane, nread, nprecise);
    if (lane == 0 && nread) {
        atomicAdd(&s_rows[0], nread);
        if (nprecise) atomicAdd(&s_rows[1], nprecise);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_rows[0]) {  // summed + cleared by resolve
        wg_rows[2 * blockIdx.x] = s_rows[0];
        wg_rows[2 * blockIdx.x + 1] = s_rows[1];
    }
}

template <typename T, bool HOT>
__global__ __launch_bounds__(SCAN_THREADS, 4) void scan_kernel(
    SelCtl *__restrict__ ctl, const T *__restrict__ mat, const uint32_t *__restrict__ totals,
    const double *__restrict__ rowH, const uint32_t *__restrict__ order,
    const uint32_t *__restrict__ labels, const uint8_t *__restrict__ inset, uint32_t nlabels,
    const double *__restrict__ base, uint32_t *__restrict__ wg_rows, uint64_t B, int base_in_lds) {
    // all LDS in the dynamic region (a static __shared__ in front of it would shift its
    // base off 16 B and every ds_read_b128 of the state vector would be replayed)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    scan_body<T, HOT>(ctl, mat, totals, rowH, order, labels, inset, nlabels, base, wg_rows, B, base_in_lds,
                      smem);
}

// ------------------------------------------------------------- state kernels
// JSD of the set with `lowest` swapped for the candidate in d.cand
// (src/records.rs:70-84), all threads of the block get the result.
// *h_out: the entropy of that mean vector; *clamped: some bin of S - lowest is one drop_lowest
// would clamp to zero (records.rs:100-105) -- when none is, the vector is bit for bit the one
// replace_lowest leaves in S / size, so an accept need not evaluate its entropy again.
__device__ double block_delta_jsd(const SelDev &d, const SelCtl *ctl, double cand_H,
                                  double *scratch, double *sum_out, double *h_out, int *clamped) {
    const uint32_t low_slot = d.ord[ctl->lowest];
    const double *low = d.M + uint64_t(low_slot) * d.B;
    const double dsize = double(ctl->size);
    Ent e;
    int cl = 0;
    for (uint64_t i = threadIdx.x; i < d.B; i += blockDim.x) {
        const double v = d.S[i] - low[i];
        cl |= (v <= DVS_EPS && v != 0.0) ? 1 : 0;
        e.add((v + d.cand[i]) / dsize);
    }
    double h = e.h, mn = e.mn, sm = e.sum;
    block_red3(h, mn, sm, scratch);
    *clamped = __syncthreads_or(cl);
    *h_out = (mn < 0.0) ? NAN : h;
    if (sum_out) *sum_out = sm;
    const double mean_entropy = (ctl->sum_entropy - d.mH[low_slot] + cand_H) / dsize;
    return (mn < 0.0) ? NAN : h - mean_entropy;
}

// H(vec / div) over the block, plus sum for the tolerance check
__device__ double block_entropy_div(const double *vec, double div, uint64_t B, double *scratch,
                                    double *sum_out) {
    Ent e;
    for (uint64_t i = threadIdx.x; i < B; i += blockDim.x) e.add(vec[i] / div);
    double h = e.h, mn = e.mn, sm = e.sum;
    block_red3(h, mn, sm, scratch);
    if (sum_out) *sum_out = sm;
    return (mn < 0.0) ? NAN : h;
}


template <typename T>
__device__ void resolve_body(SelDev &d, const T *__restrict__ mat, double *scratch, int &s_action) {
    SelCtl *ctl = d.ctl;
    if (ctl->status != SEL_RUN) return;
    const int tid = threadIdx.x;
    const uint32_t WIDE = blockDim.x;
    const double *ext_row = nullptr, *ext_H = nullptr;
    unsigned long long gathered_p = SEL_NONE;
    // (stepwise re-entry behind the arbiter: the candidate is the one resolve stopped at, still in d.cand --
    // the gathered slots are not looked at: the caller's buffer may have been reused since the step's apply)
    const bool reentry = d.gather_all && (ctl->forced == FORCE_ACCEPT || ctl->forced == FORCE_REJECT);
    if (d.gather_all && !reentry) {
        // stepwise mode: the earliest event among the gathered slots ([pos, H, row]) is this step's
        // event on every rank
        __shared__ int s_best;
        if (tid == 0) {
            int best = -1;
            double bp = 0.0;
            const uint64_t stride = d.B + 2;
            for (uint32_t r = 0; r < d.gather_world; r++) {
                const double q = d.gather_all[uint64_t(r) * stride];
                if (q >= 0.0 && (best < 0 || q < bp)) {
                    best = int(r);
                    bp = q;
                }
            }
            s_best = best;
            ctl->event_pos = best < 0 ? SEL_NONE : (unsigned long long)bp;
        }
        __syncthreads();
        const double *src = d.gather_all + uint64_t(s_best < 0 ? 0 : s_best) * (d.B + 2);
        ext_row = src + 2;
        ext_H = src + 1;
        gathered_p = s_best < 0 ? SEL_NONE : (unsigned long long)src[0];
    }
    const uint64_t p = reentry ? ctl->arb_pos : d.gather_all ? gathered_p : ctl->event_pos;
    if (reentry && tid == 0) ctl->event_pos = p;
    if (ctl->ev_kind != 0) return;  // a finalize is pending (arbiter re-entry)
    if (p == SEL_NONE) {
        if (tid == 0) {
            const uint64_t end = umin64(ctl->cursor + uint64_t(ctl->window), ctl->npos);
            ctl->n_windows++;
            ctl->cursor = end;
            ctl->mb_stuck = 0;
            if (end >= ctl->npos) ctl->status = SEL_DONE;
            ctl_next_window(ctl);
        }
        return;
    }
    const uint32_t row = d.order ? d.order[p] : uint32_t(p);
    uint32_t lab;
    double cand_H;
    if (reentry) {
        lab = (row == DVS_ROW_REMOTE) ? DVS_ROW_REMOTE : (d.labels ? d.labels[p] : row);
        cand_H = ctl->arb_H;
    } else if (ext_row) {  // exchanged candidate (its row may live on another rank)
        lab = (row == DVS_ROW_REMOTE) ? DVS_ROW_REMOTE : (d.labels ? d.labels[p] : row);
        cand_H = *ext_H;
        for (uint64_t i = tid; i < d.B; i += WIDE) d.cand[i] = ext_row[i];
    } else {
        lab = d.labels ? d.labels[p] : row;
        const double tot = double(d.totals[row]);
        cand_H = d.rowH[row];
        const T *rp = mat + uint64_t(row) * d.B;
        for (uint64_t i = tid; i < d.B; i += WIDE) d.cand[i] = cand_freq(rp, i, tot);
    }
    __syncthreads();
    double sm;
    double h_swapped;
    int any_clamped;
    const double jsd = block_delta_jsd(d, ctl, cand_H, scratch, &sm, &h_swapped, &any_clamped);
    if (tid == 0) {
        int action;
        const uint32_t forced = ctl->forced;
        if (forced == FORCE_ACCEPT || forced == FORCE_REJECT) {
            action = forced == FORCE_ACCEPT ? 1 : 0;
            ctl->forced = FORCE_NONE;
        } else if (sum_risky(sm, d.B) || fabs(jsd - ctl->thr) <= ctl->band) {
            ctl->status = SEL_ARBITER;
            ctl->arb_stage = ARB_RESOLVE;
            ctl->arb_pos = p;
            ctl->arb_H = cand_H;
            action = 3;
        } else {
            action = (jsd > ctl->thr) ? 1 : 0;  // NaN -> reject (records.rs:91)
        }
        if (action == 1 && ctl->mode == DVS_MODE_MAX && ctl->size < ctl->max_size) action = 2;
        if (action != 3) {
            ctl->n_windows++;
            ctl->n_events++;
            ctl->cursor = p + 1;
            ctl->event_pos = SEL_NONE;
            ctl->last_jsd = jsd;
            if (action == 0) ctl->mb_stuck = 0;  // (rejected: the row a batch stopped at is behind the cursor now)
            if (action == 0 && ctl->cursor >= ctl->npos) ctl->status = SEL_DONE;
        }
        s_action = action;
    }
    __syncthreads();
    const int action = s_action;
    if (action == 0 || action == 3) return;

    if (action == 1) {
        // replace_lowest = drop_lowest (records.rs:94-109) + push (:120-147)
        const uint32_t li = ctl->lowest, n = ctl->size;
        const uint32_t s = d.ord[li];
        double *mrow = d.M + uint64_t(s) * d.B;
        const uint32_t log_at = ctl->n_logged;  // (read by every thread before thread 0 moves it on, below)
        double *logrow = d.rowlog ? d.rowlog + uint64_t(log_at % d.rowlog_cap) * d.B : nullptr;  // (a ring: the host drains it at every poll)
        __syncthreads();
        if (tid == 0) ctl->s_is_resum = 0;
        for (uint64_t i = tid; i < d.B; i += WIDE) {
            double v = d.S[i] - mrow[i];
            if (v <= DVS_EPS) v = 0.0;
            const double f = d.cand[i];
            d.S[i] = v + f;
            mrow[i] = f;
            if (logrow) logrow[i] = f;
        }
        __syncthreads();
        if (tid == 0) {
            double sh = ctl->sum_entropy - d.mH[s];
            sh += cand_H;
            ctl->sum_entropy = sh;
            const uint32_t old_lab = d.mLabel[s];
            if (old_lab < d.nlabels) d.inset[old_lab] = 0;
            if (lab < d.nlabels) d.inset[lab] = 1;
            d.mH[s] = cand_H;
            d.mLabel[s] = lab;
            d.mPos[s] = p;
            ctl->n_accepts++;
            d.evlog_pos[ctl->n_logged] = p;
            d.evlog_kind[ctl->n_logged] = 1;
            ctl->n_logged++;
        }
        // Vec::remove(li) + push: the member order moves up by one from li, a block-wide chunk at a
        // time (read, barrier, write; thread 0 doing it alone was a chain of n dependent round trips)
        for (uint32_t b0 = li; b0 + 1 < n; b0 += WIDE) {
            const uint32_t i = b0 + tid;
            const uint32_t o = (i + 1 < n) ? d.ord[i + 1] : 0u;
            __syncthreads();
            if (i + 1 < n) d.ord[i] = o;
        }
        if (tid == 0) d.ord[n - 1] = s;  // (slot n-1 is read by no chunk after the one that wrote n-2)
        __syncthreads();
        // H(S / n) of the new set: what delta_jsd evaluated, unless drop_lowest's clamp changed a bin
        double sm2 = sm, hm = h_swapped;
        if (any_clamped) hm = block_entropy_div(d.S, double(n), d.B, scratch, &sm2);
        if (tid == 0) {
            ctl->total_jsd = hm - ctl->sum_entropy / double(n);
            ctl->ev_kind = 1;
            ctl->ev_n = n;
            if (sum_risky(sm2, d.B) || !(hm == hm)) ctl->ev_risky = 1;
        }
    } else {
        // MODE_MAX with room: clone (= new over the members, records.rs:27-68,182-189)
        // then push the candidate; kept only if the stat rises (finalize decides)
        // The clone's sums are the members' rows (entropies) added up in member order.  While the
        // set has only grown by pushes -- the rule in this mode until max_size is reached, after
        // which nothing is cloned any more -- the running S / sum_entropy ARE those sums, bit for
        // bit: rebuild_kernel formed them in member order and every kept push appended its
        // candidate at the end of both the order and the addition chain.
        const uint32_t n = ctl->size;
        const bool resum = ctl->s_is_resum == 0;
        double *mrow = d.M + uint64_t(n) * d.B;  // slot n is free
        for (uint64_t i = tid; i < d.B; i += WIDE) {
            double acc;
            if (resum) {
                acc = 0.0;
                for (uint32_t r = 0; r < n; r++) acc += d.M[uint64_t(d.ord[r]) * d.B + i];
            } else {
                acc = d.S[i];
            }
            const double f = d.cand[i];
            d.Stmp[i] = acc + f;
            mrow[i] = f;
        }
        if (tid == 0) {
            double sh;
            if (resum) {
                sh = 0.0;
                for (uint32_t r = 0; r < n; r++) sh += d.mH[d.ord[r]];
            } else {
                sh = ctl->sum_entropy;
            }
            sh += cand_H;
            ctl->t_sum_entropy = sh;
            d.mH[n] = cand_H;
            d.mLabel[n] = lab;
            d.mPos[n] = p;
        }
        __syncthreads();
        double sm2;
        const double hm = block_entropy_div(d.Stmp, double(n + 1), d.B, scratch, &sm2);
        if (tid == 0) {
            ctl->t_total_jsd = hm - ctl->t_sum_entropy / double(n + 1);
            ctl->ev_kind = 2;
            ctl->ev_n = n + 1;
            if (sum_risky(sm2, d.B) || !(hm == hm)) ctl->ev_risky = 1;
        }
    }
}

// Initial set: S = sum of the member rows in member order, sumH likewise,
// total_jsd (SummedRecords::new, records.rs:36-47).  Members were written by
// seed_kernel.  Two launches: the sum bin by bin over the whole grid (every bin's adds in member order; as
// part of the one-block kernel below it was 0.5 ms at 4^7 bins and 100 members -- one CU pulling 12.8 MB),
// then one block for the entropy of the sum, whose order of additions is the block's.
constexpr int RSUM_THREADS = 256;
__global__ __launch_bounds__(RSUM_THREADS) void rebuild_sum_kernel(SelDev d) {
    __shared__ uint32_t s_ord[RSUM_THREADS];
    const uint32_t n = d.ctl->size;
    const uint64_t i = uint64_t(blockIdx.x) * RSUM_THREADS + threadIdx.x;
    double acc = 0.0;
    for (uint32_t base = 0; base < n; base += RSUM_THREADS) {
        const uint32_t cnt = n - base < RSUM_THREADS ? n - base : RSUM_THREADS;
        __syncthreads();
        if (threadIdx.x < cnt) s_ord[threadIdx.x] = d.ord[base + threadIdx.x];
        __syncthreads();
        if (i < d.B) {
            uint32_t r = 0;
            for (; r + 8 <= cnt; r += 8) {  // eight rows requested together, added in member order
                double v[8];
#pragma unroll
                for (int q = 0; q < 8; q++) v[q] = d.M[uint64_t(s_ord[r + q]) * d.B + i];
#pragma unroll
                for (int q = 0; q < 8; q++) acc += v[q];
            }
            for (; r < cnt; r++) acc += d.M[uint64_t(s_ord[r]) * d.B + i];
        }
    }
    if (i < d.B) d.S[i] = acc;
}

__global__ __launch_bounds__(WIDE_THREADS) void rebuild_kernel(SelDev d) {
    __shared__ double scratch[48];
    // the members' entropies go through LDS first: read straight from global memory thread 0's whole
    // entropy sum is a chain of dependent round trips
    __shared__ double s_mh[WIDE_THREADS];
    SelCtl *ctl = d.ctl;
    const uint32_t n = ctl->size;
    double sh = 0.0;  // (thread 0's, in member order)
    for (uint32_t base = 0; base < n; base += WIDE_THREADS) {
        const uint32_t cnt = n - base < WIDE_THREADS ? n - base : WIDE_THREADS;
        __syncthreads();
        if (threadIdx.x < cnt) s_mh[threadIdx.x] = d.mH[d.ord[base + threadIdx.x]];
        __syncthreads();
        if (threadIdx.x == 0)
            for (uint32_t r = 0; r < cnt; r++) sh += s_mh[r];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ctl->sum_entropy = sh;
        ctl->s_is_resum = 1;
    }
    __syncthreads();
    double sm;
    const double hm = block_entropy_div(d.S, double(n), d.B, scratch, &sm);
    if (threadIdx.x == 0) {
        ctl->total_jsd = hm - ctl->sum_entropy / double(n);
        ctl->ev_kind = 1;
        ctl->ev_n = n;
        if (sum_risky(sm, d.B) || !(hm == hm)) ctl->ev_risky = 1;
    }
}

// member j <- matrix row of stream position seed_pos[j]
template <typename T>
__global__ __launch_bounds__(LOO_THREADS) void seed_kernel(SelDev d, const T *__restrict__ mat,
                                                         const uint64_t *__restrict__ seed_pos) {
    const uint32_t j = blockIdx.x;
    const uint64_t p = seed_pos[j];
    const uint32_t row = d.order ? d.order[p] : uint32_t(p);
    const uint32_t lab = d.labels ? d.labels[p] : row;
    const double tot = double(d.totals[row]);
    const T *rp = mat + uint64_t(row) * d.B;
    double *mrow = d.M + uint64_t(j) * d.B;
    for (uint64_t i = threadIdx.x; i < d.B; i += LOO_THREADS) mrow[i] = cand_freq(rp, i, tot);
    if (threadIdx.x == 0) {
        d.ord[j] = j;
        d.mH[j] = d.rowH[row];
        d.mLabel[j] = lab;
        d.mPos[j] = p;
        if (lab < d.nlabels) d.inset[lab] = 1;
    }
}

// Leave-one-out pass (get_lowest_record_index, records.rs:220-252): block r
// computes delta_jsd of the r-th member of the (possibly tentative) set.
__device__ void loo_body(const SelDev &d, uint32_t r, double *scratch) {
    const SelCtl *ctl = d.ctl;
    const uint32_t kind = ctl->ev_kind;
    if (kind == 0 || ctl->status != SEL_RUN) return;
    const uint32_t n = ctl->ev_n;
    if (r >= n) return;
    const bool tent = kind == 2;
    const uint32_t slot = (tent && r == n - 1) ? n - 1 : d.ord[r];
    const double *Sv = tent ? d.Stmp : d.S;
    const double sumH = tent ? ctl->t_sum_entropy : ctl->sum_entropy;
    const double tj = tent ? ctl->t_total_jsd : ctl->total_jsd;
    const double div = double(n) - 1.0;
    const double *mrow = d.M + uint64_t(slot) * d.B;
    Ent e;
    for (uint64_t i = threadIdx.x; i < d.B; i += blockDim.x) {
        double v = (Sv[i] - mrow[i]) / div;  // updated_mean_freqs, records.rs:276-286
        if (v <= DVS_EPS) v = 0.0;
        e.add(v);
    }
    double h = e.h, mnz = 0.0, sm = e.sum;
    block_red3(h, mnz, sm, scratch);
    if (threadIdx.x == 0) {
        const double mean_entropy = (sumH - d.mH[slot]) / div;
        const double jsd = h - mean_entropy;
        d.dtmp[r] = tj - jsd;
        d.dsum[r] = sm;
    }
}

// argmin / stats / commit-or-rollback / next scan state.  One block.
__device__ void finalize_body(SelDev &d, double *scratch, int &s_go) {
    SelCtl *ctl = d.ctl;
    const uint32_t kind = ctl->ev_kind;
    if (kind == 0 || ctl->status != SEL_RUN) return;
    const int tid = threadIdx.x;
    const uint32_t WIDE = blockDim.x;
    const uint32_t n = ctl->ev_n;

    // argmin with strict '<' from 1e6, earliest index on ties (records.rs:231,246-249);
    // NaN never wins a '<'.  Three fixed-tree reductions: min value, its first
    // index, and the runner-up (for the ambiguity check).
    bool risky = false;
    double best = 1e6;
    for (uint32_t r = tid; r < n; r += WIDE) {
        const double v = d.dtmp[r];
        if (sum_risky(d.dsum[r], d.B)) risky = true;
        if (v < best) best = v;
    }
    const double dmin = dvs_block_min(best, scratch);
    double fi = 4294967295.0;
    for (uint32_t r = tid; r < n; r += WIDE)
        if (dmin < 1e6 && d.dtmp[r] == dmin) fi = fmin(fi, double(r));
    const double dfirst = dvs_block_min(fi, scratch);
    uint32_t lowest = (dfirst < 4294967295.0) ? uint32_t(dfirst) : 0u;  // nothing below 1e6 -> 0
    double second = 1e6;
    for (uint32_t r = tid; r < n; r += WIDE) {
        const double v = d.dtmp[r];
        if (r != lowest && v < second) second = v;
    }
    const double dsecond = dvs_block_min(second, scratch);
    const int any_risky = __syncthreads_or(risky ? 1 : 0);

    // mean / std / cov of delta_jsd (records.rs:156-172)
    double acc = 0.0;
    for (uint32_t r = tid; r < n; r += WIDE) acc += d.dtmp[r];
    const double mean = dvs_block_sum(acc, scratch) / double(n);
    acc = 0.0;
    for (uint32_t r = tid; r < n; r += WIDE) {
        const double t = d.dtmp[r] - mean;
        acc += t * t;
    }
    const double sd = sqrt(dvs_block_sum(acc, scratch) / (double(n) - 1.0));
    const double cov = sd / mean;

    if (tid == 0) {
        int go = 1;  // 1 commit, 0 rollback, -1 stop for the arbiter
        const uint32_t forced = ctl->forced;
        const double band = sel_band(kind == 2 ? ctl->t_total_jsd + ctl->t_sum_entropy / double(n)
                                               : ctl->total_jsd + ctl->sum_entropy / double(n),
                                     d.B);
        const bool forced_fin = forced == FORCE_COMMIT || forced == FORCE_ROLLBACK;
        if (forced_fin) {
            go = forced == FORCE_COMMIT ? 1 : 0;
            if (ctl->forced_lowest != 0xFFFFFFFFu) lowest = ctl->forced_lowest;
            ctl->forced = FORCE_NONE;
            ctl->forced_lowest = 0xFFFFFFFFu;
        } else {
            bool tie = any_risky || ctl->ev_risky;
            if (n > 1 && dsecond - dmin <= band && dsecond < 1e6) tie = true;  // argmin ambiguous
            if (kind == 2) {
                const double a = ctl->stat == DVS_STAT_STDEV ? sd : cov;
                const double b = ctl->stat == DVS_STAT_STDEV ? ctl->std_delta : ctl->cov_delta;
                // every delta_jsd carries an error <= band, so std moves by <= ~band and
                // cov = std / mean by ~ band (1 + |cov|) / |mean|; NaN compares false
                const double mm = fmin(fabs(mean), fabs(ctl->mean_delta));
                const double sband = ctl->stat == DVS_STAT_STDEV
                                         ? 4.0 * band
                                         : 4.0 * band * (1.0 + fmax(fabs(a), fabs(b))) / fmax(mm, 1e-300);
                if (fabs(a - b) <= sband) tie = true;
                go = (a > b) ? 1 : 0;
            }
            if (tie) {
                ctl->status = SEL_ARBITER;
                ctl->arb_stage = ARB_FINALIZE;
                ctl->arb_pos = (kind == 2) ? d.mPos[n - 1] : ctl->cursor - 1;
                go = -1;
            }
        }
        if (go == 1) {
            if (kind == 2) {
                ctl->sum_entropy = ctl->t_sum_entropy;
                ctl->total_jsd = ctl->t_total_jsd;
                d.ord[n - 1] = n - 1;
                const uint32_t lab = d.mLabel[n - 1];
                if (lab < d.nlabels) d.inset[lab] = 1;
                ctl->size = n;
                ctl->n_accepts++;
                d.evlog_pos[ctl->n_logged] = d.mPos[n - 1];
                d.evlog_kind[ctl->n_logged] = 2;
                ctl->n_logged++;
            }
            ctl->lowest = lowest;
            ctl->mean_delta = mean;
            ctl->std_delta = sd;
            ctl->cov_delta = cov;
            ctl->band = band;
        }
        s_go = go;
    }
    __syncthreads();
    const int go = s_go;
    if (go < 0) return;
    if (go == 1) {
        if (kind == 2 && d.rowlog && ctl->n_logged) {  // the kept push's row
            const double *src = d.M + uint64_t(n - 1) * d.B;
            double *dst = d.rowlog + uint64_t((ctl->n_logged - 1) % d.rowlog_cap) * d.B;
            for (uint64_t i = tid; i < d.B; i += WIDE) dst[i] = src[i];
        }
        for (uint32_t r = tid; r < n; r += WIDE) d.mDelta[r] = d.dtmp[r];
        if (kind == 2)
            for (uint64_t i = tid; i < d.B; i += WIDE) d.S[i] = d.Stmp[i];
    }
    __syncthreads();
    // state for the next scan: b_i = (S_i - low_i) / size, thresholds
    const uint32_t sz = ctl->size;
    const uint32_t low_slot = d.ord[ctl->lowest];
    const double *low = d.M + uint64_t(low_slot) * d.B;
    const double dsize = double(sz);
    for (uint64_t i = tid; i < d.B; i += WIDE) d.base[i] = (d.S[i] - low[i]) / dsize;
    if (tid == 0) {
        ctl->he_base = ctl->sum_entropy - d.mH[low_slot];
        ctl->thr = ctl->total_jsd + DVS_EPS;
        ctl->ev_kind = 0;
        ctl->ev_risky = 0;
        ctl->mb_stuck = 0;
        ctl->event_pos = SEL_NONE;
        if (ctl->cursor >= ctl->npos) ctl->status = SEL_DONE;
        ctl_next_window(ctl);
    }
}

// Resolve kernel (one block).  (Resolve + leave-one-out + finalize as ONE single-block launch for
// small sets measured slower -- 10.6 vs 8.9 ms per stepwise selection: one CU issues every
// leave-one-out bin itself -- and was removed.)
template <typename T>
__global__ __launch_bounds__(WIDE_THREADS) void resolve_kernel(SelDev d, const T *__restrict__ mat) {
    __shared__ double scratch[48];
    __shared__ int s_flag;
    resolve_body<T>(d, mat, scratch, s_flag);
}

// Block r < n: the leave-one-out job of member r.  The LAST block adds up the rows the scan
// launch read (per-workgroup counters, cleared for the next launch) beside them, off the event's
// chain of dependent round trips.
__global__ __launch_bounds__(LOO_THREADS) void loo_kernel(SelDev d, uint32_t scan_grid) {
    __shared__ double scratch[48];
    if (blockIdx.x + 1 == gridDim.x) {
        double cnt = 0.0, cnt2 = 0.0, mnz = 0.0;
        for (uint32_t i = threadIdx.x; i < scan_grid; i += LOO_THREADS) {
            cnt += double(d.wg_rows[2 * i]);
            cnt2 += double(d.wg_rows[2 * i + 1]);
            d.wg_rows[2 * i] = 0;
            d.wg_rows[2 * i + 1] = 0;
        }
        block_red3(cnt, mnz, cnt2, scratch);
        if (threadIdx.x == 0 && (cnt != 0.0 || cnt2 != 0.0)) {  // (finalize_kernel, next in the stream, writes other words)
            d.ctl->rows_scored += (unsigned long long)cnt;
            d.ctl->rows_rechecked += (unsigned long long)cnt2;
        }
        return;
    }
    loo_body(d, blockIdx.x, scratch);
}

__global__ __launch_bounds__(WIDE_THREADS) void finalize_kernel(SelDev d) {
    __shared__ double scratch[48];
    __shared__ int s_go;
    finalize_body(d, scratch, s_go);
}

// delta_jsd of every query row against the set (SummedRecordsWrapper.delta_jsd,
// src/records_py.rs:111-120 -> records.rs:70-84).  One block per query.
template <typename T>
__global__ __launch_bounds__(LOO_THREADS) void score_kernel(SelDev d, const T *__restrict__ qmat,
                                                          const uint32_t *__restrict__ qtotals,
                                                          const double *__restrict__ qH,
                                                          const uint32_t *__restrict__ qlabels,
                                                          double *__restrict__ out) {
    __shared__ double scratch[32];
    const SelCtl *ctl = d.ctl;
    const uint32_t q = blockIdx.x;
    const uint32_t tot_u = qtotals[q];
    if (tot_u == 0) {
        if (threadIdx.x == 0) out[q] = NAN;
        return;
    }
    if (qlabels) {
        const uint32_t lab = qlabels[q];
        if (lab < d.nlabels && d.inset[lab]) {
            if (threadIdx.x == 0) out[q] = 0.0;
            return;
        }
    }
    const double tot = double(tot_u);
    const T *rp = qmat + uint64_t(q) * d.B;
    const uint32_t low_slot = d.ord[ctl->lowest];
    const double *low = d.M + uint64_t(low_slot) * d.B;
    const double dsize = double(ctl->size);
    Ent e;
    for (uint64_t i = threadIdx.x; i < d.B; i += LOO_THREADS)
        e.add((d.S[i] - low[i] + cand_freq(rp, i, tot)) / dsize);
    const double h = dvs_block_sum(e.h, scratch);
    const double mn = dvs_block_min(e.mn, scratch);
    if (threadIdx.x == 0) {
        const double mean_entropy = (ctl->sum_entropy - d.mH[low_slot] + qH[q]) / dsize;
        out[q] = (mn < 0.0) ? NAN : h - mean_entropy;
    }
}

// members in set order -> a dense device buffer (for the device-side chunk merge)
__global__ __launch_bounds__(LOO_THREADS) void gather_members_kernel(SelDev d, double *__restrict__ rows,
                                                                    double *__restrict__ meta) {
    const uint32_t r = blockIdx.x, n = d.ctl->size;
    double *out = rows + uint64_t(r) * d.B;
    if (r >= n) {
        for (uint64_t i = threadIdx.x; i < d.B; i += LOO_THREADS) out[i] = 0.0;
        if (threadIdx.x == 0) meta[2 * r] = meta[2 * r + 1] = 0.0;
        return;
    }
    const uint32_t slot = d.ord[r];
    const double *src = d.M + uint64_t(slot) * d.B;
    for (uint64_t i = threadIdx.x; i < d.B; i += LOO_THREADS) out[i] = src[i];
    if (threadIdx.x == 0) {
        meta[2 * r] = double(d.mPos[slot]);  // stream position (exact below 2^53)
        meta[2 * r + 1] = 1.0;
    }
}

}  // namespace

// ------------------------------------------------------------------ host side
static void sel_free(dvs_select *s) {
    if (!s) return;
#ifdef DVS_FS_TRACE
    dvs_stepwise_trace_report(s);
#endif
    // Work this selection queued on the context's side streams (the head phase's sync block, the seed
    // list, set-up kernels) may still be pending on an error path; the pool only orders reuse on the
    // context's own stream, so those streams are drained before their blocks go back to it.
    if (s->used_side_streams && s->ctx) {
        if (s->ctx->stream_head) (void)hipStreamSynchronize(s->ctx->stream_head);
        if (s->ctx->stream2) (void)hipStreamSynchronize(s->ctx->stream2);
    }
    void *ptrs[] = {s->dev.ctl, s->dev.S, s->dev.Stmp, s->dev.base, s->dev.cand, s->dev.M,
                    s->dev.mH, s->dev.mDelta, s->dev.dtmp, s->dev.dsum, s->dev.mLabel, s->dev.mPos,
                    s->dev.ord, s->dev.inset, s->dev.wg_rows, s->dev.evlog_pos, s->dev.evlog_kind, s->dev.rowlog,
                    (void *)s->dev.order, (void *)s->dev.labels};
    for (void *p : ptrs)
        dvs_dev_free(s->ctx, p);
    dvs_stepwise_wait(s);  // (in front of the pinned blocks' return: the fast step's queued launches write into one)
    dvs_pinned_put(s->ctx, s->h_ctl);
    for (hipEvent_t e : s->ev_pool) dvs_event_put(s->ctx, e);
    // each engine's own blocks, in the order the device pool takes them (the fast step's status history goes to the
    // pinned cache here, behind h_ctl)
    dvs_max_batch_free(s);
    dvs_stepwise_free(s);
    dvs_persist_free(s);
    if (!s->seed_list_in_ctl) dvs_dev_free(s->ctx, s->d_seed_list);
    if (s->ev_side_done) dvs_event_put(s->ctx, s->ev_side_done);
    dvs_select_arbiter_free(s);
    dvs_ctx_release(s->ctx);
    delete s;
}

hipEvent_t dvs_scan_timing_start(dvs_ctx *ctx, dvs_select *s, hipStream_t on) {
    if (!s->time_scan) return nullptr;
    if (s->ev_used + 2 > s->ev_pool.size()) {
        hipEvent_t a = dvs_event_get(ctx), b = dvs_event_get(ctx);
        s->ev_pool.push_back(a);
        s->ev_pool.push_back(b);
    }
    s->ev_used += 2;
    (void)hipEventRecord(s->ev_pool[s->ev_used - 2], on);
    return s->ev_pool[s->ev_used - 1];
}

// the pairs of the scan launches since the last poll (which synchronised the stream: the events are complete)
static void sel_add_scan_times(dvs_select *s) {
    for (size_t i = 0; i + 1 < s->ev_used; i += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s->ev_pool[i], s->ev_pool[i + 1]) == hipSuccess) {
            s->scan_ms += ms;
            s->scan_ms_last = ms;
        }
        s->scan_launches++;
    }
    s->ev_used = 0;
}

// one scan_kernel launch with the selection's geometry, against the control block `ctl` and the row counters `wg_rows`
// (the caller says which instantiation: `hot` picks scan_kernel<T, true>)
template <typename T>
static void launch_scan(const dvs_select *s, const T *mat, bool hot, SelCtl *ctl, uint32_t *wg_rows, hipStream_t st) {
    const SelDev &d = s->dev;
    if (hot)
        hipLaunchKernelGGL((scan_kernel<T, true>), dim3(s->scan_grid), dim3(SCAN_THREADS), s->scan_lds, st, ctl, mat, d.totals,
                           d.rowH, d.order, d.labels, d.inset, d.nlabels, d.base, wg_rows, d.B, s->base_in_lds ? 1 : 0);
    else
        hipLaunchKernelGGL((scan_kernel<T, false>), dim3(s->scan_grid), dim3(SCAN_THREADS), s->scan_lds, st, ctl, mat, d.totals,
                           d.rowH, d.order, d.labels, d.inset, d.nlabels, d.base, wg_rows, d.B, s->base_in_lds ? 1 : 0);
}

// stage 0: scan + resolve + loo + finalize; 1: resolve + loo + finalize; 2: loo + finalize
template <typename T>
static void launch_iteration(dvs_ctx *ctx, dvs_select *s, const T *mat, int stage, hipStream_t on = nullptr) {
    const SelDev &d = s->dev;
    const hipStream_t stream = on ? on : ctx->stream;
    if (stage == 0) {
        const hipEvent_t e1 = dvs_scan_timing_start(ctx, s, stream);
        launch_scan<T>(s, mat, s->scan_hot, d.ctl, d.wg_rows, stream);
        if (s->time_scan) (void)hipEventRecord(e1, stream);
    }
    if (stage <= 1)
        hipLaunchKernelGGL((resolve_kernel<T>), dim3(1), dim3(WIDE_THREADS), 0, stream, d, mat);
    hipLaunchKernelGGL(loo_kernel, dim3(s->loo_grid + 1), dim3(LOO_THREADS), 0, stream, d, s->scan_grid);
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(WIDE_THREADS), 0, stream, d);
}

// ... and both for stepwise.hip, on the context's stream (the matrix's element type is found here)
void dvs_select_launch_scan(dvs_ctx *ctx, dvs_select *s, bool hot) {
    dvs_mat_dispatch(s->mat, [&](auto *mp) { launch_scan(s, mp, hot, s->dev.ctl, s->dev.wg_rows, ctx->stream); return 0; });
}
void dvs_select_launch_iteration(dvs_ctx *ctx, dvs_select *s, int stage) {
    dvs_mat_dispatch(s->mat, [&](auto *mp) { launch_iteration(ctx, s, mp, stage); return 0; });
}

int dvs_select_poll(dvs_ctx *ctx, dvs_select *s) {
    DVS_HIP(ctx, hipMemcpyAsync(s->h_ctl, s->dev.ctl, sizeof(SelCtl), hipMemcpyDeviceToHost,
                                ctx->stream));
    DVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const_cast<dvs_matrix *>(s->mat)->in_flight = false;  // (the stream held the matrix's build, or the wait for it)
    return DVS_OK;
}

template <typename T>
static int sel_seed(dvs_ctx *ctx, dvs_select *s, const T *mat, hipStream_t st, bool light = false);

// Drop the seeded start: the set-up kernels set the initial set up after all (enqueued on `st`), and the next
// persistent launch starts from the state they leave
template <typename T>
static int sel_drop_seeded(dvs_ctx *ctx, dvs_select *s, const T *mat, hipStream_t st) {
    s->seeded_start = false;
    s->persist.seeded = false;
    return sel_seed<T>(ctx, s, mat, st);
}

// Leave the persistent engine for good: the multi-launch engine, which needs no co-residency, carries on from the
// state the engine left or, with `restart`, starts the selection over from its seeds
template <typename T>
static int sel_leave_persist(dvs_ctx *ctx, dvs_select *s, const T *mat, bool restart) {
    s->persist.on = false;
    if (!restart) return DVS_OK;
    dvs_select_arbiter_free(s);  // (its replay of the event log belongs to the abandoned run)
    return sel_drop_seeded<T>(ctx, s, mat, ctx->stream);
}

// A decision inside the rounding band (status SEL_ARBITER, h_ctl current): the host arbiter takes it, and the kernels
// of the stage the device stopped at carry on from its verdict
template <typename T>
static int sel_arbitrate(dvs_ctx *ctx, dvs_select *s, const T *mat) {
    const SelCtl &c = *s->h_ctl;
    if (s->params.flags & DVS_SELECT_NO_ARBITER)
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED,
                             "ambiguous decision at stream position %llu (stage %u): "
                             "|score - threshold| within the rounding band",
                             (unsigned long long)c.arb_pos, c.arb_stage);
    const uint32_t stage = c.arb_stage;  // (the arbiter hands it back as it came)
    const auto t_arb = std::chrono::steady_clock::now();
    const int rc = dvs_select_arbitrate(ctx, s);
    s->arbiter_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_arb).count();
    if (rc) return rc;
    launch_iteration<T>(ctx, s, mat, stage == ARB_RESOLVE ? 1 : 2);
    DVS_HIP(ctx, hipGetLastError());
    return DVS_OK;
}

int dvs_select_arbitrate_resume(dvs_ctx *ctx, dvs_select *s) {
    return dvs_mat_dispatch(s->mat, [&](auto *mp) { return sel_arbitrate(ctx, s, mp); });
}

// the engine behind the set-up sel_start enqueued, driven to the end of the stream
template <typename T>
static int sel_run_loop(dvs_ctx *ctx, dvs_select *s, const T *mat) {
    unsigned long long persist_cursor = 0;
    unsigned persist_launches = 0;
    bool persist_was_last = false;  // nothing but the poll happened since the last persistent launch
    unsigned persist_idle = 0;      // persistent launches in a row that came back where they started
    bool mb_seen = false, mb_dense = true;  // MODE_MAX batches: events per row between the last two looks (dense until seen otherwise)
    unsigned long long mb_cursor = 0, mb_events = 0;
    bool mb_useful = true;
    uint32_t mb_rows_seen = 0, mb_round_pairs = 0, mb_idle_rounds = 0;
    // one persistent launch from the state at `cursor`.  A grid the runtime refuses leaves the engine for the
    // multi-launch kernels -- from the seeds if it was a seeded start's first launch (nothing set the initial set up
    // yet: the set-up kernels do)
    auto persist_launch = [&](unsigned long long cursor) {
        persist_cursor = cursor;
        persist_launches++;
        persist_was_last = true;
        const int rc = dvs_persist_launch(ctx, s);
        if (rc != DVS_ERR_UNSUPPORTED) return rc;
        return sel_leave_persist<T>(ctx, s, mat, s->seeded_start && persist_launches == 1);
    };
    if (s->persist.on) {
        // straight behind the set-up kernels, no host round trip in between: the kernel itself
        // returns at once unless the control block says RUN
        int rc = persist_launch(s->params.n_seed);  // (the cursor the set-up leaves behind)
        if (rc) return rc;
    }
    for (;;) {
        int rc = dvs_select_poll(ctx, s);
        if (rc) return rc;
        const SelCtl &c = *s->h_ctl;
        sel_add_scan_times(s);
        if (ctx->knobs.persist_debug) dvs_persist_debug_report(ctx, s);
        const bool fake_error = ctx->knobs.test_persist_fake_error;  // (test knob: needs DVS_TEST_KNOBS=1 as well)
        if (s->persist.on && persist_launches && (c.status == SEL_ERROR || (fake_error && persist_launches == 1))) {
            // The persistent kernel gave up at a grid barrier: its workgroups were not all resident
            // (a CU mask, a partitioned device, another stream's kernels holding CUs).  The
            // replicas may have stopped mid-update, so the selection starts over from its seeds and
            // the multi-launch engine, which needs no co-residency, serves the request.
            if (!fake_error) ctx->persist_timeouts++;  // (three in a row and the context stops trying)
            if ((rc = sel_leave_persist<T>(ctx, s, mat, true))) return rc;
            continue;
        }
        if (s->seeded_start && s->persist.on && persist_launches == 1 &&
            (c.status == SEL_NEED_SETUP || (c.status == SEL_RUN && c.cursor == s->params.n_seed))) {
            // the seeded launch left the initial set alone (its first argmin too close to call on the
            // device): the set-up kernels after all, and the engine again from the state they leave
            if ((rc = sel_drop_seeded<T>(ctx, s, mat, ctx->stream)) || (rc = persist_launch(s->params.n_seed))) return rc;
            continue;
        }
        if (c.status == SEL_DONE) {
            if (ctx->knobs.persist_debug) dvs_persist_debug_done(c);
            if (s->persist.on && persist_launches) ctx->persist_timeouts = 0;
            return DVS_OK;
        }
        if (c.status == SEL_ARBITER) {
            if ((rc = sel_arbitrate<T>(ctx, s, mat))) return rc;
            persist_was_last = false;
            continue;
        }
        if (c.status == SEL_ERROR)
            return dvs_set_error(ctx, DVS_ERR_RUNTIME, "selection engine stopped with an internal error");
        if (c.status != SEL_RUN)
            return dvs_set_error(ctx, DVS_ERR_RUNTIME, "selection engine in state %u", c.status);
        // a `max` set that has outgrown the engine's LDS replica and may still grow: the engine would hand
        // every launch straight back (it did: 152 of 309 launches of a 664-member cov selection) -- the
        // multi-launch kernels keep the stream until the set is full
        const bool replica_full = s->params.mode == DVS_MODE_MAX && c.size + 2 > s->persist.maxn && c.size < c.max_size;
        if (s->persist.on && !replica_full) {
            // a persistent launch that comes back still RUNNING with the cursor where it was did
            // not take the state it found (e.g. an event left pending by the arbiter's hand-off):
            // the multi-launch kernels, which take any state, carry on -- never a relaunch loop
            if (persist_launches && persist_was_last && c.cursor == persist_cursor) {
                persist_was_last = false;  // multi-launch iterations, then the engine again
                persist_idle++;
            } else {
                if (persist_launches && c.cursor != persist_cursor) persist_idle = 0;
                if ((rc = persist_launch(c.cursor))) return rc;
                if (s->persist.on) continue;  // (refused: the multi-launch kernels below take over)
            }
        }
        // (behind a persistent launch that left ONE event for these kernels -- a decision inside its band --
        // a single iteration takes that event; the engine is launched again right after)
        // (an engine that keeps coming back where it started -- a set its replica cannot hold -- gets whole batches)
        if (replica_full) persist_was_last = false;
        const int iters = (s->persist.on && !replica_full && persist_launches && !persist_was_last && persist_idle < 2) ? 1 : s->batch;
        // MODE_MAX while the set may grow: where at least every second row since the last look was an event,
        // a batch pair goes in front of every iteration (it skips the rows that change nothing)
        if (mb_seen) {
            const unsigned long long rows = c.cursor - mb_cursor, evs = c.n_events - mb_events;
            if (rows) mb_dense = evs * 2 >= rows;
        }
        mb_seen = true;
        mb_cursor = c.cursor;
        mb_events = c.n_events;
        // ... and only while the pairs earn their keep: a stream whose pushes are nearly all KEPT (cov over
        // sequences of very different composition) stops every batch at its first row -- then they are left
        // out, and tried again every eighth look
        // (a probe: pairs in front of the first two iterations of a look only)
        if (mb_round_pairs) mb_useful = (c.mb_rows - mb_rows_seen) >= 2u * mb_round_pairs;
        mb_rows_seen = c.mb_rows;
        mb_round_pairs = 0;
        const bool mb_can = mb_dense && iters > 1 && c.mode == DVS_MODE_MAX && c.size < c.max_size && c.s_is_resum != 0 &&
                            !(s->params.flags & DVS_SELECT_STEPWISE);
        const bool mb_probe = mb_can && !mb_useful && ++mb_idle_rounds >= 4;
        if (mb_probe || mb_useful) mb_idle_rounds = 0;
        const int mb_iters = !mb_can ? 0 : mb_useful ? iters : mb_probe ? 2 : 0;  // (a selection starts with them on)
        for (int i = 0; i < iters; i++) {
            for (int b = 0; i < mb_iters && b < 3; b++) {  // (the second and third return at once where the first one stopped at a row)
                if ((rc = dvs_max_batch_launch(ctx, s, c.size + uint32_t(i)))) return rc;
                mb_round_pairs += b == 0;
            }
            launch_iteration<T>(ctx, s, mat, 0);
        }
        DVS_HIP(ctx, hipGetLastError());
    }
}

// The stream a selection's set-up (control block, seed list, set-up kernels) goes to, decided once per
// selection (the label flags are cleared on it ahead of time).  When the rest of the matrix is still being
// built on the context's stream (a split build, kmer_hist.hip: the head rows are finished, the host has their
// totals), the set-up -- which reads only the seed rows -- goes to a side stream and runs beside that launch
// instead of queueing behind it; the engine itself is launched on the first stream behind both.
// HEAD PHASE: that launch runs on the context's stream_rest and leaves the head CUs alone (CU split), so the
// persistent engine starts on them right behind the set-up and walks the rows that are already built -- the
// event-dense head of the stream, a chain of hand-overs that needs no more than a few workgroups -- while
// the histogram runs; the launch over the full grid then carries on from the state it mirrors.  (nmost; a
// set whose leave-one-out jobs fit the head grid one per workgroup.)
static void sel_plan_setup_stream(dvs_ctx *ctx, dvs_select *s) {
    s->setup_side = nullptr;
    s->head_phase = false;
    if (s->mat->head_rows_built && s->params.n_seed <= s->mat->head_rows_built && s->h_order.empty() &&
        !(s->params.flags & DVS_SELECT_STEPWISE)) {
        s->head_phase = s->mat->rest_beside_head && ctx->stream_head && s->persist.on &&
                        s->params.mode == DVS_MODE_NMOST && s->params.window == 0 &&
                        s->cap + 2 <= uint32_t(ctx->head_cus) && s->npos > 4ull * s->mat->head_rows_built &&
                        s->params.n_seed + 64 <= s->mat->head_rows_built && !ctx->knobs.no_head_phase;
        s->setup_side = s->head_phase ? ctx->stream_head : dvs_ctx_stream2(ctx);
    }
}

template <typename T>
static int sel_start(dvs_ctx *ctx, dvs_select *s, const T *mat) {
    hipStream_t side = s->setup_side;
    const bool head_phase = s->head_phase;
    hipStream_t st = side ? side : ctx->stream;
    if (side) s->used_side_streams = true;
    int rc = sel_seed<T>(ctx, s, mat, st, s->seeded_start);
    if (rc) return rc;
    if (head_phase) {
        rc = dvs_persist_launch_head(ctx, s, uint32_t(ctx->head_cus), s->mat->head_rows_built, side);
        if (rc == DVS_ERR_UNSUPPORTED)  // (refused: the full-grid launch starts from the seeds -- which, unseeded, it needs the set-up kernels for)
            rc = s->seeded_start ? sel_drop_seeded<T>(ctx, s, mat, st) : DVS_OK;
        if (rc) return rc;
        // the full-grid launch's sync block and accumulators: behind the histogram on the context's
        // stream, i.e. while the head phase runs, not between the two launches
        rc = dvs_persist_prepare_main(ctx, s);
        if (rc) return rc;
        // (a later selection over the same matrix finds the histogram finished: nothing to run beside)
        const_cast<dvs_matrix *>(s->mat)->rest_beside_head = false;
    }
    if (side) {
        if (!s->ev_side_done) s->ev_side_done = dvs_event_get(ctx);
        DVS_HIP(ctx, hipEventRecord(s->ev_side_done, side));
        DVS_HIP(ctx, hipStreamWaitEvent(ctx->stream, s->ev_side_done, 0));
    }
    if (s->params.flags & DVS_SELECT_STEPWISE) return dvs_select_poll(ctx, s);
    return sel_run_loop<T>(ctx, s, mat);
}

// control block of a fresh selection + the initial set from the seed positions (SummedRecords::new
// over the first n usable records, records.rs:288-308), enqueued on `st`; also the way back to a clean
// state when the persistent engine has to be abandoned
// light: only what a SEEDED persistent launch reads -- the control block and the seed list; the initial
// set is worked out by that launch itself (persist.hip) instead of the four kernels below
template <typename T>
static int sel_seed(dvs_ctx *ctx, dvs_select *s, const T *mat, hipStream_t st, bool light) {
    const std::vector<uint64_t> &seeds = s->seed_positions;
    SelDev &d = s->dev;
    SelCtl c = s->ctl0;
    // default window: a quarter of the persistent grid's waves (measured best: early in the
    // stream an accept comes every few hundred rows), else 4096 rows per scan launch
    const uint32_t wdef = s->params.window ? s->params.window : (s->persist.on ? s->persist.grid * 2u : 4096u);
    c.window_min = wdef;
    c.window_max = std::max<uint32_t>(wdef, s->scan_grid * (SCAN_THREADS / 64) * 8);
    c.window = wdef;
    // (the control block travels through the pinned mirror: a pageable source would have to stay
    // alive until the copy has been performed)
    *s->h_ctl = c;
    // (a restart, or a start on another stream than the planned one: the flags are cleared here)
    if (!s->inset_clean || st != (s->setup_side ? s->setup_side : ctx->stream))
        DVS_HIP(ctx, hipMemsetAsync(d.inset, 0, std::max<size_t>(d.nlabels, 1), st));
    s->inset_clean = false;
    if (!s->d_seed_list) {
        int rc0 = dvs_dev_alloc(ctx, &s->d_seed_list, seeds.size() * sizeof(uint64_t), "seed list");
        if (rc0) return rc0;
    }
    uint64_t *d_seed = static_cast<uint64_t *>(s->d_seed_list);
    if (s->seed_list_in_ctl) {  // control block + seed list: one block, one copy
        std::memcpy(reinterpret_cast<unsigned char *>(s->h_ctl) + SEL_SEEDS_AT, seeds.data(), seeds.size() * sizeof(uint64_t));
        DVS_HIP(ctx, hipMemcpyAsync(d.ctl, s->h_ctl, SEL_SEEDS_AT + seeds.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    } else {
        DVS_HIP(ctx, hipMemcpyAsync(d.ctl, s->h_ctl, sizeof c, hipMemcpyHostToDevice, st));
        DVS_HIP(ctx, hipMemcpyAsync(d_seed, seeds.data(), seeds.size() * sizeof(uint64_t),
                                    hipMemcpyHostToDevice, st));
    }
    if (light) {
        DVS_HIP(ctx, hipGetLastError());
        return DVS_OK;
    }
    hipLaunchKernelGGL((seed_kernel<T>), dim3(uint32_t(seeds.size())), dim3(LOO_THREADS), 0,
                       st, s->dev, mat, d_seed);
    hipLaunchKernelGGL(rebuild_sum_kernel, dim3(uint32_t((s->dev.B + RSUM_THREADS - 1) / RSUM_THREADS)), dim3(RSUM_THREADS), 0, st, s->dev);
    hipLaunchKernelGGL(rebuild_kernel, dim3(1), dim3(WIDE_THREADS), 0, st, s->dev);
    launch_iteration<T>(ctx, s, mat, 2, st);  // loo + finalize of the initial set
    // (one fused launch of one block for sets of <= 16 measured no faster: 2.29 vs 2.27 ms per step)
    DVS_HIP(ctx, hipGetLastError());
    return DVS_OK;
}

// ---- dvs_select_run's phases, in the order it calls them

// The caller's arguments, checked, and what follows from them (host only: nothing is allocated yet)
struct SelArgs {
    uint32_t n_seed = 0, max_size = 0, nlabels = 0, cap = 0;
    const uint32_t *labels = nullptr;         // the labels the engine runs with (nullptr: label = row) ...
    const uint32_t *caller_labels = nullptr;  // ... and the caller's, when they were all distinct
};

static int sel_check_args(dvs_ctx *ctx, const dvs_matrix *m, const uint32_t *order, const uint32_t *labels,
                          uint64_t npos, const dvs_select_params *params, SelArgs &a) {
    const uint64_t B = m->nbins;
    if (!order && npos > m->nrows)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "npos %llu exceeds the matrix rows %u",
                             (unsigned long long)npos, m->nrows);
    uint32_t n_seed = params->n_seed;
    uint32_t max_size = params->max_size;
    if (params->mode == DVS_MODE_SET) n_seed = uint32_t(npos);
    // Labels only say which positions are the same sequence id (records.rs:71-73: an id already in
    // the set scores 0.0).  When every label occurs once -- what the reference's callers pass: the
    // ids of a store are unique -- no position can meet its own id in the set, so the engine runs
    // label-free (label = position: the persistent engine qualifies) and the caller's values are
    // put back on the way out (dvs_select_get_members, dvs_select_delta_jsd).
    if (labels && !order && params->mode != DVS_MODE_SET) {
        bool distinct = true;
        bool rising = true;  // (the usual call: the positions themselves -- one pass, no copy)
        for (uint64_t p = 1; p < npos && rising; p++) rising = labels[p] > labels[p - 1];
        if (!rising) {
            std::vector<uint32_t> sorted(labels, labels + npos);
            std::sort(sorted.begin(), sorted.end());
            for (uint64_t p = 1; p < npos && distinct; p++)
                distinct = sorted[p] != sorted[p - 1] || sorted[p] == 0xFFFFFFFFu;
        }
        if (distinct) {
            a.caller_labels = labels;
            labels = nullptr;
        }
    }
    a.labels = labels;
    // src/records.rs:323-325, 404-410, 369-371, 464-469
    if (npos < n_seed)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "The number of sequences %llu is < n %u",
                             (unsigned long long)npos, n_seed);
    if (params->mode == DVS_MODE_MAX && npos <= max_size) max_size = uint32_t(npos);  // :412-416
    if (params->mode != DVS_MODE_MAX) max_size = n_seed;

    // usable seeds: rows with at least one valid k-mer (records.rs:299-306)
    uint32_t nlabels = 0;
    if (order || labels) {
        for (uint64_t p = 0; p < npos; p++) {
            const uint32_t row = order ? order[p] : uint32_t(p);
            if (row == DVS_ROW_REMOTE) continue;
            if (row >= m->nrows)
                return dvs_set_error(ctx, DVS_ERR_VALUE, "order[%llu] = %u out of range",
                                     (unsigned long long)p, row);
            const uint32_t lab = labels ? labels[p] : row;
            if (lab != 0xFFFFFFFFu) nlabels = std::max(nlabels, lab + 1);
        }
    } else {
        nlabels = uint32_t(npos);  // label = row = position
    }
    // only the seed rows' totals are needed on the host
    if (order)
        for (uint64_t p = 0; p < n_seed; p++)
            if (order[p] == DVS_ROW_REMOTE)
                return dvs_set_error(ctx, DVS_ERR_VALUE,
                                     "seed position %llu is not local: the first n rows must be replicated",
                                     (unsigned long long)p);
    const uint32_t cap = std::max<uint32_t>(std::max<uint32_t>(max_size, n_seed) + 1, 2);  // (seeds <= n_seed)
    const size_t need = size_t(cap) * B * 8 + 5 * B * 8 + size_t(npos) * 8 + nlabels + (1 << 20);
    size_t free_b = 0, total_b = 0;
    if (need > (size_t(1) << 30)) DVS_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    if (need > (size_t(1) << 30) && need > free_b + ctx->pool_bytes)
        return dvs_set_error(ctx, DVS_ERR_NOMEM, "selection state needs %zu bytes, %zu free", need,
                             free_b);
    a.n_seed = n_seed;
    a.max_size = max_size;
    a.nlabels = nlabels;
    a.cap = cap;
    return DVS_OK;
}

// launch geometry of the multi-launch kernels
static int sel_geometry(dvs_ctx *ctx, dvs_select *s, const uint32_t *order, const uint32_t *labels) {
    const uint64_t B = s->dev.B;
    s->base_in_lds = B * 8 <= 128 * 1024 && B * 8 + 1024 <= ctx->lds_per_block;
    s->scan_lds = 16 + (s->base_in_lds ? B * 8 : 0);
    const uint32_t wg_fit = s->base_in_lds ? std::max<uint32_t>(1, uint32_t((160 * 1024) / (B * 8 + 512))) : 4;
    uint32_t wg_per_cu = std::min<uint32_t>(wg_fit, 2);  // 16 waves per CU, 16 KB of loads in flight each
    s->scan_grid = std::max<uint32_t>(1, uint32_t(ctx->n_cu) * wg_per_cu);
    s->loo_grid = s->cap;
    // measured slower than three launches (one CU does the whole leave-one-out pass): opt-in only
    s->batch = 16;
    s->time_scan = ctx->timing;
    s->scan_hot = B % (256 * SCAN_CH) == 0 && !order && !labels && s->base_in_lds;
    if (s->scan_lds <= 48 * 1024) return DVS_OK;
    const void *fn = dvs_mat_dispatch(s->mat, [&](auto *mp) -> const void * {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(mp)>>;
        return s->scan_hot ? reinterpret_cast<const void *>(scan_kernel<T, true>)
                           : reinterpret_cast<const void *>(scan_kernel<T, false>);
    });
    return dvs_raise_dyn_lds(ctx, fn, s->scan_lds);
}

// Device and pinned memory: the set state, the stepwise mode's blocks (stepwise.hip), the engine's copies of
// the order and labels (uploaded on the context's stream) and the control block's pinned mirror
static int sel_alloc(dvs_ctx *ctx, dvs_select *s, const uint32_t *order, const uint32_t *labels) {
    SelDev &d = s->dev;
    const uint64_t B = d.B, npos = s->npos;
    const uint32_t cap = s->cap, nlabels = d.nlabels;
    const size_t nlog = size_t(npos - s->params.n_seed + 2);
    // (the control block and, behind it, the seed list: ONE upload per selection, sel_seed)
    static_assert(sizeof(SelCtl) <= SEL_SEEDS_AT, "the seed list starts behind the control block");
    const struct { void **ptr; size_t bytes; const char *what; } blocks[] = {
        {(void **)&d.ctl, 4096, "d.ctl"},
        {(void **)&d.S, B * 8, "d.S"},
        {(void **)&d.Stmp, B * 8, "d.Stmp"},
        {(void **)&d.base, B * 8, "d.base"},
        {(void **)&d.cand, B * 8, "d.cand"},
        {(void **)&d.M, size_t(cap) * B * 8, "d.M"},
        {(void **)&d.mH, size_t(cap) * 8, "d.mH"},
        {(void **)&d.mDelta, size_t(cap) * 8, "d.mDelta"},
        {(void **)&d.dtmp, size_t(cap) * 8, "d.dtmp"},
        {(void **)&d.dsum, size_t(cap) * 8, "d.dsum"},
        {(void **)&d.mLabel, size_t(cap) * 4, "d.mLabel"},
        {(void **)&d.mPos, size_t(cap) * 8, "d.mPos"},
        {(void **)&d.ord, size_t(cap) * 4, "d.ord"},
        {(void **)&d.inset, std::max<size_t>(nlabels, 1), "d.inset"},
        {(void **)&d.wg_rows, size_t(s->scan_grid) * 8, "d.wg_rows"},
        {(void **)&d.evlog_pos, nlog * 8, "d.evlog_pos"},
        {(void **)&d.evlog_kind, nlog * 4, "d.evlog_kind"},
    };
    for (const auto &b : blocks)
        if (int rc = dvs_dev_alloc(ctx, b.ptr, b.bytes, b.what)) return rc;
    if (s->params.flags & DVS_SELECT_STEPWISE)
        if (int rc = dvs_stepwise_alloc(ctx, s, labels)) return rc;
    if (order) {
        if (int rc = dvs_dev_alloc(ctx, (void **)&d.order, size_t(npos) * 4, "d.order")) return rc;
        DVS_HIP(ctx, hipMemcpyAsync((void *)d.order, order, size_t(npos) * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    if (labels) {
        if (int rc = dvs_dev_alloc(ctx, (void **)&d.labels, size_t(npos) * 4, "d.labels")) return rc;
        DVS_HIP(ctx, hipMemcpyAsync((void *)d.labels, labels, size_t(npos) * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    static_assert(sizeof(SelCtl) <= 4096, "control block must fit a cached pinned block");
    return dvs_pinned_get(ctx, (void **)&s->h_ctl);
}

// The engine (persist.hip decides whether the persistent one serves) and the stream of its set-up, with what can go
// out before the matrix is waited for
static int sel_prepare_engine(dvs_ctx *ctx, dvs_select *s, const uint32_t *order, const uint32_t *labels) {
    SelDev &d = s->dev;
    const dvs_matrix *m = s->mat;
    const uint32_t n_seed = s->params.n_seed, nlabels = d.nlabels;
    int rc = dvs_persist_setup(ctx, s);
    if (rc) return rc;
    // The label flags are cleared NOW, on the stream the set-up will use (same stream: ordered in front of
    // everything that sets one): nothing about them depends on the seeds, so the fill runs while the matrix's
    // head rows are still being built, not between the host's wake-up and the first launch.
    sel_plan_setup_stream(ctx, s);
    if (s->setup_side) s->used_side_streams = true;
    DVS_HIP(ctx, hipMemsetAsync(d.inset, 0, std::max<size_t>(nlabels, 1), s->setup_side ? s->setup_side : ctx->stream));
    s->inset_clean = true;
    // ... and so are the scan workgroups' row counters, which the set-up's own leave-one-out launch adds up (on the
    // context's stream this fill raced with a set-up on a side stream: `rows_scored` of a selection with a set of
    // more than 32 came out 4.4 M too high whenever the pool's block still held another selection's counters)
    DVS_HIP(ctx, hipMemsetAsync(d.wg_rows, 0, size_t(s->scan_grid) * 8, s->setup_side ? s->setup_side : ctx->stream));
    // SEEDED start (persist.hip): an nmost selection whose state fits the persistent kernel's register
    // cache is begun by that kernel itself -- S, the entropy sum, the leave-one-out pass and the first
    // lowest member from nothing but the seed positions -- instead of four launches in front of it
    // (sets of up to 32: beyond that the S of the seeds -- a memory round trip per four members -- costs
    // what the launches cost; DVS_PERSIST_NO_SEEDED=1 turns it off)
    // (a STEPWISE selection never launches the persistent kernel: its set-up kernels must run)
    s->seeded_start = s->persist.on && s->params.mode == DVS_MODE_NMOST && d.B <= 4096 && !order && !labels &&
                      !(s->params.flags & DVS_SELECT_STEPWISE) && n_seed >= 2 && n_seed <= 32 && !ctx->knobs.persist_no_seeded;
    s->persist.seeded = s->seeded_start;
    if (size_t(n_seed) * sizeof(uint64_t) <= 4096 - SEL_SEEDS_AT) {
        s->d_seed_list = reinterpret_cast<unsigned char *>(d.ctl) + SEL_SEEDS_AT;
        s->seed_list_in_ctl = true;
    } else if (s->seeded_start) {
        if ((rc = dvs_dev_alloc(ctx, &s->d_seed_list, size_t(n_seed) * sizeof(uint64_t), "seed list"))) return rc;
    }
    // (what the head phase needs besides the seeds goes out before the wait below, on its stream)
    if (s->persist.on && m->rest_beside_head && ctx->stream_head && m->head_rows_built && s->params.mode == DVS_MODE_NMOST &&
        !order && !labels) {
        s->used_side_streams = true;
        return dvs_persist_prepare_head(ctx, s, m->head_rows_built, ctx->stream_head);
    }
    return DVS_OK;
}

// The usable seeds -- positions among the first n whose row has a valid k-mer -- into s->seed_positions
static int sel_read_seeds(dvs_ctx *ctx, dvs_select *s, const uint32_t *order) {
    const dvs_matrix *m = s->mat;
    const uint32_t n_seed = s->params.n_seed;
    std::vector<uint32_t> h_tot(n_seed);
    // (a matrix whose build is still in flight is waited for HERE, with everything above -- the
    // allocations, the memsets, the engine set-up -- done while its kernels ran)
    int rc = dvs_matrix_settle(ctx, m);
    if (rc) return rc;
    hipError_t ce = hipSuccess;
    if (!order && n_seed && n_seed <= m->h_head_totals.size()) {
        std::copy(m->h_head_totals.begin(), m->h_head_totals.begin() + n_seed, h_tot.begin());  // no round trip
    } else if (!order && n_seed) {
        ce = hipMemcpyAsync(h_tot.data(), m->d_totals, size_t(n_seed) * 4, hipMemcpyDeviceToHost, ctx->stream);
    } else {
        for (uint64_t p = 0; p < n_seed && ce == hipSuccess; p++)
            ce = hipMemcpyAsync(&h_tot[p], m->d_totals + order[p], 4, hipMemcpyDeviceToHost, ctx->stream);
    }
    if ((order || n_seed > m->h_head_totals.size()) &&
        (hipStreamSynchronize(ctx->stream) != hipSuccess || ce != hipSuccess))
        return dvs_set_error(ctx, DVS_ERR_RUNTIME, "reading the seed rows' totals failed");
    std::vector<uint64_t> &seeds = s->seed_positions;
    for (uint64_t p = 0; p < n_seed; p++)
        if (h_tot[p] > 0) seeds.push_back(p);
    if (seeds.size() < 2)
        return seeds.empty() ? dvs_set_error(ctx, DVS_ERR_VALUE, "records cannot be empty")   // :28-30
                             : dvs_set_error(ctx, DVS_ERR_VALUE, "must have > 1 KmerSeq");     // :227-230
    return DVS_OK;
}

// the control block of the fresh selection (sel_seed adds the window policy of the engine in charge and uploads it)
static void sel_init_ctl(dvs_ctx *ctx, dvs_select *s) {
    SelCtl c;
    std::memset(&c, 0, sizeof c);
    c.cursor = s->params.n_seed;
    c.npos = s->npos;
    c.event_pos = SEL_NONE;
    c.status = SEL_RUN;  // finalize flips to DONE when cursor >= npos
    c.size = uint32_t(s->seed_positions.size());
    c.mode = s->params.mode;
    c.max_size = s->params.max_size;
    c.stat = s->params.stat;
    c.forced = FORCE_NONE;
    c.forced_lowest = 0xFFFFFFFFu;
    c.band = 0.0;
    // measured on the north-star shape: {2, 3, 4} x window_min {256..2048}, and power laws
    // wc * gap^0.5..0.75 for the early stream, are all within 3 % of each other
    c.wscale = 4.0;
    if (ctx->knobs.persist_no_events) c.wscale = 1e5;  // (the pure-stream measurement: a few long windows)
    s->ctl0 = c;
}

extern "C" int dvs_select_run(dvs_ctx *ctx, const dvs_matrix *m, const uint32_t *order,
                              const uint32_t *labels, uint64_t npos,
                              const dvs_select_params *params, dvs_select **out) {
    if (!ctx || !m || !params || !out) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    *out = nullptr;
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    SelArgs a;
    int rc = sel_check_args(ctx, m, order, labels, npos, params, a);
    if (rc) return rc;
    labels = a.labels;
    // (the selection under construction is released on every way out but the last)
    std::unique_ptr<dvs_select, void (*)(dvs_select *)> s(new dvs_select(), sel_free);
    s->ctx = ctx;
    dvs_ctx_retain(ctx);
    s->params = *params;
    s->params.n_seed = a.n_seed;
    s->params.max_size = a.max_size;
    s->mat = m;
    s->mat_kind = m->kind;
    s->npos = npos;
    s->h_order.assign(order ? order : nullptr, order ? order + npos : nullptr);
    s->h_labels.assign(labels ? labels : nullptr, labels ? labels + npos : nullptr);
    if (a.caller_labels) s->h_out_labels.assign(a.caller_labels, a.caller_labels + npos);
    s->cap = a.cap;
    s->dev.B = m->nbins;
    s->dev.nlabels = a.nlabels;
    s->dev.totals = m->d_totals;
    s->dev.rowH = m->d_entropy;
    // (a set-up that fails has uploads, fills and perhaps kernels queued on the context's stream over blocks that sel_free
    // is about to hand back: the stream is waited for first; the side streams are sel_free's own, used_side_streams)
    auto failed = [&](int code) {
        (void)hipStreamSynchronize(ctx->stream);
        return code;
    };
    if ((rc = sel_geometry(ctx, s.get(), order, labels)) || (rc = sel_alloc(ctx, s.get(), order, labels)) ||
        (rc = sel_prepare_engine(ctx, s.get(), order, labels)) || (rc = sel_read_seeds(ctx, s.get(), order)))
        return failed(rc);
    sel_init_ctl(ctx, s.get());
    if ((rc = dvs_mat_dispatch(m, [&](auto *mp) { return sel_start(ctx, s.get(), mp); }))) return failed(rc);
    *out = s.release();
    return DVS_OK;
}

extern "C" void dvs_select_destroy(dvs_select *s) { sel_free(s); }

extern "C" int dvs_select_get_summary(dvs_ctx *ctx, const dvs_select *s, dvs_select_summary *out) {
    if (!s || !out) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    const SelCtl &c = *s->h_ctl;
    std::memset(out, 0, sizeof *out);
    out->size = c.size;
    out->lowest_index = c.lowest;
    out->total_jsd = c.total_jsd;
    out->mean_delta_jsd = c.mean_delta;
    out->std_delta_jsd = c.std_delta;
    out->cov_delta_jsd = c.cov_delta;
    out->summed_entropies = c.sum_entropy;
    out->rows_scored = c.rows_scored;
    out->rows_rechecked = c.rows_rechecked;
    out->n_windows = c.n_windows;
    out->n_events = c.n_events;
    out->n_accepts = c.n_accepts;
    out->n_arbitrated = s->n_arbitrated;
    out->scan_ms = s->scan_ms;
    out->scan_launches = s->scan_launches;
    out->engine = s->persist.on ? 1u : 0u;
    out->rows_coarse_passed = uint32_t(std::min<unsigned long long>(c.rows_coarse_passed, 0xFFFFFFFFull));
    out->scan_ms_last = s->scan_ms_last;
    out->rows_scored_last = s->persist.on ? c.rows_scored - std::min(c.rows_before_launch, c.rows_scored) : 0;
    out->arbiter_ms = s->arbiter_ms;
    return DVS_OK;
}

extern "C" int dvs_select_get_members(dvs_ctx *ctx, const dvs_select *s, uint64_t *positions,
                                      uint32_t *labels, double *delta_jsd, double *entropy,
                                      double *freqs) {
    if (!s) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    const uint32_t n = s->h_ctl->size;
    const uint64_t B = s->dev.B;
    std::vector<uint32_t> ord(n), lab(s->cap);
    std::vector<uint64_t> pos(s->cap);
    std::vector<double> mh(s->cap);
    DVS_HIP(ctx, hipMemcpy(ord.data(), s->dev.ord, size_t(n) * 4, hipMemcpyDeviceToHost));
    DVS_HIP(ctx, hipMemcpy(lab.data(), s->dev.mLabel, size_t(s->cap) * 4, hipMemcpyDeviceToHost));
    DVS_HIP(ctx, hipMemcpy(pos.data(), s->dev.mPos, size_t(s->cap) * 8, hipMemcpyDeviceToHost));
    DVS_HIP(ctx, hipMemcpy(mh.data(), s->dev.mH, size_t(s->cap) * 8, hipMemcpyDeviceToHost));
    if (delta_jsd)  // mDelta is indexed by member order already
        DVS_HIP(ctx, hipMemcpy(delta_jsd, s->dev.mDelta, size_t(n) * 8, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t sl = ord[i];
        if (positions) positions[i] = pos[sl];
        if (labels) labels[i] = s->h_out_labels.empty() ? lab[sl] : s->h_out_labels[pos[sl]];
        if (entropy) entropy[i] = mh[sl];
        if (freqs)
            DVS_HIP(ctx, hipMemcpy(freqs + uint64_t(i) * B, s->dev.M + uint64_t(sl) * B, B * 8,
                                   hipMemcpyDeviceToHost));
    }
    return DVS_OK;
}

extern "C" int dvs_select_delta_jsd(dvs_ctx *ctx, const dvs_select *s, const dvs_matrix *q,
                                    const uint32_t *qlabels, double *out) {
    if (!s || !q || !out) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (q->nbins != s->dev.B)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "query matrix has %llu bins, the set %llu",
                             (unsigned long long)q->nbins, (unsigned long long)s->dev.B);
    if (q->nrows == 0) return DVS_OK;
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    double *d_out = nullptr;
    uint32_t *d_lab = nullptr;
    std::vector<uint32_t> qtrans;
    if (qlabels && !s->h_out_labels.empty()) {
        // label-free engine: a query carrying a member's (caller) label gets that member's engine
        // label (its stream position), any other query none
        const uint32_t n = s->h_ctl->size;
        std::vector<uint64_t> pos(s->cap);
        std::vector<uint32_t> ord(n);
        DVS_HIP(ctx, hipMemcpy(ord.data(), s->dev.ord, size_t(n) * 4, hipMemcpyDeviceToHost));
        DVS_HIP(ctx, hipMemcpy(pos.data(), s->dev.mPos, size_t(s->cap) * 8, hipMemcpyDeviceToHost));
        std::map<uint32_t, uint32_t> member_of;
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t p = pos[ord[i]];
            if (s->h_out_labels[p] != 0xFFFFFFFFu) member_of[s->h_out_labels[p]] = uint32_t(p);
        }
        qtrans.resize(q->nrows);
        for (uint32_t i = 0; i < q->nrows; i++) {
            auto it = member_of.find(qlabels[i]);
            qtrans[i] = it == member_of.end() ? 0xFFFFFFFFu : it->second;
        }
        qlabels = qtrans.data();
    }
    // (blocks of the context's cache; whatever fails once something is enqueued, the stream is waited for before they go back)
    PooledBuf b_out{ctx}, b_lab{ctx};
    if (int rc = dvs_dev_alloc(ctx, &b_out.p, size_t(q->nrows) * 8, "query scores")) return rc;
    if (qlabels)
        if (int rc = dvs_dev_alloc(ctx, &b_lab.p, size_t(q->nrows) * 4, "query labels")) return rc;
    d_out = b_out.as<double>();
    d_lab = b_lab.as<uint32_t>();
    hipError_t e = hipSuccess;
    if (qlabels) e = hipMemcpyAsync(d_lab, qlabels, size_t(q->nrows) * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        dvs_mat_dispatch(q, [&](auto *qp) {
            using T = std::remove_cv_t<std::remove_pointer_t<decltype(qp)>>;
            hipLaunchKernelGGL((score_kernel<T>), dim3(q->nrows), dim3(LOO_THREADS), 0, ctx->stream, s->dev, qp,
                               q->d_totals, q->d_entropy, d_lab, d_out);
            return 0;
        });
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, size_t(q->nrows) * 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t se = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, "dvs_select_delta_jsd");
    return DVS_OK;
}

// Measurement aid: ONE scan_kernel launch over every streamed row against the set's current
// state with an unreachable threshold (no events), timed with HIP events on the ctx stream.
// This is the steady-state streaming rate of the scan arithmetic, without the greedy chain's
// per-event latencies.  The selection's state is not touched (a scratch control block is used).
extern "C" int dvs_select_bench_scan(dvs_ctx *ctx, const dvs_select *s, int repeats, double *ms_out,
                                     uint64_t *rows_out) {
    if (!ctx || !s || !ms_out || !rows_out || repeats < 1)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "bad argument");
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    SelCtl c = *s->h_ctl;
    const uint64_t first = s->params.n_seed;
    if (s->npos <= first) return dvs_set_error(ctx, DVS_ERR_VALUE, "nothing to scan");
    c.status = SEL_RUN;
    c.cursor = first;
    c.window = uint32_t(std::min<uint64_t>(s->npos - first, 0xFFFFFFFFull));
    c.event_pos = SEL_NONE;
    c.thr = 1e300;
    c.ev_kind = 0;
    SelCtl *d_c = nullptr;
    uint32_t *d_rows = nullptr;
    int rc = dvs_dev_alloc(ctx, (void **)&d_c, sizeof(SelCtl), "scratch control block");
    if (!rc) rc = dvs_dev_alloc(ctx, (void **)&d_rows, size_t(s->scan_grid) * 8, "scratch row counters");
    if (rc) {
        dvs_dev_free(ctx, d_c);
        return rc;
    }
    hipEvent_t e0 = dvs_event_get(ctx), e1 = dvs_event_get(ctx);
    auto launch = [&]() {
        dvs_mat_dispatch(s->mat, [&](auto *mp) {
            launch_scan(s, mp, s->scan_hot, d_c, d_rows, ctx->stream);
            return 0;
        });
    };
    hipError_t e = hipMemcpyAsync(d_c, &c, sizeof c, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_rows, 0, size_t(s->scan_grid) * 8, ctx->stream);
    launch();  // warm-up
    if (e == hipSuccess) e = hipEventRecord(e0, ctx->stream);
    for (int i = 0; i < repeats; i++) launch();
    if (e == hipSuccess) e = hipEventRecord(e1, ctx->stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e == hipSuccess) e = hipGetLastError();
    dvs_event_put(ctx, e0);
    dvs_event_put(ctx, e1);
    dvs_dev_free(ctx, d_c);
    dvs_dev_free(ctx, d_rows);
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, "scan benchmark");
    *ms_out = double(ms) / repeats;
    *rows_out = s->npos - first;
    return DVS_OK;
}

// Members in set order into caller-provided DEVICE buffers: rows[cap_rows x nbins] and
// meta[cap_rows x 2] = (stream position, 1.0) -- rows beyond the set's size are zeroed with
// meta (0, 0).  Enqueued on the ctx stream; the caller orders it against its own streams.
extern "C" int dvs_select_gather_members(dvs_ctx *ctx, const dvs_select *s, double *d_rows, double *d_meta,
                                         uint32_t cap_rows) {
    if (!ctx || !s || !d_rows || !d_meta) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (cap_rows < s->h_ctl->size)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "buffer of %u rows for a set of %u", cap_rows, s->h_ctl->size);
    if (!cap_rows) return DVS_OK;
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(gather_members_kernel, dim3(cap_rows), dim3(LOO_THREADS), 0, ctx->stream, s->dev,
                       d_rows, d_meta);
    DVS_HIP(ctx, hipGetLastError());
    return DVS_OK;
}
