// The MODE_MAX batch pair of the multi-launch selection engine (select.hip sel_run_loop launches it in front of its
// ordinary iterations).
#include "dvs_internal.h"
#include "select.h"
#include "select_dev.h"

#include <algorithm>
#include <type_traits>

namespace {

// ---- MODE_MAX while the set may grow: a BATCH of rows against the unchanged set.
// A tentative push that is rolled back leaves the set as it was (records.rs:439-450), and so does a row that
// is no event: the rows from the cursor up to the next push that is KEPT all face the same set.  Where
// events come back to back (genome collections: nearly every row is one, one in fifty is kept) the iteration
// above -- five launches and ~130 us per event -- walks them one by one.  These two kernels take MB_ROWS rows
// at once: max_batch_jobs works out, for every row, its own increases_jsd score and the leave-one-out pass
// of the bigger set (one workgroup per row and member), max_batch_decide takes the decisions (the
// arithmetic and the bands of resolve / finalize) and moves the cursor over the rows that are NOT events or
// whose push is clearly rolled back -- nothing else: the first row that would be kept, or that is too close
// to call, stays where it is, and the ordinary iteration behind the pair deals with it (commit, arbiter).
// The persistent engine has the same thing in-kernel (persist.hip); this one has no limits on 4^k or the set.
constexpr uint32_t MB_ROWS = 32;
constexpr int MB_THREADS = 256;
constexpr uint32_t MB_MAX_MEMBERS = 4096;  // sets up to this size (the result block is 3 x MB_ROWS x (this + 3) doubles)

__device__ __forceinline__ bool max_batch_applies(const SelCtl *ctl, const SelDev &d, uint32_t JW) {
    return ctl->status == SEL_RUN && ctl->ev_kind == 0 && ctl->mode == DVS_MODE_MAX && ctl->size < ctl->max_size &&
           ctl->s_is_resum != 0 && ctl->forced == FORCE_NONE && !d.gather_all && ctl->size + 3 <= JW && ctl->size >= 2 &&
           ctl->mb_stuck == 0;
}

// One workgroup: ONE member r (or the whole bigger set, or the score) and MB_RG consecutive rows of the batch --
// S and the member's row are read once for the group, and what differs per row is the candidate's counts.  The
// jobs only steer the cursor over rows that change nothing (anything inside a band stops the batch), so their
// quotients are the exact ones by fma (exact_div_u32) and the means multiply by reciprocals, like the persistent
// engine's batches (persist.hip): two f64 divisions per bin fewer -- the kernel was bound by them (4^7 bins, 117
// members, 32 rows: 150 us, ~100 vector instructions per bin).
constexpr uint32_t MB_RG = 2;
static_assert(MB_ROWS % MB_RG == 0, "whole groups");
template <typename T>
__global__ __launch_bounds__(MB_THREADS) void max_batch_jobs_kernel(SelDev d, const T *__restrict__ mat,
                                                                    double *__restrict__ res, uint32_t JW) {
    __shared__ double scratch[48];
    __shared__ double2 ltab[128];  // log2_tab's table (select_dev.h): ~18 instead of ~33 instructions per logarithm
    const SelCtl *ctl = d.ctl;
    if (!max_batch_applies(ctl, d, JW)) return;
    const uint32_t n = ctl->size, r = blockIdx.x, e0 = blockIdx.y * MB_RG;
    if (r >= n + 3) return;
    if (threadIdx.x < 128) log2_tab_fill(ltab, threadIdx.x);
    __syncthreads();
    // the group's rows (the same answers in every thread: the branches below are uniform)
    const T *rp[MB_RG];
    double tot[MB_RG], rt[MB_RG];
    bool live[MB_RG], any = false;
#pragma unroll
    for (uint32_t q = 0; q < MB_RG; q++) {
        const uint64_t p = ctl->cursor + e0 + q;
        live[q] = false;
        rp[q] = mat;
        tot[q] = rt[q] = 1.0;
        if (p >= ctl->npos) continue;
        const uint32_t row = d.order ? d.order[p] : uint32_t(p);
        const uint32_t lab = d.labels ? d.labels[p] : row;
        if (lab < d.nlabels && d.inset[lab]) continue;  // a member already: no event (records.rs:71-74,87-89)
        const uint32_t toti = d.totals[row];
        if (toti == 0) continue;  // no valid k-mer: the stream skips the row (records.rs:419-423)
        live[q] = any = true;
        rp[q] = mat + uint64_t(row) * d.B;
        tot[q] = double(toti);
        rt[q] = 1.0 / tot[q];
    }
    if (!any) return;
    Ent en[MB_RG];
    // Four bins a thread per pass: S, the second row and the rows' counts are requested together, then the
    // arithmetic -- every row's terms still in bin order (i, i + 256, ...), as the one-bin loop adds them.
    auto run = [&](const double *second, auto term) {
        constexpr int U = 4;
        uint64_t i = threadIdx.x;
        for (; i + uint64_t(U - 1) * MB_THREADS < d.B; i += uint64_t(U) * MB_THREADS) {
            double sv[U], mv[U];
            T c[MB_RG][U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                sv[u] = d.S[i + uint64_t(u) * MB_THREADS];
                mv[u] = second ? second[i + uint64_t(u) * MB_THREADS] : 0.0;
            }
#pragma unroll
            for (uint32_t q = 0; q < MB_RG; q++)
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (live[q]) c[q][u] = rp[q][i + uint64_t(u) * MB_THREADS];
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (uint32_t q = 0; q < MB_RG; q++)
                    if (live[q]) en[q].add(term(sv[u], mv[u], count_freq_x(c[q][u], tot[q], rt[q])), ltab);
        }
        for (; i < d.B; i += MB_THREADS) {
            const double sv = d.S[i], mv = second ? second[i] : 0.0;
#pragma unroll
            for (uint32_t q = 0; q < MB_RG; q++)
                if (live[q]) en[q].add(term(sv, mv, cand_freq_x(rp[q], i, tot[q], rt[q])), ltab);
        }
    };
    if (r == n + 2) {  // increases_jsd: block_delta_jsd's arithmetic
        const double rn = 1.0 / double(n);
        run(d.M + uint64_t(d.ord[ctl->lowest]) * d.B, [&](double sv, double lowv, double f) { return ((sv - lowv) + f) * rn; });
    } else if (r == n + 1) {  // the bigger set as a whole (resolve_body: Stmp = S + candidate, H(Stmp / (n + 1)))
        const double rn1 = 1.0 / double(n + 1);
        run(nullptr, [&](double sv, double, double f) { return (sv + f) * rn1; });
    } else if (r < n) {  // without member r (loo_body)
        const double rdiv = 1.0 / double(n);
        run(d.M + uint64_t(d.ord[r]) * d.B, [&](double sv, double mv, double f) {
            double v = ((sv + f) - mv) * rdiv;  // updated_mean_freqs, records.rs:276-286
            return v <= DVS_EPS ? 0.0 : v;
        });
    } else {  // r == n: without the candidate itself
        const double rdiv = 1.0 / double(n);
        run(nullptr, [&](double sv, double, double f) {
            double v = ((sv + f) - f) * rdiv;
            return v <= DVS_EPS ? 0.0 : v;
        });
    }
#pragma unroll
    for (uint32_t q = 0; q < MB_RG; q++) {
        if (!live[q]) continue;
        double h = en[q].h, mn = en[q].mn, sm = en[q].sum;
        block_red3(h, mn, sm, scratch);
        if (threadIdx.x == 0) {
            const uint32_t e = e0 + q;
            res[(uint64_t(e) * 3 + 0) * JW + r] = h;
            res[(uint64_t(e) * 3 + 1) * JW + r] = sm;
            res[(uint64_t(e) * 3 + 2) * JW + r] = mn;
        }
    }
}

__global__ __launch_bounds__(WIDE_THREADS) void max_batch_decide_kernel(SelDev d, const double *__restrict__ res, uint32_t JW) {
    __shared__ double s_kind[MB_ROWS], s_counted[MB_ROWS];
    SelCtl *ctl = d.ctl;
    if (!max_batch_applies(ctl, d, JW)) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwave = WIDE_THREADS / 64;
    const uint32_t n = ctl->size, n1 = n + 1;
    const uint64_t p0 = ctl->cursor;
    const uint32_t nrows = uint32_t(umin64(MB_ROWS, ctl->npos - p0));
    const double dn = double(n), dn1 = double(n1);
    for (uint32_t e = wave; e < nrows; e += nwave) {
        // kind: 0 the stream moves on (no event, or a push that is clearly rolled back), 2 it stops here (a push
        // that would be kept, or anything too close to call)
        double kind = 0.0, counted = 0.0;
        const uint64_t p = p0 + e;
        const uint32_t row = d.order ? d.order[p] : uint32_t(p);
        const uint32_t lab = d.labels ? d.labels[p] : row;
        const bool dead = (lab < d.nlabels && d.inset[lab]) || d.totals[row] == 0;
        if (!dead) {
            const double H_e = d.rowH[row];
            const double *re = res + uint64_t(e) * 3 * JW;
            const double hs = re[n + 2], ss = re[JW + n + 2], ms = re[2 * JW + n + 2];
            const double jsd = (ms < 0.0) ? NAN : hs - (ctl->he_base + H_e) / dn;  // block_delta_jsd
            counted = 1.0;
            if (sum_risky(ss, d.B) || fabs(jsd - ctl->thr) <= ctl->band) {
                kind = 2.0;
                counted = 0.0;
            } else if (jsd > ctl->thr) {  // an event: the tentative push (resolve_body, loo_body, finalize_body)
                const double sumH_t = ctl->sum_entropy + H_e;
                const double hm = re[n1], svm = re[JW + n1];
                const double tj = hm - sumH_t / dn1;
                const double div = dn1 - 1.0;
                auto delta = [&](uint32_t r) {
                    const double mh = r < n ? d.mH[d.ord[r]] : H_e;
                    return tj - (re[r] - (sumH_t - mh) / div);
                };
                // (a lane's first four members' deltas stay in registers for the second and third pass -- every delta is
                // two dependent global loads, and sets of up to 256 members need no more; the same values either way)
                constexpr uint32_t KEEP = 4;
                double kept[KEEP];
                auto delta_again = [&](uint32_t r) {
                    const uint32_t q = (r - lane) >> 6;
                    double v = 0.0;
                    bool have = false;
#pragma unroll
                    for (uint32_t x = 0; x < KEEP; x++)
                        if (q == x) {
                            v = kept[x];
                            have = true;
                        }
                    return have ? v : delta(r);
                };
                double best = 1e6, acc = 0.0;
                bool risky = sum_risky(svm, d.B) || !(hm == hm);
#pragma unroll
                for (uint32_t x = 0; x < KEEP; x++) kept[x] = 0.0;
                for (uint32_t r = lane; r < n1; r += 64) {
                    const double v = delta(r);
                    const uint32_t q = (r - lane) >> 6;
#pragma unroll
                    for (uint32_t x = 0; x < KEEP; x++)
                        if (q == x) kept[x] = v;
                    risky |= sum_risky(re[JW + r], d.B);
                    acc += v;
                    if (v < best) best = v;
                }
                const double dmin = dvs_wave_min(best);
                double fi = 4294967295.0;
                for (uint32_t r = lane; r < n1; r += 64)
                    if (dmin < 1e6 && delta_again(r) == dmin) fi = fmin(fi, double(r));
                const double dfirst = dvs_wave_min(fi);
                const uint32_t lowest = (dfirst < 4294967295.0) ? uint32_t(dfirst) : 0u;
                const double mean = dvs_wave_sum(acc) / dn1;
                double second = 1e6, tv = 0.0;
                for (uint32_t r = lane; r < n1; r += 64) {
                    const double v = delta_again(r);
                    if (r != lowest && v < second) second = v;
                    const double t = v - mean;
                    tv += t * t;
                }
                const double dsecond = dvs_wave_min(second);
                const double sd = sqrt(dvs_wave_sum(tv) / (dn1 - 1.0));
                const double cov = sd / mean;
                const bool any_risky = __ballot(risky) != 0ull;
                const double band = sel_band(tj + sumH_t / dn1, d.B);
                const double a = ctl->stat == DVS_STAT_STDEV ? sd : cov;
                const double b = ctl->stat == DVS_STAT_STDEV ? ctl->std_delta : ctl->cov_delta;
                const double mm = fmin(fabs(mean), fabs(ctl->mean_delta));
                const double sband = ctl->stat == DVS_STAT_STDEV
                                         ? 4.0 * band
                                         : 4.0 * band * (1.0 + fmax(fabs(a), fabs(b))) / fmax(mm, 1e-300);
                const bool tie = any_risky || (dsecond - dmin <= band && dsecond < 1e6) || !(fabs(a - b) > sband);
                if (tie || a > b) {  // too close to call, or a push that is kept: the ordinary iteration's
                    kind = 2.0;
                    counted = 0.0;
                }
            }
        }
        if (lane == 0) {
            s_kind[e] = kind;
            s_counted[e] = counted;
        }
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t stop = nrows, events = 0;
        for (uint32_t e = 0; e < nrows; e++) {
            if (s_kind[e] == 2.0) {
                stop = e;
                break;
            }
            events += s_counted[e] != 0.0;
        }
        // (a batch that stopped in front of a row leaves that row to the ordinary iteration; the batch pairs
        // queued behind this one return at once until finalize has dealt with it)
        if (stop < nrows) ctl->mb_stuck = 1;
        if (stop > 0) {
            ctl->cursor = p0 + stop;
            ctl->mb_rows += stop;
            ctl->n_events += events;
            ctl->n_windows++;
            ctl->rows_scored += stop;
            ctl->event_pos = SEL_NONE;
            if (ctl->cursor >= ctl->npos) ctl->status = SEL_DONE;
            ctl_next_window(ctl);
        }
    }
}

}  // namespace

// the batch pair in front of an ordinary iteration (MODE_MAX while the set may grow and events are dense);
// size_bound: no set this launch can meet is larger
int dvs_max_batch_launch(dvs_ctx *ctx, dvs_select *s, uint32_t size_bound) {
    if (!s->mb.d_res) {
        s->mb.jw = std::min<uint32_t>(s->cap, MB_MAX_MEMBERS) + 3;
        int rc = dvs_dev_alloc(ctx, (void **)&s->mb.d_res, size_t(3) * MB_ROWS * s->mb.jw * sizeof(double), "max batch results");
        if (rc) return rc;
    }
    if (size_bound + 3 > s->mb.jw) return DVS_OK;  // (a set beyond the result block: the ordinary iterations alone)
    dvs_mat_dispatch(s->mat, [&](auto *mp) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(mp)>>;
        hipLaunchKernelGGL((max_batch_jobs_kernel<T>), dim3(size_bound + 3, MB_ROWS / MB_RG), dim3(MB_THREADS), 0, ctx->stream, s->dev, mp,
                           s->mb.d_res, s->mb.jw);
        return 0;
    });
    hipLaunchKernelGGL(max_batch_decide_kernel, dim3(1), dim3(WIDE_THREADS), 0, ctx->stream, s->dev, s->mb.d_res, s->mb.jw);
    s->mb.launched++;
    return DVS_OK;
}

void dvs_max_batch_free(dvs_select *s) { dvs_dev_free(s->ctx, s->mb.d_res); }
