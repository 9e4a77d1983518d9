// The three scan tiers of the persistent engine (persist.hip): a row per wave, a row per workgroup, and the
// streamed row per workgroup.
#pragma once

#include "persist_dev.h"

namespace {

// One wave's share of the window, as scan_rows_hot but against the unscaled vector sl:
// x = (sl_i + c_i / T) / n  computed as  fma(c, 1/T, sl) * (1/n).
template <typename T, bool COARSE>
__device__ __forceinline__ void p_scan_rows(const T *__restrict__ mat,
                                            const uint32_t *__restrict__ totals,
                                            const double *__restrict__ rowH, const double *sl,
                                            const float *slf, uint64_t B, const PState &st, double he_base,
                                            const PWin &win,
                                            uint64_t first, uint64_t stride, uint64_t nrows,
                                            uint32_t lane, uint32_t &nread,
                                            uint32_t &nprecise, uint32_t &nmid, bool coarse_on,
                                            bool burst_drop = true) {
    const double dn = double(st.n), rn = 1.0 / dn;
    const double thr_lo = st.thr - st.band;
    const double thr_fast = thr_lo - FAST_BAND, thr_sure = st.thr + st.band + FAST_BAND;
    (void)thr_lo;
    const bool vec = (B & 255) == 0;
    const double cband = coarse_band(B);
    const double thr_c_lo = st.thr - st.band - cband, thr_c_hi = st.thr + st.band + cband;
    for (uint64_t r = first; r < nrows; r += stride) {
        const uint64_t p = st.cursor + r;
        const T *rp = mat + p * B;
        const uint64_t ev = p_hint_pos(win);
        const uint32_t tot = totals[p];
        const double hrow = rowH[p];
        if (ev < p) break;
        if (tot == 0) continue;
        const double rt = 1.0 / double(tot);
        const double mean_entropy = (he_base + hrow) / dn;
        nread++;
        if constexpr (COARSE) {
            if (vec && coarse_on) {  // COARSE tier: decides every row farther than cband from the threshold
                const float rtn = float(rt * rn);
                const dvs_f2 r2 = {rtn, rtn};
                double c0 = 0.0, c1 = 0.0;
                bool done16 = false;
                if constexpr (sizeof(T) == 2) {
                    // 16-bit rows of 4096 bins: eight 16-byte loads per lane (lane l owns bins
                    // 512 j + 8 l .. + 7), the whole 8 KiB row requested at once.  (Requesting it beside the
                    // look at the event word instead of behind it -- all of it, half, a quarter -- measured
                    // the same step and event-free pass, and half again as much traffic for rows dropped.)
                    if (B == 4096) {
                        uint4 raw8[8];
#pragma unroll
                        for (int j = 0; j < 8; j++) raw8[j] = *reinterpret_cast<const uint4 *>(rp + j * 512 + lane * 8);
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int j = 0; j < 8; j++) {
                            asm volatile("" : "+v"(raw8[j].x), "+v"(raw8[j].y), "+v"(raw8[j].z), "+v"(raw8[j].w));
                            coarse8(raw8[j], slf + j * 512 + lane * 8, r2, c0, c1);
                        }
                        done16 = true;
                    }
                }
                if (!done16) {
                // Bursts of C_CH chunks: 4 KiB of a row requested at a time keep the memory pipe as full
                // as 16 KiB do (scripts/micro/stream_read.hip), and a row that an earlier event has made
                // pointless is dropped at the next burst with its other bytes never requested.
                constexpr int C_CH = sizeof(T) == 2 ? 16 : 8;  // (16-bit rows: the same bytes per burst)
                const uint64_t full = B - B % (256 * C_CH);
                uint64_t i0 = 0;
                bool dropped = false;
                for (; i0 < full; i0 += 256 * C_CH) {
                    if (i0 && burst_drop && p_hint_pos(win) < p) {
                        dropped = true;
                        break;
                    }
                    Raw4<T> raw[C_CH];
#pragma unroll
                    for (int j = 0; j < C_CH; j++) raw[j].load(rp + i0 + uint64_t(j) * 256 + lane * 4);
                    // (the scheduler would otherwise sink each load to its use: one 1 KiB request in
                    // flight per wave instead of four)
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int j = 0; j < C_CH; j += 2) {
                        const uint64_t i = i0 + uint64_t(j) * 256 + lane * 4;
                        raw[j].pin();  // nothing of chunk j is consumed (converted) above this point
                        raw[j + 1].pin();
                        c0 += double(coarse4(raw[j].c, *reinterpret_cast<const float4 *>(slf + i), r2));
                        c1 += double(coarse4(raw[j + 1].c, *reinterpret_cast<const float4 *>(slf + i + 256), r2));
                    }
                }
                if (dropped) {  // (an earlier event exists: this wave's later rows are pointless too)
                    nread--;    // not a row scored: it does not count towards the algorithmic bytes
                    break;
                }
                for (; i0 < B; i0 += 256) {
                    const uint64_t i = i0 + lane * 4;
                    Raw4<T> raw;
                    raw.load(rp + i);
                    c0 += double(coarse4(raw.c, *reinterpret_cast<const float4 *>(slf + i), r2));
                }
                }  // !done16
                const double jf0 = -dvs_wave_sum_dpp(c0 + c1) - mean_entropy;
                if (!(jf0 > thr_c_lo)) continue;  // (NaN: a negative bin, rejected as the reference does)
                if (jf0 > thr_c_hi) {
                    p_post_event_wave(win, p, true, lane);
                    continue;
                }
                nmid++;
            }
        }
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, xmin = 0.0;
        if (vec) {
            // (behind the COARSE tier this pass sees a few dozen rows per selection: half the burst, half the registers)
            constexpr int F_CH = COARSE ? P_CH / 2 : P_CH;
            const uint64_t full = B - B % (256 * F_CH);
            uint64_t i0 = 0;
            for (; i0 < full; i0 += 256 * F_CH) {  // F_CH chunks of 1 KiB per wave instruction per burst
                Raw4<T> raw[F_CH];
#pragma unroll
                for (int j = 0; j < F_CH; j++) raw[j].load(rp + i0 + uint64_t(j) * 256 + lane * 4);
#pragma unroll
                for (int j = 0; j < F_CH; j++) {
                    const uint64_t i = i0 + uint64_t(j) * 256 + lane * 4;
                    const double2 b01 = *reinterpret_cast<const double2 *>(sl + i);
                    const double2 b23 = *reinterpret_cast<const double2 *>(sl + i + 2);
                    double v0, v1, v2, v3;
                    raw[j].get(v0, v1, v2, v3);
                    const double x0 = fma(v0, rt, b01.x) * rn, x1 = fma(v1, rt, b01.y) * rn;
                    const double x2 = fma(v2, rt, b23.x) * rn, x3 = fma(v3, rt, b23.y) * rn;
                    a0 += fast_neg_xlog2x(x0);
                    a1 += fast_neg_xlog2x(x1);
                    a2 += fast_neg_xlog2x(x2);
                    a3 += fast_neg_xlog2x(x3);
                    xmin = fmin(fmin(xmin, fmin(x0, x1)), fmin(x2, x3));
                }
            }
            for (; i0 < B; i0 += 256) {
                const uint64_t i = i0 + lane * 4;
                double v0, v1, v2, v3;
                load4(rp, i, v0, v1, v2, v3);
                const double2 b01 = *reinterpret_cast<const double2 *>(sl + i);
                const double2 b23 = *reinterpret_cast<const double2 *>(sl + i + 2);
                const double x0 = fma(v0, rt, b01.x) * rn, x1 = fma(v1, rt, b01.y) * rn;
                const double x2 = fma(v2, rt, b23.x) * rn, x3 = fma(v3, rt, b23.y) * rn;
                a0 += fast_neg_xlog2x(x0);
                a1 += fast_neg_xlog2x(x1);
                a2 += fast_neg_xlog2x(x2);
                a3 += fast_neg_xlog2x(x3);
                xmin = fmin(fmin(xmin, fmin(x0, x1)), fmin(x2, x3));
            }
        } else {
            for (uint64_t i = lane; i < B; i += 64) {
                const double x = fma(row_value(rp, i), rt, sl[i]) * rn;
                a0 += fast_neg_xlog2x(x);
                xmin = fmin(xmin, x);
            }
        }
        const double hf = dvs_wave_sum((a0 + a1) + (a2 + a3));
        const double mn = dvs_wave_min(xmin);
        const double jf = hf - mean_entropy;
        if (!(mn < 0.0) && jf > thr_sure) {
            // above the threshold by more than every error bound: no f64 re-evaluation needed
            p_post_event_wave(win, p, true, lane);
        } else if (!(mn < 0.0) && jf > thr_fast && lane == 0) {
            {
                // within FAST_BAND of the threshold: listed, not an event -- the scan goes on and
                // the workgroups settle it in f64 after the rendezvous (a wave doing that alone
                // would hold the whole grid at the barrier for 4^k f64 logarithms)
                nprecise++;
                p_list_candidate(win, p);
            }
        }
    }
}

// The same scores with one row per WORKGROUP (8 waves x 512 bins at k=6): a row takes an eighth of
// the time a lone wave needs for it, so a short window -- early in the stream an accept comes every
// few hundred rows and the scan is pure latency -- ends that much sooner, and the rows in flight
// when an event is found are 255, not 2040.  One barrier per row: the waves' partial sums alternate
// between two sets of LDS slots.  Lane l of wave w owns bins 4 (512 c + 64 w + l) .. + 3 of every
// 2048-bin chunk c.  red: 2 x 24 doubles.
template <typename T, bool COARSE>
__device__ __forceinline__ void p_scan_rows_wg(const T *__restrict__ mat, const uint32_t *__restrict__ totals,
                                               const double *__restrict__ rowH, const double *sl,
                                               const float *slf, uint64_t B,
                                               const PState &st, double he_base, const PWin &win,
                                               uint64_t first, uint64_t stride,
                                               uint64_t nrows, double *red, uint32_t &nread,
                                               uint32_t &nprecise, uint32_t &nmid, bool coarse_on,
                                            bool burst_drop = true) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double dn = double(st.n), rn = 1.0 / dn;
    const double thr_fast = st.thr - st.band - FAST_BAND, thr_sure = st.thr + st.band + FAST_BAND;
    const bool vec = (B & 2047) == 0;
    const double cband = coarse_band(B);
    const double thr_c_lo = st.thr - st.band - cband, thr_c_hi = st.thr + st.band + cband;
    uint32_t par = 0;
    for (uint64_t r = first; r < nrows; r += stride, par ^= 1) {
        const uint64_t p = st.cursor + r;
        const T *rp = mat + p * B;
        const uint64_t ev = wave == 0 ? p_hint_pos(win) : 0ull;
        const uint32_t tot = totals[p];
        const double hrow = rowH[p];
        const double rt = tot ? 1.0 / double(tot) : 0.0;
        if constexpr (COARSE) {
            if (vec && B <= 4 * 2048 && coarse_on) {  // COARSE tier first (select_dev.h); its sums use red[48..]
                const float rtn = float(rt * rn);
                const dvs_f2 r2 = {rtn, rtn};
                double c0 = 0.0;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint64_t i = uint64_t(j) * 2048 + tid * 4;
                    if (i < B) {
                        Raw4<T> raw;
                        raw.load(rp + i);
                        c0 += double(coarse4(raw.c, *reinterpret_cast<const float4 *>(slf + i), r2));
                    }
                }
                c0 = dvs_wave_sum_dpp(c0);
                double *cslot = red + 48 + par * 16;
                if (lane == 0) {
                    cslot[wave] = c0;
                    if (wave == 0) cslot[8] = __longlong_as_double((long long)ev);
                }
                __syncthreads();
                if ((unsigned long long)__double_as_longlong(cslot[8]) < p) break;
                if (tot == 0) continue;
                double hc = 0.0;
#pragma unroll
                for (int w = 0; w < P_THREADS / 64; w++) hc += cslot[w];
                const double jf0 = -hc - (he_base + hrow) / dn;
                if (tid == 0) nread++;
                if (!(jf0 > thr_c_lo)) continue;
                if (jf0 > thr_c_hi) {
                    if (tid < 8) p_post_event_wave(win, p, true, tid);  // (eight lanes, one instruction: every thread knows the score)
                    continue;
                }
                if (tid == 0) {
                    nmid++;
                    nread--;  // counted again below
                }
            }
        }
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, xmin = 0.0;
        if (vec) {
            for (uint64_t i0 = 0; i0 < B; i0 += 4 * 2048) {  // up to four chunks requested at once
                Raw4<T> raw[4];
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (i0 + uint64_t(j) * 2048 < B) raw[j].load(rp + i0 + uint64_t(j) * 2048 + tid * 4);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint64_t i = i0 + uint64_t(j) * 2048 + tid * 4;
                    if (i < B) {
                        const double2 b01 = *reinterpret_cast<const double2 *>(sl + i);
                        const double2 b23 = *reinterpret_cast<const double2 *>(sl + i + 2);
                        double v0, v1, v2, v3;
                        raw[j].get(v0, v1, v2, v3);
                        const double x0 = fma(v0, rt, b01.x) * rn, x1 = fma(v1, rt, b01.y) * rn;
                        const double x2 = fma(v2, rt, b23.x) * rn, x3 = fma(v3, rt, b23.y) * rn;
                        a0 += fast_neg_xlog2x(x0);
                        a1 += fast_neg_xlog2x(x1);
                        a2 += fast_neg_xlog2x(x2);
                        a3 += fast_neg_xlog2x(x3);
                        xmin = fmin(fmin(xmin, fmin(x0, x1)), fmin(x2, x3));
                    }
                }
            }
        } else {
            for (uint64_t i = tid; i < B; i += P_THREADS) {
                const double x = fma(row_value(rp, i), rt, sl[i]) * rn;
                a0 += fast_neg_xlog2x(x);
                xmin = fmin(xmin, x);
            }
        }
        const double hw = dvs_wave_sum((a0 + a1) + (a2 + a3));
        const bool negw = __ballot(xmin < 0.0) != 0ull;
        double *slot = red + par * 24;
        if (lane == 0) {
            slot[wave] = hw;
            slot[8 + wave] = negw ? 1.0 : 0.0;
            if (wave == 0) slot[16] = __longlong_as_double((long long)ev);
        }
        __syncthreads();
        // every thread takes the same decisions from the same LDS words
        if ((unsigned long long)__double_as_longlong(slot[16]) < p) break;
        if (tot == 0) continue;
        double hf = 0.0, neg = 0.0;
#pragma unroll
        for (int w = 0; w < P_THREADS / 64; w++) {
            hf += slot[w];
            neg += slot[8 + w];
        }
        const double jf = hf - (he_base + hrow) / dn;
        // (a sure event goes out from eight lanes in one instruction: every thread knows the score)
        if (tid < 8 && neg == 0.0 && jf > thr_fast && jf > thr_sure) p_post_event_wave(win, p, true, tid);
        if (tid == 0) {
            nread++;
            if (neg == 0.0 && jf > thr_fast) {
                if (jf > thr_sure) {
                } else {
                    nprecise++;
                    p_list_candidate(win, p);
                }
            }
        }
    }
}

// The row-per-workgroup scan as a stream (4^k = 4096 bins, COARSE tier): every thread keeps the
// two 16-byte requests of each of the next D rows of its workgroup in flight, so the grid streams
// rows at memory speed while an event still leaves only ~one row per workgroup to drain.  A row the
// COARSE tier cannot decide is scored again by p_scan_rows_wg (FAST tier) as a one-row window.
// red: the 128-double scratch area minus its first 32 (slots [48..80) are this function's).
template <typename T>
__device__ __forceinline__ void p_scan_rows_wg_stream(const T *__restrict__ mat,
                                                      const uint32_t *__restrict__ totals,
                                                      const double *__restrict__ rowH, const double *sl,
                                                      const float *slf, const PState &st, double he_base,
                                                      const PWin &win, uint64_t first,
                                                      uint64_t stride, uint64_t nrows, double *red,
                                                      uint32_t &nread, uint32_t &nprecise, uint32_t &nmid,
                                                      bool no_first_poll = true) {
    constexpr uint64_t B = 4096;
    constexpr int D = 4;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double dn = double(st.n), rn = 1.0 / dn;
    const double cband = coarse_band(B);
    const double thr_c_lo = st.thr - st.band - cband, thr_c_hi = st.thr + st.band + cband;
    constexpr bool W16 = sizeof(T) == 2;  // 16-bit rows: ONE 16-byte load per thread (bins 8 tid .. + 7)
    struct Row {
        Raw4<T> r0, r1;
        uint4 q;
        uint32_t tot;
        double hrow;
        unsigned long long ev;
    };
    // poll: also look at the event word (a device-scope round trip, longer than an L2 hit on the row).  The
    // window's first rows go without it -- the window has only just begun, and a row scored for nothing
    // changes no answer -- so the first score waits for its row alone.
    auto issue = [&](Row &w, uint64_t r, bool poll) {
        const uint64_t p = st.cursor + r;
        const T *rp = mat + p * B;
        if constexpr (W16) {
            w.q = *reinterpret_cast<const uint4 *>(rp + tid * 8);
        } else {
            w.r0.load(rp + tid * 4);
            w.r1.load(rp + 2048 + tid * 4);
        }
        w.tot = totals[p];
        if (wave == 0) {  // the row's entropy and the event word travel through LDS with the partial sums
            w.hrow = rowH[p];
            w.ev = poll ? p_hint_pos(win) : SEL_NONE;
        }
    };
    uint32_t par = 0;
    auto process = [&](Row &w, uint64_t r) -> bool {  // false: an earlier event exists, the workgroup is done
        const uint64_t p = st.cursor + r;
        const float rtn = w.tot ? float(rn / double(w.tot)) : 0.0f;
        const dvs_f2 r2 = {rtn, rtn};
        double c;
        if constexpr (W16) {
            asm volatile("" : "+v"(w.q.x), "+v"(w.q.y), "+v"(w.q.z), "+v"(w.q.w));
            double ca = 0.0, cb = 0.0;
            coarse8(w.q, slf + tid * 8, r2, ca, cb);
            c = ca + cb;
        } else {
            w.r0.pin();
            w.r1.pin();
            c = double(coarse4(w.r0.c, *reinterpret_cast<const float4 *>(slf + tid * 4), r2)) +
                double(coarse4(w.r1.c, *reinterpret_cast<const float4 *>(slf + 2048 + tid * 4), r2));
        }
        const double cs = dvs_wave_sum_dpp(c);
        double *slot = red + 48 + par * 16;
        par ^= 1;
        if (lane == 0) {
            slot[wave] = cs;
            if (wave == 0) {
                slot[8] = __longlong_as_double((long long)w.ev);
                slot[9] = w.hrow;
            }
        }
        __syncthreads();
        if ((unsigned long long)__double_as_longlong(slot[8]) < p) return false;
        if (w.tot == 0) return true;
        double hc = 0.0;
#pragma unroll
        for (int q = 0; q < P_THREADS / 64; q++) hc += slot[q];
        const double jf0 = -hc - (he_base + slot[9]) / dn;
        if (tid == 0) nread++;
        if (!(jf0 > thr_c_lo)) return true;  // (NaN: a negative bin, rejected as the reference does)
        if (jf0 > thr_c_hi) {
            if (tid < 8) p_post_event_wave(win, p, true, tid);  // (eight lanes, one instruction: every thread knows the score)
            return true;
        }
        if (tid == 0) {
            nmid++;
            nread--;  // counted again by the FAST pass
        }
        uint32_t nm = 0;
        p_scan_rows_wg<T, false>(mat, totals, rowH, sl, slf, B, st, he_base, win, r, nrows, nrows, red,
                                 nread, nprecise, nm, false);
        return true;
    };
    Row w[D];
#pragma unroll
    for (int d = 0; d < D; d++)
        if (first + uint64_t(d) * stride < nrows) issue(w[d], first + uint64_t(d) * stride, no_first_poll ? d >= 2 : true);
    for (uint64_t base = first; base < nrows; base += uint64_t(D) * stride) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            const uint64_t r = base + uint64_t(d) * stride;
            if (r >= nrows) return;
            if (!process(w[d], r)) return;
            if (r + uint64_t(D) * stride < nrows) issue(w[d], r + uint64_t(D) * stride, true);
        }
    }
}

}  // namespace
