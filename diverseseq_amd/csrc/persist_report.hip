// What DVS_PERSIST_DEBUG prints about the persistent engine's launches (persist.hip): phase times, a
// -DDVS_PERSIST_STAMPS build's window timelines, a -DDVS_PROBE build's interval, and why launches ended early.
#include "persist_dev.h"

#include <algorithm>
#include <cstddef>

#ifdef DVS_PERSIST_STAMPS
// four windows' timelines across the grid of `G` workgroups (PSync::trace of the launch's sync block `blk`)
static void persist_trace_report(const void *blk, uint32_t G) {
    std::vector<unsigned long long> tr(4 * 8 * 256);
    if (hipMemcpy(tr.data(), static_cast<const char *>(blk) + offsetof(PSync, trace), tr.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    for (int w_ = 0; w_ < 4; w_++) {
        const unsigned long long *t0 = &tr[(w_ * 8 + 0) * 256], *t1 = &tr[(w_ * 8 + 1) * 256], *t2 = &tr[(w_ * 8 + 2) * 256], *tg = &tr[(w_ * 8 + 3) * 256];
        const unsigned long long *t4 = &tr[(w_ * 8 + 4) * 256], *t5 = &tr[(w_ * 8 + 5) * 256], *t6 = &tr[(w_ * 8 + 6) * 256], *t7 = &tr[(w_ * 8 + 7) * 256];
        if (!tg[2] || G < 4) continue;
        std::vector<double> top, arr, seen, pub, tot, end_;
        unsigned long long first_top = ~0ull;
        for (uint32_t b = 0; b + 2 < G; b++) if (t0[b]) first_top = std::min(first_top, t0[b]);
        for (uint32_t b = 0; b + 2 < G; b++) {
            if (!t0[b] || !t1[b] || !t2[b]) continue;
            top.push_back((t0[b] - first_top) / 100.0);
            arr.push_back((t1[b] - first_top) / 100.0);
            seen.push_back((double(t2[b]) - double(tg[2])) / 100.0);
            if (t4[b] > tg[2] && t5[b] > tg[2] && t6[b] > tg[2]) {  // (the window ended in an accept)
                pub.push_back((double(t4[b]) - double(tg[2])) / 100.0);
                tot.push_back((double(t5[b]) - double(tg[2])) / 100.0);
                end_.push_back((double(t6[b]) - double(tg[2])) / 100.0);
            }
        }
        if (arr.empty()) continue;
        auto srt = [](std::vector<double> &v) { std::sort(v.begin(), v.end()); };
        srt(top); srt(arr); srt(seen);
        auto q_ = [](const std::vector<double> &v, double f) { return v[size_t(f * (v.size() - 1))]; };
        fprintf(stderr, "[dvs persist trace] window %d: tops 0 / %.2f / %.2f (min/median/max us), records stored %.2f / %.2f / %.2f / %.2f (min/median/90%%/max), "
                "gather begun %.2f, last record seen %.2f, release stored %.2f, release seen +%.2f / +%.2f / +%.2f (min/median/max after it was stored)\n",
                w_ * 12 + 12, q_(top, 0.5), top.back(), arr.front(), q_(arr, 0.5), q_(arr, 0.9), arr.back(),
                (double(tg[0]) - double(first_top)) / 100.0, (double(tg[1]) - double(first_top)) / 100.0, (double(tg[2]) - double(first_top)) / 100.0,
                seen.front(), q_(seen, 0.5), seen.back());
        if (pub.empty()) continue;
        {   // the five workgroups that published last: when each arrived, saw the release, published
            std::vector<std::pair<double, uint32_t>> late;
            for (uint32_t b = 0; b + 2 < G; b++)
                if (t4[b] > tg[2]) late.emplace_back((double(t4[b]) - double(tg[2])) / 100.0, b);
            std::sort(late.rbegin(), late.rend());
            for (size_t i = 0; i < late.size() && i < 5; i++) {
                const uint32_t b = late[i].second;
                fprintf(stderr, "[dvs persist trace] window %d: workgroup %u arrived %.2f before the release was stored, saw it +%.2f, handed its speculative job over +%.2f, was through the job loop +%.2f\n",
                        w_ * 12 + 12, b, (double(tg[2]) - double(t1[b])) / 100.0, (double(t2[b]) - double(tg[2])) / 100.0,
                        (double(t7[b]) - double(tg[2])) / 100.0, late[i].first);
            }
        }
        {   // when the speculative jobs were handed over (mailboxes: stored), relative to the release
            std::vector<double> sp;
            for (uint32_t b = 0; b + 2 < G; b++)
                if (t7[b] && t4[b] > tg[2]) sp.push_back((double(t7[b]) - double(tg[2])) / 100.0);
            if (!sp.empty()) {
                srt(sp);
                fprintf(stderr, "[dvs persist trace] window %d: speculative jobs handed over %.2f / %.2f / %.2f / %.2f us after the release was stored "
                        "(min/median/90%%/max over %zu workgroups; negative: before)\n", w_ * 12 + 12, sp.front(), q_(sp, 0.5), q_(sp, 0.9), sp.back(), sp.size());
            }
        }
        srt(pub); srt(tot); srt(end_);
        fprintf(stderr, "[dvs persist trace] window %d, its accept (us after the release was stored; min/median/max): job published %.2f / %.2f / %.2f, "
                "totals read %.2f / %.2f / %.2f, rebuild done %.2f / %.2f / %.2f\n", w_ * 12 + 12, pub.front(), q_(pub, 0.5), pub.back(),
                tot.front(), q_(tot, 0.5), tot.back(), end_.front(), q_(end_, 0.5), end_.back());
    }
}
#endif

// DVS_PERSIST_DEBUG, at every poll of a selection on the persistent engine: what its launches left in their sync blocks
// (the head phase's launch first, then the full grid's) on stderr -- scripts/stamps_to_json.py parses these lines
void dvs_persist_debug_report(dvs_ctx *ctx, const dvs_select *s) {
    for (int which = 0; which < 2 && s->persist.on; which++) {
        unsigned long long dbg[32];  // dbg2[16] then dbg[16]
        const void *blk = which ? s->persist.sync : s->persist.sync_head;
        if (!blk || hipMemcpy(dbg, static_cast<const char *>(blk) + offsetof(PSync, dbg2), sizeof dbg, hipMemcpyDeviceToHost) != hipSuccess)
            continue;
        fprintf(stderr, "[dvs persist] %s launch\n", which ? "full-grid" : "head-phase");
#if defined(DVS_PERSIST_STAMPS) && defined(DVS_PROBE)
        if (DVS_PROBE) {  // (a one-interval build: [0] ticks, [1] passes; block 0 then the last scanning block)
            fprintf(stderr, "[dvs persist probe %d] block 0 (owns a job): %.3f us x %llu; the last scanning block (no job): %.3f us x %llu\n",
                    int(DVS_PROBE), dbg[1] ? dbg[0] / 100.0 / double(dbg[1]) : 0.0, dbg[1],
                    dbg[17] ? dbg[16] / 100.0 / double(dbg[17]) : 0.0, dbg[17]);
            continue;
        }
#endif
        for (int w = 0; w < 2; w++)
            fprintf(stderr, "[dvs persist %s] us: scan %.1f bar1 %.1f resolve %.1f loo %.1f bar2 %.1f | partials %.1f combine %.1f lowest-row fetch %.1f rebuild %.1f\n",
                    w ? "mirror block" : "block 0", dbg[0 + 16 * w] / 100.0, dbg[1 + 16 * w] / 100.0,
                    dbg[2 + 16 * w] / 100.0, dbg[3 + 16 * w] / 100.0, dbg[4 + 16 * w] / 100.0,
                    dbg[6 + 16 * w] / 100.0, dbg[7 + 16 * w] / 100.0, dbg[8 + 16 * w] / 100.0,
                    dbg[5 + 16 * w] / 100.0);
#ifdef DVS_PERSIST_STAMPS
        persist_trace_report(blk, which ? s->persist.grid : uint32_t(ctx->head_cus));
#endif
        if (dbg[15] + dbg[14])
            fprintf(stderr, "[dvs persist block 0] accepts for which its leave-one-out job was ready when the release came: %llu (the candidate's frequencies: %llu)\n", dbg[15], dbg[14]);
        if (dbg[9] + dbg[10] + dbg[11] + dbg[12])
            fprintf(stderr, "[dvs persist block 0] us inside the phases: window top %.1f own rows scanned %.1f hint look + record %.1f (then: scan = the rest) | behind the rebuild %.1f\n",
                    dbg[9] / 100.0, dbg[10] / 100.0, dbg[11] / 100.0, dbg[12] / 100.0);
        if (dbg[16 + 10] + dbg[16 + 12])
            fprintf(stderr, "[dvs persist] scan + rendezvous: row-per-workgroup windows %llu (%.1f us, %llu rows), "
                    "row-per-wave windows %llu (%.1f us, %llu rows)\n", dbg[16 + 10], dbg[16 + 9] / 100.0,
                    dbg[16 + 13], dbg[16 + 12], dbg[16 + 11] / 100.0, dbg[16 + 14]);
    }
}

// DVS_PERSIST_DEBUG, when a selection is done: why its persistent launches ended early (SelCtl::why)
void dvs_persist_debug_done(const SelCtl &c) {
    fprintf(stderr, "[dvs persist] launches ended early: replica full %u, sum check %u, push argmin %u, stat comparison %u, "
            "candidate in band %u, replace argmin %u, state not taken %u / %u\n", c.why[0], c.why[1], c.why[2], c.why[3],
            c.why[4], c.why[5], c.why[6], c.why[7]);
}
