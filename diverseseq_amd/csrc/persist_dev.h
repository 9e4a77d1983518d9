// What the persistent engine's workgroups share (persist.hip; the host reports of persist_report.hip read the sync
// block): the words that cross workgroups, the sync block, the counter barrier, the window's rendezvous, the window
// policy, the members' argmin, and the LDS budget of a launch.
//
// Inter-workgroup protocol (MI355X: 8 XCDs, private L2s; written down in DESIGN.md 4.3c).  Nothing a
// workgroup stores with plain stores is read by another workgroup during the launch: the matrix, totals
// and row entropies are read-only (a member's frequency row is re-derived from its matrix row, whose
// position every workgroup keeps in LDS) and the set state is replicated.  What crosses workgroups are
// single 64-bit words, read and written with relaxed agent-scope atomics, and every one of them carries
// in itself what a reader needs to know that it is the word it is waiting for -- no word's meaning depends
// on the order in which stores to two different addresses become visible:
//   * WINDOW words carry the window's number in their top bits (p_word).  A workgroup that has scanned its
//     share stores ONE arrival record (its first event, how many near-threshold candidates it listed); the
//     mirror block, which scans nothing, polls the records, and when all carry the window's number stores
//     the release word (the window's first event) to eight copies that the others poll.  Events found
//     early also go, by atomicMin, to a hint word beside the release word so that waves can stop scanning
//     rows behind them; a newer window's tag is SMALLER, so a straggler of an older window never wins, and
//     nothing is ever cleared.  The outcome never depends on a hint: a wave only skips rows behind a hint
//     of the current window, and whoever posted that hint has the same event in its record.
//   * LEAVE-ONE-OUT sums are added to monotonic accumulators (fixed point + a contribution count in the low
//     bits, p_acc_word) that are never cleared: every workgroup remembers the totals it read at the previous
//     use (LDS) and takes the difference; the count's difference says when the K contributions are in.
// The counter barrier below (grid_barrier) is a pure rendezvous for the few places that still want one (the
// seeded start, `max` batches): two-level monotonic arrival counters (per group of blockIdx % 8, then one
// top counter) and a generation word per group, all on their own cache lines, zeroed by the host before
// every launch; every spin is bounded (a grid that is not fully resident ends with SEL_ERROR instead of
// hanging).
#pragma once

#include "select_dev.h"

namespace {

constexpr int P_THREADS = 512;
constexpr int P_J = 8;                      // bins per thread kept in registers (B <= 4096)
constexpr int P_CH = 16;                    // row chunks requested per burst (4096 bins)
constexpr uint32_t P_MAXN = 512;            // members the LDS replica holds when 4^k <= 4096 ...
constexpr uint32_t P_MAXN_BIG = 256;        // ... and beyond (k = 7: 128 KB of LDS go to the set state)
constexpr uint32_t P_MAXN_MAX = 896;        // ... `max` with 4^k <= 4096 (sets grow; what 160 KB of LDS hold beside S, sl and the batches)
constexpr uint32_t p_maxn(bool cached, bool maxm = false) { return cached ? (maxm ? P_MAXN_MAX : P_MAXN) : P_MAXN_BIG; }
// SMALL sets (nmost over 16-bit count rows of 4096 bins): the members' count rows live in every
// workgroup's LDS (see the kernel)
constexpr uint32_t P_SMALLN = 16;      // members the replica arrays of a SMALL launch hold ...
constexpr uint32_t P_SMALL_ROWS = 13;  // ... and rows (8 KB each) that fit beside the state in 160 KB of LDS
// leave-one-out jobs per event: (n + 1) * K <= max(G - 1, n + 1) <= maxn + 1 (G <= maxn + 2 is checked)
constexpr uint32_t p_maxjobs(bool cached, bool maxm = false) { return p_maxn(cached, maxm) + 1; }
// leave-one-out accumulators: 8 group replicas x (maxn + 1) members x 2 words, zeroed by the host before the
// launch and never cleared again.  A word = (2^-50 fixed-point sum << 6) + number of contributions, added to
// by every job of every use; a reader keeps the totals it read at the previous use (LDS, p_prev) and works
// with the DIFFERENCE: its low six bits are the contributions of this use -- complete at K -- and the rest
// is their sum (two's complement: wrap-around cancels in the difference; |sum| < 64 per use and K <= 32
// keep one use inside the word).  Integer addition is associative, so the totals do not depend on the order
// the jobs arrive in; nothing is ever reset, so there is no clear that a late add could race with, and an
// add can never be mistaken for one of an earlier use: the earlier use was complete, in every replica,
// when it was read (each job adds the same word to all eight replicas).
constexpr size_t p_acc_bytes(uint32_t maxn) { return size_t(8) * (maxn + 1) * 2 * sizeof(unsigned long long); }
__device__ __forceinline__ unsigned long long p_acc_word(double v) {
    return ((unsigned long long)__double2ll_rn(v * 0x1p50) << 6) + 1ull;
}
__device__ __forceinline__ double p_acc_value(unsigned long long w) { return double((long long)w >> 6) * 0x1p-50; }
// A job's two words added to an accumulator pair (non-returning adds: the readers wait for the counts)
__device__ __forceinline__ void p_acc_add(unsigned long long *dst, double th, double ts) {
    atomicAdd(dst, p_acc_word(th));
    atomicAdd(dst + 1, p_acc_word(ts));
}
__device__ __forceinline__ uint32_t p_acc_count(unsigned long long w) { return uint32_t(w & 63ull); }
// this use's share of an accumulator word once all K contributions are in: (total now) - (total at the previous
// use, *prev, which is brought up to date).  Bounded spin: ok = false on a time-out (an error and the
// multi-launch kernels, never a wrong total).
__device__ __forceinline__ unsigned long long p_acc_complete(const unsigned long long *w, unsigned long long *prev,
                                                             uint32_t K, bool &ok) {
    const unsigned long long before = *prev;
    unsigned long long v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t spins = 0;
    while (uint32_t((v - before) & 63ull) != K) {
        if (++spins > (1u << 20)) {
            ok = false;
            break;
        }
        __builtin_amdgcn_s_sleep(1);
        v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    *prev = v;
    return v - before;
}
constexpr uint32_t P_SPIN_LIMIT = 1u << 22;  // ~0.5 s of polling
constexpr uint32_t P_MAXG = 256;             // workgroups a launch may have (one arrival record each)
constexpr uint32_t P_FLAT_GRID = 64;         // counter barrier: grids of up to this many workgroups use one counter
constexpr uint32_t P_WINWORDS = 64;          // LDS words of a window's bookkeeping (s_win)
constexpr uint32_t P_LIST = 2;               // near-threshold candidates a workgroup lists per window (more become plain events)
// MODE_MAX, growth phase: consecutive rows evaluated against the same set in one go (see the kernel)
constexpr uint32_t P_BATCH = 32;             // rows per batch at most
constexpr uint32_t P_BATCH_MEMBERS = 256;    // set size + 2 up to which batches are formed (4 members per lane)
constexpr size_t p_batch_bytes() { return size_t(P_BATCH) * (P_BATCH_MEMBERS + 2) * 4 * sizeof(double); }
constexpr size_t p_batch_lds() { return size_t(P_BATCH) * (2 + 12 + 24) * sizeof(double); }

// The dynamic LDS of a launch, in the order persist_nmost_kernel (persist.hip) carves it up by pointer arithmetic --
// that arithmetic and this function change together:
//   [sl: B f64, B rounded up to 2][slf: B f32, B rounded up to 4 -- COARSE: count rows, state in the register cache]
//   [Sl: as sl -- MAXM][scratch: 128 f64]
//   [s_mH, s_tot, s_rt, s_dl, s_ds: maxn f64 each][s_pos: maxn u64][s_slot: maxn u32 (maxn is a multiple of 4)]
//   [s_win: P_WINWORDS u64][flags: 16 bytes][s_ltab: 128 double2][s_prev: (maxn + 1) x 2 u64]
//   [s_tail -- MAXM: a batch's block (p_batch_lds) | SMALL: small_rows count rows of B u16 |
//              OWN: s_inv maxn u32, s_own P_J * P_THREADS counts | else nothing]
//   ... [the last 128 bytes: the ticks of a -DDVS_PERSIST_STAMPS build]
// kind: the matrix's (0: 32-bit counts, 1: f64 rows, 2: 16-bit counts).  small_rows != 0: the SMALL instantiation with that
// many member rows; 0: OWN wherever the kernel has it (nmost over count rows in the register cache).
// The byte count is the key of the context's occupancy answers, what the kernel's LDS limit is raised to and what decides
// whether a selection falls to the multi-launch engine: it asks for a little more than the carve-up uses, and keeps doing so.
constexpr size_t P_LDS_SLACK = 56;        // bytes asked for beyond the carve-up ...
constexpr size_t P_LDS_SLACK_SMALL = 16;  // ... and by a SMALL launch on top of them
constexpr size_t p_lds_bytes(uint64_t B, int kind, bool cached, bool maxm, uint32_t small_rows) {
    const bool coarse = cached && kind != 1, own = coarse && !maxm && !small_rows;
    const size_t maxn = small_rows ? P_SMALLN : p_maxn(cached, maxm);
    const size_t sl = ((B + 1) & ~1ull) * sizeof(double);
    const size_t slf = coarse ? ((B + 3) & ~3ull) * sizeof(float) : 0;
    const size_t Sl = maxm ? sl : 0;
    const size_t scratch = 128 * sizeof(double);
    const size_t members = maxn * (5 * sizeof(double) + sizeof(uint64_t) + sizeof(uint32_t));
    const size_t s_win = P_WINWORDS * sizeof(unsigned long long), flags = 16, s_ltab = 128 * sizeof(double2);
    const size_t s_prev = (maxn + 1) * 2 * sizeof(unsigned long long);
    const size_t tail = maxm         ? p_batch_lds()
                        : small_rows ? small_rows * B * sizeof(uint16_t) + P_LDS_SLACK_SMALL
                        : own        ? maxn * sizeof(uint32_t) + size_t(P_J) * P_THREADS * (kind == 2 ? sizeof(uint16_t) : sizeof(uint32_t))
                                     : 0;
    const size_t stamps = 128;
    return sl + slf + Sl + scratch + members + s_win + flags + s_ltab + s_prev + tail + stamps + P_LDS_SLACK;
}
// (the values of the formula this function replaced, worked out from that formula)
static_assert(p_lds_bytes(4096, 2, true, false, 2) == 70440 && p_lds_bytes(4096, 2, true, false, 13) == 160552, "nmost, 4096 bins, 16-bit, SMALL");
static_assert(p_lds_bytes(4096, 2, true, false, 0) == 98008, "nmost, 4096 bins, 16-bit, OWN");
static_assert(p_lds_bytes(4096, 0, true, false, 0) == 106200 && p_lds_bytes(4096, 1, true, false, 0) == 71384, "nmost, 4096 bins, 32-bit and f64");
static_assert(p_lds_bytes(16384, 2, false, false, 0) == 152280 && p_lds_bytes(16384, 0, false, false, 0) == 152280, "nmost, 16384 bins");
static_assert(p_lds_bytes(4096, 2, true, true, 0) == 156376 && p_lds_bytes(256, 2, true, true, 0) == 79576, "max, 16-bit");
static_assert(p_lds_bytes(125, 0, true, false, 0) == 58568, "nmost, 125 bins, 32-bit");

struct PLine {  // a polled word on a cache line of its own (256 B apart)
    uint32_t v;
    uint32_t pad[63];
};
struct PRel {  // what a waiting workgroup polls with ONE 16-byte load, on a cache line of its own
    unsigned long long rel;   // the release word of the current window: its first event (window word, below)
    unsigned long long hint;  // events posted so far (atomicMin of window words; starts as all ones)
    unsigned long long pad[30];
};

struct PSync {
    uint32_t count;  // counter barrier: top-level arrivals (one per group and barrier), monotonic over the launch
    uint32_t pad0[63];
    PLine gcount[8];  // ... arrivals of group g = blockIdx % 8 (workgroups are dealt round-robin to the 8 XCDs)
    PLine ggen[8];    // ... completed barriers, one copy per group so 32 pollers share a line, not 256
    uint32_t timeout;
    uint32_t wg_thresh;  // windows of up to wg_thresh rows per workgroup are scanned a row per WORKGROUP (0: never)
    float wg_scale;      // ... and are cursor * wg_scale / size rows long (rounded up to whole rounds)
    uint32_t no_coarse;  // measurement aid: skip the COARSE tier
    uint32_t stop_at;    // head phase: leave at this stream position with status RUN (0: walk the whole stream)
    uint32_t seeded;     // the set is still only its seed positions: the launch works the initial state out itself
    const unsigned long long *seed_list;  // ... those positions (ctl->size of them)
    uint32_t small_rows;  // SMALL instantiation: member rows the LDS replica has room for
    uint32_t lds_bytes;   // the launch's dynamic LDS (a -DDVS_PERSIST_STAMPS build keeps its ticks in the last 128 bytes)
    uint32_t wmax;        // longest window of this engine (the control block's cap is the multi-launch scan's)
    uint32_t pad2[53];
    PRel rel[8];                            // one copy per group g = blockIdx % 8
    // Two sets of arrival records and listed candidates, taking turns by the window's parity: a workgroup that is
    // still walking window e's listed candidates reads the others' records and entries of window e, while a quick
    // one may already have scanned window e + 1 and stored its record for it.  Window e + 2's words (the same set as
    // e's) cannot be written before every workgroup has stored its record for e + 1, i.e. has left window e.
    unsigned long long wrec[2][P_MAXG];          // arrival record of every workgroup (a window word)
    unsigned long long soft[2][P_MAXG][P_LIST];  // the candidates a workgroup listed in the window (window words)
#ifdef DVS_PERSIST_STAMPS
    // four traced windows (epochs 12, 24, 36, 48): 100 MHz ticks per workgroup at the window's top, at its arrival record,
    // when it saw the release; [3] = the gathering block's own: gather begun, last record seen, release stored
    // [4..6]: the accept behind the window: this workgroup's job published (or nothing to publish), its totals read, its
    // rebuild of sl done
    unsigned long long trace[4][8][P_MAXG];  // ([7]: the speculative job's sums handed to the accumulators, or that point passed)
#endif
    unsigned long long dbg2[16];   // block 0 (owns a job): phase ticks
    unsigned long long dbg[16];    // mirror block: 100 MHz ticks per phase (scan, bar1, resolve, loo, bar2, finalize)
};

struct PState {  // replicated scalars (identical in every workgroup)
    uint64_t cursor, npos;
    uint32_t window, wmin, wmax;
    uint32_t n, li;
    double sumH, total_jsd, thr, band, wscale;
    uint32_t n_windows, n_events, n_accepts;
    // MODE_MAX: the set grows while it is below max_size (tentative pushes, records.rs:427-451)
    uint32_t max_size, stat;
    double mean_d, std_d, cov_d;  // statistics of the current set's delta_jsd
};

#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ---- window words.  [63:40] tag = P_TAG0 - window number (a NEWER window has the SMALLER tag: an atomicMin
// prefers it and a straggler of an older window can never replace it; all ones -- the hint words' initial
// value -- and zero -- everything else's -- are no window's tag), [39:3] stream position (all ones: none),
// [2:1] candidates listed (arrival record: how many this workgroup listed; release word: non-zero if anybody
// did), [0] set when the event is not a sure one (its exact score decides).
constexpr uint32_t P_TAG0 = 0xFFFFFEu;
constexpr uint32_t P_EPOCH_MAX = 0xFFFFF0u;  // windows a launch may walk (it leaves with status RUN there)
constexpr unsigned long long P_POS_NONE = (1ull << 37) - 1;
__device__ __forceinline__ unsigned long long p_word(uint32_t epoch, uint64_t pos, bool sure) {
    return ((unsigned long long)(P_TAG0 - epoch) << 40) | ((pos == SEL_NONE ? P_POS_NONE : pos) << 3) | (sure ? 0ull : 1ull);
}
__device__ __forceinline__ bool p_word_is(unsigned long long w, uint32_t epoch) { return uint32_t(w >> 40) == P_TAG0 - epoch; }
// the position a word of window `epoch` names (SEL_NONE: none, or a word of another window)
__device__ __forceinline__ uint64_t p_word_pos(unsigned long long w, uint32_t epoch) {
    const unsigned long long pos = (w >> 3) & P_POS_NONE;
    return (!p_word_is(w, epoch) || pos == P_POS_NONE) ? SEL_NONE : uint64_t(pos);
}
__device__ __forceinline__ bool p_word_sure(unsigned long long w) { return (w & 1ull) == 0; }
__device__ __forceinline__ uint32_t p_word_listed(unsigned long long w) { return uint32_t(w >> 1) & 3u; }

// returns false on timeout (every thread of the block gets the same answer).
// Two levels: a workgroup arrives on its group's counter, the last of a group arrives on the top
// counter, the last group publishes the generation to all eight group words.  Measured on MI355X
// (scripts/micro/barrier_bench.hip, 256 workgroups): 1.9 us against 3.7 us for one counter + one
// word -- the 256 same-address atomics serialise at ~11 ns each.
// The barrier is a pure rendezvous: no fences.  What is handed across it are atomic words whose readers
// can tell that they are complete (the accumulators' contribution counts) or whose writer consumed the
// result of the exchange that put them there (the `max` batches' results); the matrix is read-only for the
// whole launch, and what the mirror block stores to global memory is read by nobody before the kernel
// ends.  (An agent-scope release + acquire pair around the barrier -- L2 write-back and invalidate on
// every XCD -- cost another 4 us per barrier.)
__device__ bool grid_barrier(PSync *sync, uint32_t G, uint32_t &gen, int *s_ok) {
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t target = gen + 1;
        const uint32_t x = blockIdx.x & 7u, ng = G < 8u ? G : 8u;
        const uint32_t gsz = (G - x + 7u) >> 3;  // workgroups with blockIdx % 8 == x
        int ok = 1;
        bool released = false;
        const bool last = G <= P_FLAT_GRID
                              ? __hip_atomic_fetch_add(&sync->count, 1u, RLX_AGENT) == G * target - 1
                              : (__hip_atomic_fetch_add(&sync->gcount[x].v, 1u, RLX_AGENT) == gsz * target - 1 &&
                                 __hip_atomic_fetch_add(&sync->count, 1u, RLX_AGENT) == ng * target - 1);
        if (last) {
            for (uint32_t g = 0; g < ng; g++) __hip_atomic_store(&sync->ggen[g].v, target, RLX_AGENT);
            released = true;
        }
        if (!released) {
            uint32_t spins = 0;
            while (__hip_atomic_load(&sync->ggen[x].v, RLX_AGENT) < target) {
                if ((++spins & 255u) == 0 &&
                    (spins > P_SPIN_LIMIT || __hip_atomic_load(&sync->timeout, RLX_AGENT))) {
                    __hip_atomic_store(&sync->timeout, 1u, RLX_AGENT);
                    ok = 0;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        *s_ok = ok;
    }
    __syncthreads();
    gen++;
    return *s_ok != 0;
}

// 16 bytes in one agent-scope load (one request for a PRel's two words; each word validates itself)
__device__ __forceinline__ uint4 p_load16_agent(const void *ptr) {
    uint4 v;
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(ptr) : "memory");
    return v;
}

// What a scanning wave needs of the window it is in (uniform values).
struct PWin {
    uint32_t epoch;               // the window's number
    const unsigned long long *hintp;  // this group's hint word
    PRel *rel;                    // the eight group copies (hints are posted to all of them)
    unsigned long long *wgev;     // LDS: this workgroup's first event so far (becomes its arrival record)
    uint32_t *nlist;              // LDS: candidates this workgroup has listed in this window
    unsigned long long *mysoft;   // this workgroup's list entries (sync->soft[epoch & 1][blockIdx.x])
};
// the first event posted so far in this window, as far as this group's hint word knows
__device__ __forceinline__ uint64_t p_hint_pos(const PWin &w) {
    return p_word_pos(__hip_atomic_load(w.hintp, RLX_AGENT), w.epoch);
}
// An event found by a wave (called by its lanes 0..7 at least): into the workgroup's record (LDS) and, as a
// hint for the waves still scanning, into every group's hint word -- fire and forget, nothing waits for it.
__device__ __forceinline__ void p_post_event_wave(const PWin &w, uint64_t p, bool sure, uint32_t lane) {
    const unsigned long long word = p_word(w.epoch, p, sure);
    if (lane == 0) atomicMin(w.wgev, word);
    if (lane < 8) atomicMin(&w.rel[lane].hint, word);
}
__device__ __forceinline__ void p_post_event_thread(const PWin &w, uint64_t p, bool sure) {
    const unsigned long long word = p_word(w.epoch, p, sure);
    atomicMin(w.wgev, word);
    for (uint32_t g = 0; g < 8; g++) atomicMin(&w.rel[g].hint, word);
}
// A candidate whose fast score is within FAST_BAND of the threshold: listed, not an event -- the scan goes on
// and the workgroups settle it in f64 after the rendezvous.  A workgroup's list holds P_LIST entries per
// window (window words: a reader knows which window an entry belongs to); the count travels in its arrival
// record.  A full list makes the candidate a plain (unsure) event.  One thread.
__device__ __forceinline__ void p_list_candidate(const PWin &w, uint64_t p) {
    const uint32_t idx = atomicAdd(w.nlist, 1u);
    if (idx < P_LIST) __hip_atomic_store(w.mysoft + idx, p_word(w.epoch, p, false), RLX_AGENT);
    else p_post_event_thread(w, p, false);
}
// wave-wide minimum of 64-bit words by DPP (register cross-lane moves, as dvs_wave_sum_dpp): every lane gets it
template <int CTRL>
__device__ __forceinline__ unsigned long long p_dpp_mov_u64(unsigned long long v) {
    int lo = int(uint32_t(v)), hi = int(uint32_t(v >> 32));
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    return ((unsigned long long)uint32_t(hi) << 32) | uint32_t(lo);
}
__device__ __forceinline__ unsigned long long p_wave_min_u64(unsigned long long v) {
    auto mn = [](unsigned long long a, unsigned long long b) { return b < a ? b : a; };
    v = mn(v, p_dpp_mov_u64<0xB1>(v));   // quad_perm [1,0,3,2]
    v = mn(v, p_dpp_mov_u64<0x4E>(v));   // quad_perm [2,3,0,1]
    v = mn(v, p_dpp_mov_u64<0x141>(v));  // row_half_mirror
    v = mn(v, p_dpp_mov_u64<0x140>(v));  // row_mirror: every lane holds the minimum of its row of 16
    const int lo = int(uint32_t(v)), hi = int(uint32_t(v >> 32));
    auto row = [&](int l) {
        return ((unsigned long long)uint32_t(__builtin_amdgcn_readlane(hi, l)) << 32) | uint32_t(__builtin_amdgcn_readlane(lo, l));
    };
    return mn(mn(row(0), row(16)), mn(row(32), row(48)));
}

// The gathering block's part of a window's rendezvous, by ONE wave: lane l waits for the arrival records of
// workgroups l, l + 64, l + 128, l + 192 (four loads in flight per look; records of other windows are not looked
// at twice), the minimum is taken by DPP, lanes 0..7 store the release word -- no LDS, no barrier between the last
// record's arrival and the release.  `own`: the gathering block's own record.  Returns the release word; ok = false
// on a time-out (the launch is then given up: sync->timeout).  seen_all / stored: 100 MHz ticks (stamps builds).
__device__ __forceinline__ unsigned long long p_gather(PSync *sync, uint32_t G, uint32_t epoch, unsigned long long own,
                                                       uint32_t lane, bool &ok, unsigned long long *seen_all = nullptr,
                                                       unsigned long long *stored = nullptr) {
    constexpr uint32_t Q = P_MAXG / 64;
    unsigned long long w[Q];
    bool have[Q];
#pragma unroll
    for (uint32_t q = 0; q < Q; q++) {
        w[q] = ~0ull;
        have[q] = lane + 64 * q >= G - 1;  // (this workgroup's own record is `own`)
    }
    uint32_t spins = 0;
    ok = true;
    for (;;) {
        unsigned long long got[Q];
#pragma unroll
        for (uint32_t q = 0; q < Q; q++)
            got[q] = have[q] ? 0ull : __hip_atomic_load(&sync->wrec[epoch & 1u][lane + 64 * q], RLX_AGENT);
        bool all = true;
#pragma unroll
        for (uint32_t q = 0; q < Q; q++) {
            if (!have[q] && p_word_is(got[q], epoch)) {
                w[q] = got[q];
                have[q] = true;
            }
            all = all && have[q];
        }
        if (__ballot(!all) == 0ull) break;
        if ((++spins & 255u) == 0 && (spins > P_SPIN_LIMIT || __hip_atomic_load(&sync->timeout, RLX_AGENT))) {
            ok = false;
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    if (seen_all) *seen_all = __builtin_amdgcn_s_memrealtime();
    unsigned long long m = own & ~6ull, fl = own & 6ull;
#pragma unroll
    for (uint32_t q = 0; q < Q; q++)
        if (lane + 64 * q < G - 1 && have[q]) {
            m = (w[q] & ~6ull) < m ? (w[q] & ~6ull) : m;
            fl |= w[q] & 6ull;
        }
    m = p_wave_min_u64(m);
    const bool anyl = __ballot(fl != 0ull) != 0ull;
    const unsigned long long relw = m | (anyl ? 2ull : 0ull);
    if (ok && lane < 8) __hip_atomic_store(&sync->rel[lane].rel, relw, RLX_AGENT);
    if (!ok && lane == 0) __hip_atomic_store(&sync->timeout, 1u, RLX_AGENT);
    if (stored) *stored = __builtin_amdgcn_s_memrealtime();
    return relw;
}

// Window policy of the persistent engine.  Short windows run a row per workgroup (p_scan_rows_wg) and
// are whole rounds of the scanning workgroups long; the scale aims at ~3 in 4 windows ending in an
// accept (the accept probability at stream position i is ~ size / i).
__device__ __forceinline__ uint32_t p_next_window(const PState &st, uint32_t nwg, uint32_t wg_thresh,
                                                  double wg_scale, bool &wgmode) {
    if (wg_thresh) {
        uint64_t w = uint64_t(double(st.cursor) * wg_scale / double(st.n ? st.n : 1u));
        w = (w + nwg - 1) / nwg * nwg;
        if (w < nwg) w = nwg;
        if (w <= uint64_t(wg_thresh) * nwg) {
            wgmode = true;
            return uint32_t(w);
        }
    }
    wgmode = false;
    return sel_next_window(st.cursor, st.n, st.wmin, st.wmax, st.wscale);
}

// argmin (strict '<' from 1e6, first index), runner-up, mean and standard deviation of the
// members' delta_jsd by ONE wave: lane l owns members l, l + 64, ... (Q per lane; re-read from LDS
// in every pass when Q > 1 -- registers are the scan loop's).
// scratch[100..105] = min, index, second, mean, sd, any-risky.
template <uint32_t Q>
__device__ __forceinline__ void p_argmin(const double *s_dl, const double *s_ds, uint32_t n, uint64_t B,
                                         uint32_t lane, double *scratch) {
    const double v0 = lane < n ? s_dl[lane] : 1e6;
    auto val = [&](uint32_t q) { return (Q == 1 || q == 0) ? v0 : s_dl[lane + 64 * q]; };
    double best = 1e6, acc = 0.0;
    bool rk = false;
#pragma unroll
    for (uint32_t q = 0; q < Q; q++) {
        const uint32_t r = lane + 64 * q;
        if (r < n) {
            const double v = val(q);
            rk |= sum_risky(s_ds[r], B);
            acc += v;
            if (v < best) best = v;
        }
    }
    const double dn = double(n);
    const double mnv = dvs_wave_min(best);
    double fi = 4294967295.0;
#pragma unroll
    for (uint32_t q = 0; q < Q; q++)
        if (mnv < 1e6 && lane + 64 * q < n && val(q) == mnv) fi = fmin(fi, double(lane + 64 * q));
    const double first = dvs_wave_min(fi);
    const uint32_t lw = (first < 4294967295.0) ? uint32_t(first) : 0u;
    const double mu = dvs_wave_sum(acc) / dn;
    double sec = 1e6, tv = 0.0;
#pragma unroll
    for (uint32_t q = 0; q < Q; q++) {
        const uint32_t r = lane + 64 * q;
        if (r < n) {
            const double v = val(q);
            if (r != lw && v < sec) sec = v;
            const double t = v - mu;
            tv += t * t;
        }
    }
    sec = dvs_wave_min(sec);
    const double var = dvs_wave_sum(tv);
    const unsigned long long anyr = __ballot(rk);
    if (lane == 0) {
        scratch[100] = mnv;
        scratch[101] = double(lw);
        scratch[102] = sec;
        scratch[103] = mu;
        scratch[104] = sqrt(var / (dn - 1.0));
        scratch[105] = anyr ? 1.0 : 0.0;
    }
}

}  // namespace
