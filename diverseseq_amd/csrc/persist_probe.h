// Diagnostic builds of the persistent engine (persist.hip): the stamp, trace, probe and chaos macros.  They expand
// inside persist_nmost_kernel, which declares what they name (s_dbg, t_prev; lead, tid, epoch, n_work).
#pragma once

#ifdef DVS_PERSIST_STAMPS
#ifdef DVS_PROBE
// ONE interval per build (-DDVS_PERSIST_STAMPS -DDVS_PROBE=k, scripts/probe.sh): thread 0 of block 0 (it owns a leave-one-out
// job) and of the last scanning block (it owns none) take two clock reads per pass -- everything else is switched off, so
// what is measured is not the stamps.  [0] the ticks, [1] the passes.
#define P_PROBE_BEGIN(id)                                                                          \
    do {                                                                                           \
        if ((id) == DVS_PROBE && (blockIdx.x == 0 || blockIdx.x == n_work - 1) && tid == 0)        \
            t_prev = __builtin_amdgcn_s_memrealtime();                                             \
    } while (0)
#define P_PROBE_END(id)                                                                            \
    do {                                                                                           \
        if ((id) == DVS_PROBE && (blockIdx.x == 0 || blockIdx.x == n_work - 1) && tid == 0) {      \
            s_dbg[0] += __builtin_amdgcn_s_memrealtime() - t_prev;                                 \
            s_dbg[1] += 1;                                                                         \
        }                                                                                          \
    } while (0)
#define P_STAMP(k) do { } while (0)
#define P_STAMP_B0(k) do { } while (0)
#define P_TRACE(which) do { } while (0)
#define P_TRACE_G(slot) do { } while (0)
#else
#define P_PROBE_BEGIN(id) do { } while (0)
#define P_PROBE_END(id) do { } while (0)
#define P_STAMP(k)                                                         \
    do {                                                                   \
        if ((lead || blockIdx.x == 0) && tid == 0) {                       \
            const unsigned long long t_now = __builtin_amdgcn_s_memrealtime(); \
            s_dbg[k] += t_now - t_prev;                                    \
            t_prev = t_now;                                                \
        }                                                                  \
    } while (0)
// (block 0 only: finer stamps inside a phase -- slots 9..14 are the mirror block's window statistics)
#define P_STAMP_B0(k)                                                      \
    do {                                                                   \
        if (blockIdx.x == 0 && !lead && tid == 0) {                        \
            const unsigned long long t_now = __builtin_amdgcn_s_memrealtime(); \
            s_dbg[k] += t_now - t_prev;                                    \
            t_prev = t_now;                                                \
        }                                                                  \
    } while (0)
// one window's timeline across the grid (DVS_PERSIST_DEBUG prints it): slot `which` of the traced window
#define P_TRACE(which)                                                                             \
    do {                                                                                           \
        if (tid == 0 && (epoch == 12 || epoch == 24 || epoch == 36 || epoch == 48))               \
            sync->trace[epoch / 12 - 1][which][blockIdx.x] = __builtin_amdgcn_s_memrealtime();     \
    } while (0)
#define P_TRACE_G(slot)                                                                            \
    do {                                                                                           \
        if (tid == 0 && (epoch == 12 || epoch == 24 || epoch == 36 || epoch == 48))               \
            sync->trace[epoch / 12 - 1][3][slot] = __builtin_amdgcn_s_memrealtime();               \
    } while (0)
#endif  // DVS_PROBE
#else
#define P_STAMP(k) do { } while (0)
#define P_STAMP_B0(k) do { } while (0)
#define P_TRACE(which) do { } while (0)
#define P_TRACE_G(slot) do { } while (0)
#define P_PROBE_BEGIN(id) do { } while (0)
#define P_PROBE_END(id) do { } while (0)
#endif
// A -DDVS_PERSIST_CHAOS build holds pseudo-randomly chosen workgroups back (one in sixteen up to ~10 us, one in four
// thousand for ~60 us) at the points where they are about to write or read a word another workgroup reads or
// writes: the answers must not change
// (scripts/chaos.sh runs the parity suite and the repeat script against such a build).
#ifdef DVS_PERSIST_CHAOS
#define P_CHAOS(k)                                                                                         \
    do {                                                                                                   \
        uint32_t h_ = (epoch * 0x9E3779B1u) ^ ((blockIdx.x + 1u) * 0x85EBCA77u) ^ (uint32_t(k) * 0xC2B2AE3Du); \
        h_ ^= h_ >> 15;                                                                                    \
        h_ *= 0x27D4EB2Fu;                                                                                 \
        h_ ^= h_ >> 13;                                                                                    \
        if ((h_ & 15u) == 0u)                                                                              \
            for (uint32_t z_ = (h_ >> 8) & 31u; z_ > 0; z_--) __builtin_amdgcn_s_sleep(12);               \
        if ((h_ & 0xFFF0u) == 0x1230u) /* now and then for the length of several windows (~60 us) */      \
            for (uint32_t z_ = 0; z_ < 160; z_++) __builtin_amdgcn_s_sleep(14);                            \
    } while (0)
#else
#define P_CHAOS(k) do { } while (0)
#endif
