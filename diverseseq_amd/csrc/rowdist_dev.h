// What the square (rowdist.hip) and the rectangular (crossdist.hip) Jensen-Shannon kernels share: the tile shape and
// the per-bin term.  A cell is the same bits in both because both go through these.
#pragma once

#include "select_dev.h"

constexpr int JSD_THREADS = 256;
constexpr uint32_t JSD_TILE = 32;    // rows of a tile on either side; a thread owns rows t, t + 16 of both
constexpr uint32_t JSD_CHUNK = 64;   // bins staged at a time
constexpr uint32_t JSD_LD = 2 * JSD_TILE + 1;  // doubles per staged bin: 32 i-rows, 32 j-rows, one of padding

// acc -= m log2 m.  An empty bin (m == 0) takes the logarithm of 2^-1000 instead and adds -0 * -1000, which leaves
// acc as it is: no branch, so the chains of a thread's 2 x 2 block interleave.  (A count row's m is 0 or >= 2^-33.)
__device__ __forceinline__ void jsd_add(double &acc, double m, const double2 *tab) {
    acc = fma(-m, log2_tab(fmax(m, 0x1p-1000), tab), acc);
}

constexpr int EUC_THREADS = 512;
constexpr uint32_t EUC_CHUNK = 4096;  // bins of row i staged at a time (32 KB)
