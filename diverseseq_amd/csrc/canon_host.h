// Host part of the canonical fold (canon_host.cpp); include/dvs_hip.h "canonical k-mer count rows" has the definition.
#pragma once

#include <cstdint>

#include "../../include/dvs_hip.h"

constexpr uint32_t DVS_CANON_MAX_K = 16;  // 4^16 bins: the widest dense row (api.cpp build_shape)

uint32_t dvs_canon_rc(uint32_t idx, uint32_t k);  // idx < 4^k, 1 <= k <= 16
uint64_t dvs_canon_count(uint32_t k);             // C(k); 0 for k outside 1 .. 16
// dvs_canonical_bins without the error text: DVS_ERR_VALUE for k outside 1 .. 16 or two NULL outputs
int dvs_canon_bins(uint32_t k, uint32_t *reps_out, uint64_t *n_out);
// why dvs_matrix_fold_canonical refuses these arguments (all DVS_ERR_VALUE, in the header's order), or NULL
const char *dvs_canon_fold_refusal(bool null_argument, int kind, uint32_t num_states, bool canonical);
