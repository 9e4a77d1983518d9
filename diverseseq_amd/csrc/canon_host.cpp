// Canonical k-mer bins, the host part (include/dvs_hip.h "canonical k-mer count rows"): the reverse complement of a
// k-mer index, the list of representatives, and the argument checks of dvs_matrix_fold_canonical.  Plain C++ with no
// HIP and no other file of the library behind it, so that it also compiles on its own (scripts/micro/canon_host_check.cpp
// builds it under the host sanitizers).
#include "canon_host.h"

// first base most significant (src/record.rs:18-29); the complement of a digit is d ^ 2 ((base + 2) % 4,
// src/distance.rs:18)
uint32_t dvs_canon_rc(uint32_t idx, uint32_t k) {
    uint32_t out = 0;
    for (uint32_t i = 0; i < k; i++) {
        out = (out << 2) | ((idx & 3u) ^ 2u);
        idx >>= 2;
    }
    return out;
}

// C(k) = 4^k / 2 for odd k (no k-mer is its own reverse complement), (4^k + 4^(k/2)) / 2 for even k (the 4^(k/2)
// palindromes are their own); 0 outside 1 .. DVS_CANON_MAX_K
uint64_t dvs_canon_count(uint32_t k) {
    if (k == 0 || k > DVS_CANON_MAX_K) return 0;
    const uint64_t bins = 1ull << (2 * k);
    return (k & 1u) ? bins / 2 : (bins + (1ull << k)) / 2;
}

int dvs_canon_bins(uint32_t k, uint32_t *reps_out, uint64_t *n_out) {
    const uint64_t count = dvs_canon_count(k);
    if (!count || (!reps_out && !n_out)) return DVS_ERR_VALUE;
    if (n_out) *n_out = count;
    if (!reps_out) return DVS_OK;
    const uint64_t bins = 1ull << (2 * k);
    uint64_t at = 0;
    for (uint64_t idx = 0; idx < bins; idx++)
        if (uint32_t(idx) <= dvs_canon_rc(uint32_t(idx), k)) reps_out[at++] = uint32_t(idx);
    return at == count ? DVS_OK : DVS_ERR_RUNTIME;
}

const char *dvs_canon_fold_refusal(bool null_argument, int kind, uint32_t num_states, bool canonical) {
    if (null_argument) return "null argument";
    if (kind == 1) return "a frequency matrix has no k: canonical bins are folded from k-mer counts";
    if (num_states != 4) return "canonical k-mers are defined for four states only";
    if (canonical) return "the matrix is already canonical";
    return nullptr;
}
