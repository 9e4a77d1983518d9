// The host part of the canonical fold (diverseseq_amd/csrc/canon_host.cpp: the representatives, rc, the argument
// checks of dvs_matrix_fold_canonical) as a stand-alone program, for the host sanitizers -- no device, no Python:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       scripts/micro/canon_host_check.cpp diverseseq_amd/csrc/canon_host.cpp -o canon_host_check && ./canon_host_check
// Prints "canon host ok" and exits 0; the first mismatch (or sanitizer report) ends it with a non-zero status.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../diverseseq_amd/csrc/canon_host.h"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main() {
    const uint64_t expect[8] = {2, 10, 32, 136, 512, 2080, 8192, 32896};
    for (uint32_t k = 1; k <= 12; k++) {
        uint64_t n = 0;
        CHECK(dvs_canon_bins(k, nullptr, &n) == DVS_OK);
        CHECK(n == dvs_canon_count(k));
        if (k <= 8) CHECK(n == expect[k - 1]);
        // the list into a buffer of exactly C(k) words, guard words of the allocator behind it
        std::vector<uint32_t> reps(n);
        uint64_t n2 = 0;
        CHECK(dvs_canon_bins(k, reps.data(), &n2) == DVS_OK && n2 == n);
        CHECK(dvs_canon_bins(k, reps.data(), nullptr) == DVS_OK);
        const uint64_t bins = 1ull << (2 * k);
        std::vector<unsigned char> seen(bins, 0);
        uint64_t palindromes = 0;
        for (uint64_t c = 0; c < n; c++) {
            const uint32_t rep = reps[c], other = dvs_canon_rc(rep, k);
            CHECK(c == 0 || reps[c - 1] < rep);
            CHECK(rep < bins && other < bins && rep <= other);
            CHECK(dvs_canon_rc(other, k) == rep);  // an involution
            CHECK(!seen[rep] && (other == rep || !seen[other]));
            seen[rep] = seen[other] = 1;
            palindromes += other == rep;
        }
        for (uint64_t i = 0; i < bins; i++) CHECK(seen[i]);
        CHECK(palindromes == ((k & 1) ? 0 : (1ull << k)));
    }
    // T0 C1 A2 G3: TCA = 0b000110 -> TGA = 0b001110; the widest k uses all 32 bits
    CHECK(dvs_canon_rc(0x06, 3) == 0x0E && dvs_canon_rc(0, 3) == 0x2A);
    CHECK(dvs_canon_rc(0, 16) == 0xAAAAAAAAu && dvs_canon_rc(0xAAAAAAAAu, 16) == 0);
    CHECK(dvs_canon_count(16) == (1ull << 31) + (1ull << 15));
    uint64_t n = 7;
    CHECK(dvs_canon_bins(0, nullptr, &n) == DVS_ERR_VALUE && dvs_canon_bins(17, nullptr, &n) == DVS_ERR_VALUE && n == 7);
    CHECK(dvs_canon_bins(3, nullptr, nullptr) == DVS_ERR_VALUE);
    CHECK(dvs_canon_count(0) == 0 && dvs_canon_count(17) == 0 && dvs_canon_count(0xFFFFFFFFu) == 0);
    // the refusals, in the header's order; none for a plain four-state count matrix of either width
    CHECK(std::strcmp(dvs_canon_fold_refusal(true, 1, 5, true), "null argument") == 0);
    CHECK(std::strstr(dvs_canon_fold_refusal(false, 1, 5, true), "frequency matrix"));
    CHECK(std::strstr(dvs_canon_fold_refusal(false, 0, 5, true), "four states"));
    CHECK(std::strstr(dvs_canon_fold_refusal(false, 2, 4, true), "already canonical"));
    CHECK(dvs_canon_fold_refusal(false, 0, 4, false) == nullptr && dvs_canon_fold_refusal(false, 2, 4, false) == nullptr);
    std::puts("canon host ok");
    return 0;
}
