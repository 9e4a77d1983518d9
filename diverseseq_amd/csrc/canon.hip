// Canonical (strand-independent) k-mer count rows: a count matrix folded onto the representatives min(idx, rc(idx))
// (include/dvs_hip.h "canonical k-mer count rows"; no counterpart in the reference, whose only canonical form is the
// mash sketch's, src/distance.rs:17-19,65-87).  One pass over the source rows: a row is staged in LDS with 16-byte
// loads, the two bins of every representative are gathered from there, the folded row leaves with 16-byte streaming
// stores and its entropy is reduced in the same pass, as the histogram's flush does.  Bound by the bytes it moves.
#include "canon_host.h"
#include "dvs_internal.h"

#include <algorithm>

namespace {

constexpr int CLOG_TBL = 256;            // c log2 c is looked up below this count, as in kmer_hist.hip
constexpr uint32_t SMALL_ROW = 1024;     // source rows up to this many bytes: a wave per row, four rows per workgroup
constexpr uint32_t LDS_ROW_MAX = 65536;  // source rows beyond this many bytes are gathered from global memory (L2)

// rc(idx) in registers: all 32 bits reversed (which also swaps the two bits of every digit: swapped back), the 2k
// bits moved down, every digit complemented (d ^ 2).  shift = 32 - 2 k, cmask = 0xAAAAAAAA >> shift
__device__ __forceinline__ uint32_t canon_rc(uint32_t idx, uint32_t shift, uint32_t cmask) {
    uint32_t x = __brev(idx);
    x = ((x & 0xAAAAAAAAu) >> 1) | ((x & 0x55555555u) << 1);
    return (x >> shift) ^ cmask;
}

// Where 16-byte slot s of a staged row lies in LDS.  Lanes that walk the representatives in order read rc(rep) a power
// of four apart: unswizzled, 32 lanes on one bank.  The higher slot bits are folded onto the low three, so that such
// a walk spreads over the 8 slots of a bank row (4 lanes to a bank at worst: far above what HBM feeds a CU) and a slot
// stays one 16-byte store.  A bijection of [0, n) for n < 8 (the identity) and for every multiple of 8.
__device__ __forceinline__ uint32_t canon_slot(uint32_t s) {
    return s ^ ((s >> 3) & 7u) ^ ((s >> 6) & 7u) ^ ((s >> 9) & 7u);
}

__device__ __forceinline__ double clog2c(uint32_t c, const double *tbl) {
    if (c < CLOG_TBL) return tbl[c];
    const double d = double(c);
    return d * log2(d);
}

// Workgroups stride over groups of `teams` rows; team t of a workgroup (blockDim.x / teams threads, whole waves) folds
// row g * teams + t.  LDS: [teams staged rows, each padded to 16 bytes (STAGED)] [tbl 256 f64] [one f64 per wave].
// VEC: representatives per thread and step -- 1, or as many as a 16-byte store holds when that divides C (k >= 3).
template <typename T, int VEC, bool STAGED>
__global__ __launch_bounds__(512) void canon_fold_kernel(
    const T *__restrict__ in, T *__restrict__ out, const uint32_t *__restrict__ reps,
    const uint32_t *__restrict__ in_totals, uint32_t *__restrict__ out_totals, double *__restrict__ entropy,
    uint32_t nrows, uint64_t B, uint32_t C, uint32_t k, uint32_t teams) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr uint32_t PER_SLOT = 16 / sizeof(T), SLOT_SHIFT = sizeof(T) == 2 ? 3 : 2;
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    const uint32_t tthreads = nthr / teams, team = tid / tthreads, ttid = tid % tthreads;
    const uint64_t row_bytes = B * sizeof(T);
    const bool slots = (row_bytes & 15) == 0;  // (only the 8-byte rows of 16-bit counts at k = 1 are not whole slots)
    const size_t row_lds = STAGED ? size_t((row_bytes + 15) & ~15ull) : 0;
    double *tbl = reinterpret_cast<double *>(smem + teams * row_lds);
    double *scratch = tbl + CLOG_TBL;
    for (uint32_t i = tid; i < CLOG_TBL; i += nthr) tbl[i] = i ? double(i) * log2(double(i)) : 0.0;
    const uint32_t shift = 32 - 2 * k, cmask = 0xAAAAAAAAu >> shift;
    const uint32_t ngroups = (nrows + teams - 1) / teams;
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint32_t r = g * teams + team;
        const bool live = r < nrows;
        const T *src = in + uint64_t(live ? r : 0) * B;
        T *lrow = reinterpret_cast<T *>(smem + team * row_lds);
        __syncthreads();  // the table is written; the last group's gathers are done with the staged rows
        if (STAGED && live) {
            if (slots) {
                const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
                uint4 *l4 = reinterpret_cast<uint4 *>(lrow);
                const uint32_t nslots = uint32_t(row_bytes >> 4);
                for (uint32_t s = ttid; s < nslots; s += tthreads) l4[canon_slot(s)] = s4[s];
            } else {
                for (uint32_t i = ttid; i < uint32_t(B); i += tthreads) lrow[i] = src[i];
            }
        }
        __syncthreads();
        double sum = 0.0;
        if (live) {
            auto count_at = [&](uint32_t idx) -> uint32_t {
                if (!STAGED) return src[idx];
                if (!slots) return lrow[idx];
                return lrow[(canon_slot(idx >> SLOT_SHIFT) << SLOT_SHIFT) | (idx & (PER_SLOT - 1))];
            };
            T *dst = out + uint64_t(r) * C;
            for (uint32_t c = ttid * VEC; c < C; c += tthreads * VEC) {
                uint32_t rep[VEC], v[VEC];
                if constexpr (VEC == 1) {
                    rep[0] = reps[c];
                } else {
#pragma unroll
                    for (int q = 0; q < VEC / 4; q++) {
                        const uint4 w = reinterpret_cast<const uint4 *>(reps + c)[q];
                        rep[4 * q] = w.x, rep[4 * q + 1] = w.y, rep[4 * q + 2] = w.z, rep[4 * q + 3] = w.w;
                    }
                }
#pragma unroll
                for (int j = 0; j < VEC; j++) {
                    const uint32_t other = canon_rc(rep[j], shift, cmask);
                    v[j] = count_at(rep[j]) + (other != rep[j] ? count_at(other) : 0u);  // (a palindrome counts once)
                    sum += clog2c(v[j], tbl);
                }
                // written once, read by a later selection or distance stage: streaming stores, as the histogram's flush
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                if constexpr (VEC == 1) {
                    dst[c] = T(v[0]);
                } else if constexpr (sizeof(T) == 4) {
                    __builtin_nontemporal_store((u32x4){v[0], v[1], v[2], v[3]}, reinterpret_cast<u32x4 *>(dst + c));
                } else {
                    __builtin_nontemporal_store((u32x4){v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16),
                                                        v[6] | (v[7] << 16)},
                                                reinterpret_cast<u32x4 *>(dst + c));
                }
            }
        }
        // sum of c log2 c over the team's row: the waves of a team in a fixed order, the same bits on every run
        sum = dvs_wave_sum(sum);
        if ((tid & 63) == 0) scratch[tid >> 6] = sum;
        __syncthreads();
        if (live && ttid == 0) {
            const uint32_t waves = tthreads >> 6;
            double acc = 0.0;
            for (uint32_t w = 0; w < waves; w++) acc += scratch[team * waves + w];
            const uint32_t tot = in_totals[r];  // (folding moves counts between bins: the total stays)
            out_totals[r] = tot;
            entropy[r] = tot ? log2(double(tot)) - acc / double(tot) : 0.0;
        }
    }
}

// the representatives of k on the device: built once per k and kept by the context
int canon_reps_device(dvs_ctx *ctx, uint32_t k, uint64_t C, const uint32_t **out) {
    auto it = ctx->canon_reps.find(k);
    if (it != ctx->canon_reps.end()) {
        *out = it->second;
        return DVS_OK;
    }
    std::vector<uint32_t> reps(C);
    if (dvs_canon_bins(k, reps.data(), nullptr) != DVS_OK)
        return dvs_set_error(ctx, DVS_ERR_RUNTIME, "canonical bins of k = %u could not be listed", k);
    uint32_t *d = nullptr;
    const int rc = dvs_dev_alloc(ctx, (void **)&d, C * sizeof(uint32_t), "canonical representatives");
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(d, reps.data(), C * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // (the host list goes with this scope)
    if (e != hipSuccess) {
        dvs_dev_free(ctx, d);
        return dvs_hip_fail(ctx, e, "upload of the canonical representatives");
    }
    ctx->canon_reps[k] = d;
    *out = d;
    return DVS_OK;
}

template <typename T>
int canon_launch(dvs_ctx *ctx, const T *in, T *out, const uint32_t *d_reps, const dvs_matrix *m, dvs_matrix *f) {
    const uint64_t B = m->nbins, row_bytes = B * sizeof(T);
    const uint32_t C = uint32_t(f->nbins), nrows = m->nrows;
    const size_t tail = (CLOG_TBL + 8) * sizeof(double);
    const bool staged = row_bytes <= LDS_ROW_MAX && ((row_bytes + 15) & ~15ull) + tail <= ctx->lds_per_block;
    const uint32_t teams = staged && row_bytes <= SMALL_ROW ? 4 : 1;
    // 512 threads where a staged row leaves room for two workgroups a CU at most: sixteen waves instead of eight
    const uint32_t threads = staged && row_bytes > 32768 ? 512 : 256;
    const size_t lds = (staged ? teams * size_t((row_bytes + 15) & ~15ull) : 0) + tail;
    constexpr int WIDE = 16 / sizeof(T);
    const bool wide = C % WIDE == 0;
    const uint32_t ngroups = (nrows + teams - 1) / teams;
    // a few workgroups per CU stride over the groups: the table of c log2 c is made once per workgroup, not per row
    const size_t by_lds = std::max<size_t>(1, (160u << 10) / lds), by_waves = 2048 / threads;
    const uint32_t per_cu = uint32_t(std::min<size_t>(8, std::min(by_lds, by_waves)));
    const uint32_t grid = std::min<uint32_t>(ngroups, uint32_t(std::max(ctx->n_cu, 1)) * per_cu);
    int rc = DVS_OK;
#define DVS_CANON_LAUNCH(VEC, STAGED)                                                                             \
    do {                                                                                                          \
        rc = dvs_raise_dyn_lds(ctx, reinterpret_cast<const void *>(canon_fold_kernel<T, VEC, STAGED>), lds);      \
        if (!rc)                                                                                                  \
            hipLaunchKernelGGL((canon_fold_kernel<T, VEC, STAGED>), dim3(grid), dim3(threads), lds, ctx->stream, in, out, \
                               d_reps, m->d_totals, f->d_totals, f->d_entropy, nrows, B, C, m->k, teams);         \
    } while (0)
    if (wide && staged) DVS_CANON_LAUNCH(WIDE, true);
    else if (wide) DVS_CANON_LAUNCH(WIDE, false);
    else if (staged) DVS_CANON_LAUNCH(1, true);
    else DVS_CANON_LAUNCH(1, false);
#undef DVS_CANON_LAUNCH
    if (rc) return rc;
    DVS_HIP(ctx, hipGetLastError());
    return DVS_OK;
}

}  // namespace

extern "C" {

int dvs_canonical_bins(uint32_t k, uint32_t *reps_out, uint64_t *n_out) {
    if (!reps_out && !n_out) return dvs_set_error(nullptr, DVS_ERR_VALUE, "null argument");
    if (!dvs_canon_count(k))
        return dvs_set_error(nullptr, DVS_ERR_VALUE, "canonical bins are defined for k in 1..%u, not %u", DVS_CANON_MAX_K, k);
    return dvs_canon_bins(k, reps_out, n_out);
}

uint32_t dvs_matrix_is_canonical(const dvs_matrix *m) { return m && m->canonical ? 1u : 0u; }

int dvs_matrix_fold_canonical(dvs_ctx *ctx, const dvs_matrix *m, dvs_matrix **out) {
    const char *why = dvs_canon_fold_refusal(!ctx || !m || !out, m ? m->kind : 0, m ? m->num_states : 4, m && m->canonical);
    if (why) return dvs_set_error(ctx, DVS_ERR_VALUE, "%s", why);
    *out = nullptr;
    if (m->device != ctx->device)
        return dvs_set_error(ctx, DVS_ERR_VALUE, "the matrix lives on device %d, the context on device %d", m->device, ctx->device);
    const uint64_t C = dvs_canon_count(m->k);
    if (!C) return dvs_set_error(ctx, DVS_ERR_VALUE, "canonical bins are defined for k in 1..%u, not %u", DVS_CANON_MAX_K, m->k);
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    dvs_matrix *f = nullptr;  // (16-bit rows stay 16-bit: a folded count is at most the row's total)
    int rc = dvs_matrix_new(ctx, m->kind, m->nrows, C, m->k, m->num_states, &f);
    if (rc) return rc;
    f->canonical = true;
    const uint32_t *d_reps = nullptr;
    if (m->nrows) rc = canon_reps_device(ctx, m->k, C, &d_reps);
    // enqueued on the context's stream, which holds the source's build (or the wait for the rest of a split one)
    if (!rc && m->nrows)
        rc = m->kind == 2 ? canon_launch<uint16_t>(ctx, m->d_counts16, f->d_counts16, d_reps, m, f)
                          : canon_launch<uint32_t>(ctx, m->d_counts, f->d_counts, d_reps, m, f);
    // the totals of the first rows travel back in the call's wait, as a waited build's do (a selection's seeds)
    f->h_head_totals.assign(std::min<size_t>(m->nrows, 4096), 0u);
    if (!rc && !f->h_head_totals.empty() &&
        hipMemcpyAsync(f->h_head_totals.data(), f->d_totals, f->h_head_totals.size() * 4, hipMemcpyDeviceToHost,
                       ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        f->h_head_totals.clear();
    }
    if (m->nrows) {
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess && !rc) rc = dvs_hip_fail(ctx, e, "canonical fold");
    }
    if (rc) dvs_matrix_destroy(f);
    else *out = f;
    return rc;
}

}  // extern "C"
