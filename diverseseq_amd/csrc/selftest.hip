// Numeric self-tests of the device arithmetic the selection's bands rest on (select_dev.h); they belong to no selection.
#include "dvs_internal.h"
#include "select_dev.h"

namespace {

// max |double(v_log_f32(m)) - log2(m)| over every f32 m in [0.5, 1): the hardware
// term of FAST_BAND.  One thread per 2^11 consecutive mantissas.
__global__ void fast_log2_selftest_kernel(double *out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;  // 4096 threads x 2048 = 2^23
    double worst = 0.0;
    for (uint32_t j = 0; j < 2048; j++) {
        const uint32_t bits = 0x3F000000u + t * 2048u + j;  // [0.5, 1)
        const float m = __uint_as_float(bits);
        const double err = fabs(double(__builtin_amdgcn_logf(m)) - log2(double(m)));
        worst = fmax(worst, err);
    }
    for (int o = 32; o > 0; o >>= 1) worst = fmax(worst, __shfl_xor(worst, o, 64));
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *p = reinterpret_cast<unsigned long long *>(out);
        atomicMax(p, (unsigned long long)__double_as_longlong(worst));  // positive doubles order as ints
    }
}

}  // namespace

// max |log2_acc(x) - log2(x)| / max(1, |log2 x|), and the same of log2_tab, over 2^17 mantissas x 80 exponents
__global__ void log2_acc_selftest_kernel(double *out) {
    __shared__ double2 tab[128];
    if (threadIdx.x < 128) log2_tab_fill(tab, threadIdx.x);
    __syncthreads();
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;  // 2^17 threads
    double worst = 0.0;
    for (int e = -78; e <= 1; e++) {
        // mantissas spread over [1, 2), plus a dense cluster around sqrt(2) and 1
        const double m = 1.0 + double(t) / 131072.0;
        const double xs[3] = {ldexp(m, e), ldexp(1.4142135623730951 + (double(t) - 65536.0) * 1e-12, e),
                              ldexp(1.0 + (double(t) - 65536.0) * 2.2e-16, e)};
        for (int q = 0; q < 3; q++) {
            const double ref = log2(xs[q]);
            const double err = fabs(log2_acc(xs[q]) - ref) / fmax(1.0, fabs(ref));
            const double err_t = fabs(log2_tab(xs[q], tab) - ref) / fmax(1.0, fabs(ref));
            worst = fmax(worst, fmax(err, err_t));
        }
    }
    for (int o = 32; o > 0; o >>= 1) worst = fmax(worst, __shfl_xor(worst, o, 64));
    if ((threadIdx.x & 63) == 0)
        atomicMax(reinterpret_cast<unsigned long long *>(out), (unsigned long long)__double_as_longlong(worst));
}

// COARSE tier (select_dev.h): max over EVERY f32 y in [2^-101, 2) of
// |v_log_f32(y) - log2 y| / (2^-23 max(1, |log2 y|)), the k of its error bound; and the exact
// quotient by fma against the division, over 2^26 (count, total) pairs per launch
__global__ void log2_f32_selftest_kernel(double *out) {
    double worst = 0.0;
    const uint64_t first = uint64_t(26) << 23, last = uint64_t(128) << 23;  // biased exponents 26 .. 127
    for (uint64_t b = first + uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; b < last;
         b += uint64_t(gridDim.x) * blockDim.x) {
        const float y = __uint_as_float(uint32_t(b));
        const double ref = log2(double(y));
        const double err = fabs(double(__builtin_amdgcn_logf(y)) - ref) / (0x1p-23 * fmax(1.0, fabs(ref)));
        worst = fmax(worst, err);
    }
    for (int o = 32; o > 0; o >>= 1) worst = fmax(worst, __shfl_xor(worst, o, 64));
    if ((threadIdx.x & 63) == 0)
        atomicMax(reinterpret_cast<unsigned long long *>(out), (unsigned long long)__double_as_longlong(worst));
}

__global__ void exact_div_selftest_kernel(unsigned long long *bad) {
    const uint64_t t = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    unsigned long long nbad = 0;
    uint64_t x = (t + 1) * 0x9E3779B97F4A7C15ull;
    for (int it = 0; it < 64; it++) {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        uint32_t tot = uint32_t(x >> 32), c = uint32_t(x);
        if (it & 1) tot >>= (x >> 27) & 31;  // short totals too
        if (!tot) tot = 1;
        if (it & 2) c %= tot;  // frequencies proper (c <= tot), and any pair
        const double dt = double(tot);
        if (exact_div_u32(double(c), dt, 1.0 / dt) != double(c) / dt) nbad++;
    }
    // every count up to a small total, exhaustively
    const uint32_t tot = uint32_t(t % 8192) + 1, c0 = uint32_t(t / 8192);
    if (c0 <= tot) {
        const double dt = double(tot);
        if (exact_div_u32(double(c0), dt, 1.0 / dt) != double(c0) / dt) nbad++;
    }
    if (nbad) atomicAdd(bad, nbad);
}

// one launch of `kernel`, which leaves its figure in a zeroed 8-byte word, and that word into *out
template <typename W, typename R>
static int selftest_run(dvs_ctx *ctx, void (*kernel)(W *), dim3 grid, R *out) {
    static_assert(sizeof(W) == 8 && sizeof(R) == 8, "one 8-byte word");
    if (!ctx || !out) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    DVS_HIP(ctx, hipSetDevice(ctx->device));
    PooledBuf word{ctx};  // (waited for on every path below before it goes back to the cache)
    if (int rc = dvs_dev_alloc(ctx, &word.p, 8, "self-test word")) return rc;
    W *d = word.as<W>();
    hipError_t e = hipMemsetAsync(d, 0, 8, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t se = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return dvs_hip_fail(ctx, e, "self-test");
    return DVS_OK;
}

extern "C" int dvs_selftest_log2_f32(dvs_ctx *ctx, double *max_ulps) {
    return selftest_run(ctx, log2_f32_selftest_kernel, dim3(4096), max_ulps);
}
extern "C" int dvs_selftest_exact_div(dvs_ctx *ctx, uint64_t *mismatches) {
    return selftest_run(ctx, exact_div_selftest_kernel, dim3(8192 * 8192 / 256), mismatches);
}
extern "C" int dvs_selftest_log2_acc(dvs_ctx *ctx, double *max_rel_err) {
    return selftest_run(ctx, log2_acc_selftest_kernel, dim3(512), max_rel_err);
}
extern "C" int dvs_selftest_fast_log2(dvs_ctx *ctx, double *max_abs_err) {
    return selftest_run(ctx, fast_log2_selftest_kernel, dim3(16), max_abs_err);
}
