// The neighbours within a radius and the threshold clusters (include/dvs_hip.h "neighbours within a radius", "threshold
// clusters"): each strip of the strip driver (crossdist.hip dvs_strip_run) compacted on the device by the
// three within_* kernels, the list (dvs_pairs) or the union-find kept on the host.  No counterpart in the reference.
#include "dvs_internal.h"

#include <algorithm>
#include <cmath>
#include <memory>

namespace {

// The cells of a strip (mq x n) that lie within a radius, as a list per row in ascending column order (include/dvs_hip.h
// "neighbours within a radius"): three kernels over the strip as the distance kernels left it.  A row is cut into
// segments of WITHIN_SEG columns and one wave takes one (row, segment) item, 64 consecutive columns a step (lane l
// column c + l: coalesced).  A wave and not a workgroup per item because a row of a tall strip is a few cells long
// and a long row has n / WITHIN_SEG items of its own, so that either shape fills the device; the segments' counts
// meet in the scan below, in item order, and not in LDS, which none of the three kernels uses for a row.
//   within_count_kernel  counts[item]: popcount of the ballot of the predicate, summed over the steps
//   within_scan_kernel   offs[item]: the exclusive prefix sum of the counts in item order (row-major: a row's segments
//                        in column order), 64 bits; row_off[r] = base + offs of the row's first item; *total
//   within_write_kernel  the passing cells of an item at offs[item] on: a lane's slot is the running base plus the number
//                        of passing lanes below it (mbcnt of the ballot), the base advances by the ballot's popcount
// The predicate is within_cell, called by both kernels on the same buffer: d <= radius (NaN compares false) over the
// cells the rule lets it read -- every cell, every cell but the row's own position self = q0 + r (WITHIN_NOT_SELF), or
// only the columns above it (WITHIN_ABOVE_SELF: the upper triangle).  A cell the rule excludes is never loaded.  No
// atomics: every position is a function of the strip's bits alone.
constexpr int WITHIN_THREADS = 256;
constexpr uint32_t WITHIN_WAVES = WITHIN_THREADS / 64, WITHIN_SEG = 2048;
constexpr uint32_t WITHIN_ALL = 0, WITHIN_NOT_SELF = 1, WITHIN_ABOVE_SELF = 2;

struct within_seg {
    const double *g;  // the item's strip row
    uint32_t self;    // the row's own position
    uint32_t c0, j1;  // the first step's first column, the end of the segment
};

// item = r * nseg + s: columns [s WITHIN_SEG, min(n, (s + 1) WITHIN_SEG)) of strip row r.  Under WITHIN_ABOVE_SELF the
// steps that lie wholly at or below self hold nothing and are left out (whole steps: a lane keeps its columns)
__device__ __forceinline__ within_seg within_item(const double *strip, uint64_t item, uint32_t n, uint32_t nseg, uint32_t q0,
                                                  uint32_t rule) {
    const uint32_t r = nseg == 1 ? uint32_t(item) : uint32_t(item / nseg);
    const uint32_t j0 = nseg == 1 ? 0u : uint32_t(item % nseg) * WITHIN_SEG;
    within_seg w;
    w.g = strip + uint64_t(r) * n;
    w.self = q0 + r;
    w.j1 = n - j0 < WITHIN_SEG ? n : j0 + WITHIN_SEG;
    w.c0 = j0;
    if (rule == WITHIN_ABOVE_SELF && w.self >= j0) {
        const uint32_t skip = (w.self - j0 + 1) / 64 * 64;
        w.c0 = skip >= w.j1 - j0 ? w.j1 : j0 + skip;
    }
    return w;
}

// whether cell j of the item passes, and its value
__device__ __forceinline__ bool within_cell(const within_seg &w, uint32_t j, uint32_t rule, double radius, double &d) {
    const bool read = j < w.j1 && !(rule == WITHIN_NOT_SELF && j == w.self) && !(rule == WITHIN_ABOVE_SELF && j <= w.self);
    d = read ? w.g[j] : NAN;
    return d <= radius;
}

__global__ __launch_bounds__(WITHIN_THREADS) void within_count_kernel(const double *__restrict__ strip, uint32_t n,
                                                                      uint32_t nseg, uint64_t items, uint32_t q0,
                                                                      uint32_t rule, double radius,
                                                                      uint32_t *__restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t item = uint64_t(blockIdx.x) * WITHIN_WAVES + (threadIdx.x >> 6);
    if (item >= items) return;  // (the whole wave)
    const within_seg w = within_item(strip, item, n, nseg, q0, rule);
    uint32_t count = 0;
    for (uint32_t c = w.c0; c < w.j1; c += 64) {
        double d;
        count += uint32_t(__popcll(__ballot(within_cell(w, c + lane, rule, radius, d))));
    }
    if (lane == 0) counts[item] = count;
}

// One workgroup, looping: SCAN_CHUNK items a turn, SCAN_ITEMS consecutive ones per thread -- a thread over its own, the 64
// lanes by shuffle-up, the waves and the turns before through LDS and a carry every thread keeps.  Integer sums: exact in
// any shape.  items / SCAN_CHUNK turns of a load, one barrier (the waves' sums alternate between two LDS buffers, so a
// turn's readers need no second one) and a store: ~3 000 turns for the tallest strip there is, 11 million rows over 3
// references, and one turn for a strip of up to 4 096 items.
constexpr int SCAN_THREADS = 1024, SCAN_ITEMS = 4;
constexpr uint32_t SCAN_WAVES = SCAN_THREADS / 64, SCAN_CHUNK = SCAN_THREADS * SCAN_ITEMS;
__global__ __launch_bounds__(SCAN_THREADS) void within_scan_kernel(const uint32_t *__restrict__ counts, uint64_t items,
                                                                   uint32_t nseg, uint64_t base, uint64_t *__restrict__ offs,
                                                                   uint64_t *__restrict__ row_off,
                                                                   uint64_t *__restrict__ total) {
    __shared__ uint32_t s_top[2][SCAN_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t carry = 0;  // the sum of the turns before
    uint32_t flip = 0;
    for (uint64_t i0 = 0; i0 < items; i0 += SCAN_CHUNK) {
        const uint64_t t0 = i0 + uint64_t(tid) * SCAN_ITEMS;
        uint32_t c[SCAN_ITEMS];
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; k++) c[k] = t0 + k < items ? counts[t0 + k] : 0u;
        uint32_t mine = 0;  // (a turn's sum stays below 2^32: SCAN_CHUNK x WITHIN_SEG = 2^23)
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; k++) mine += c[k];
        uint32_t incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(incl, o, 64);
            if (lane >= uint32_t(o)) incl += u;
        }
        if (lane == 63) s_top[flip][wave] = incl;
        __syncthreads();  // (two buffers: the writers of the turn after next have passed the next turn's barrier)
        uint32_t before = 0, turn = 0;
#pragma unroll
        for (uint32_t x = 0; x < SCAN_WAVES; x++) {
            const uint32_t top = s_top[flip][x];
            if (x < wave) before += top;
            turn += top;
        }
        flip ^= 1;
        uint64_t at = carry + before + (incl - mine);
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; k++) {
            const uint64_t item = t0 + k;
            if (item < items) {
                offs[item] = at;
                if (nseg == 1)
                    row_off[item] = base + at;
                else if (item % nseg == 0)
                    row_off[item / nseg] = base + at;
            }
            at += c[k];
        }
        carry += turn;
    }
    if (tid == 0) *total = carry;
}

// dist may be NULL (the positions alone: the threshold clusters)
__global__ __launch_bounds__(WITHIN_THREADS) void within_write_kernel(const double *__restrict__ strip, uint32_t n,
                                                                      uint32_t nseg, uint64_t items, uint32_t q0,
                                                                      uint32_t rule, double radius,
                                                                      const uint64_t *__restrict__ offs,
                                                                      uint32_t *__restrict__ col, double *__restrict__ dist) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t item = uint64_t(blockIdx.x) * WITHIN_WAVES + (threadIdx.x >> 6);
    if (item >= items) return;  // (the whole wave)
    const within_seg w = within_item(strip, item, n, nseg, q0, rule);
    uint64_t at = offs[item];
    for (uint32_t c = w.c0; c < w.j1; c += 64) {
        double d;
        const bool pass = within_cell(w, c + lane, rule, radius, d);
        const unsigned long long mask = __ballot(pass);
        if (pass) {
            const uint64_t slot = at + __builtin_amdgcn_mbcnt_hi(uint32_t(mask >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mask), 0u));
            col[slot] = c + lane;
            if (dist) dist[slot] = d;
        }
        at += uint64_t(__popcll(mask));
    }
}

// The cells within `radius` of a stage, strip by strip: ready() -> DVS_OK or the error it set, once the stage has passed
// its check (the caller's own host memory); the three within_* kernels behind each strip's distances, then the strip's
// number of pairs read back and waited for (the one synchronisation per strip: the host has to know how much to take,
// and whether max_pairs -- 0: no limit -- is passed), then sink(q0, mq, base, count, d_row_off, d_col, d_dist) -> DVS_OK
// or the error it set: the strip's `count` pairs lie at d_col / d_dist (NULL unless want_dist) in row order,
// d_row_off[r] is base plus the pairs in front of strip row r, base the pairs of the strips before.  What sink enqueues
// on the context's stream is done before the next sink is called, and when this returns.  The pair buffers hold the
// worst case of one strip; a negative radius is passed on as NaN, which no cell is within.
template <typename Ready, typename Sink>
int cross_within_walk(dvs_ctx *ctx, const dvs_cross_stage &st, double radius, uint32_t rule, bool want_dist,
                      uint64_t max_pairs, uint64_t *n_pairs, Ready &&ready, Sink &&sink) {
    const uint32_t n = st.n, nseg = (n + WITHIN_SEG - 1) / WITHIN_SEG;
    PooledBuf d_scan{ctx}, d_col{ctx}, d_dist{ctx};  // d_scan: offs [items], row_off [rows], the total; then counts [items]
    uint64_t *d_offs, *d_row_off, *d_total;
    uint32_t *d_counts;
    const double r_eff = radius < 0.0 ? double(NAN) : radius;
    uint64_t base = 0, over = 0;
    bool stop = false;
    int sink_rc = DVS_OK;
    dvs_strip_consumer c{};
    c.begin = [&](uint32_t rows) {
        if (int rc = ready()) return rc;
        const uint64_t max_items = uint64_t(rows) * nseg, cap = uint64_t(rows) * n;
        if ((max_items + WITHIN_WAVES - 1) / WITHIN_WAVES > 0x7FFFFFFFull)
            return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "a strip of %u rows: more row segments than a grid takes", rows);
        int rc = dvs_dev_alloc(ctx, &d_scan.p, size_t(max_items + rows + 1) * 8 + size_t(max_items) * 4, "within counts and offsets");
        if (!rc) rc = dvs_dev_alloc(ctx, &d_col.p, size_t(cap) * 4, "within positions");
        if (!rc && want_dist) rc = dvs_dev_alloc(ctx, &d_dist.p, size_t(cap) * 8, "within distances");
        d_offs = d_scan.as<uint64_t>(), d_row_off = d_offs + max_items, d_total = d_row_off + rows;
        d_counts = reinterpret_cast<uint32_t *>(d_total + 1);
        return rc;
    };
    c.strip = [&](uint32_t q0, uint32_t mq, double *d_strip) {
        const uint64_t items = uint64_t(mq) * nseg;
        const dim3 grid(uint32_t((items + WITHIN_WAVES - 1) / WITHIN_WAVES));
        hipLaunchKernelGGL(within_count_kernel, grid, dim3(WITHIN_THREADS), 0, ctx->stream, d_strip, n, nseg, items, q0, rule,
                           r_eff, d_counts);
        hipLaunchKernelGGL(within_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, d_counts, items, nseg, base,
                           d_offs, d_row_off, d_total);
        hipLaunchKernelGGL(within_write_kernel, grid, dim3(WITHIN_THREADS), 0, ctx->stream, d_strip, n, nseg, items, q0, rule,
                           r_eff, d_offs, d_col.as<uint32_t>(), d_dist.as<double>());
        hipError_t e = hipGetLastError();
        uint64_t count = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&count, d_total, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return e;
        if (max_pairs && base + count > max_pairs) {
            over = base + count;
            stop = true;
            return hipSuccess;
        }
        sink_rc = sink(q0, mq, base, count, d_row_off, d_col.as<uint32_t>(), d_dist.as<double>());
        stop = sink_rc != DVS_OK;
        base += count;
        return hipSuccess;
    };
    c.stop = &stop;
    if (int rc = dvs_strip_run(ctx, st, c)) return rc;
    if (sink_rc) return sink_rc;
    if (over)
        return dvs_set_error(ctx, DVS_ERR_UNSUPPORTED, "%llu pairs within the radius so far: more than max_pairs = %llu",
                             (unsigned long long)over, (unsigned long long)max_pairs);
    *n_pairs = base;
    return DVS_OK;
}

constexpr uint32_t WITHIN_FLAGS = DVS_WITHIN_SKIP_SELF;

}  // namespace

// a CSR list of (query position, reference position, distance) on the host
struct dvs_pairs {
    std::vector<uint64_t> row_start;  // [n_rows + 1]
    std::vector<uint32_t> col;
    std::vector<double> dist;
};

// the cells within `radius` of a stage into a new dvs_pairs (include/dvs_hip.h "neighbours within a radius")
int dvs_within_strips(dvs_ctx *ctx, const dvs_cross_stage &st, double radius, uint32_t flags, uint64_t max_pairs,
                      dvs_pairs **out) {
    if (!out) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    *out = nullptr;
    if (radius != radius) return dvs_set_error(ctx, DVS_ERR_VALUE, "the radius cannot be NaN");
    if (flags & ~WITHIN_FLAGS) return dvs_set_error(ctx, DVS_ERR_VALUE, "unknown flag bits 0x%x", flags & ~WITHIN_FLAGS);
    std::unique_ptr<dvs_pairs> p;
    try {
        p.reset(new dvs_pairs);
        p->row_start.assign(size_t(st.m) + 1, 0);
    } catch (const std::exception &) {
        return dvs_set_error(ctx, DVS_ERR_NOMEM, "no host memory for the row starts of %u queries", st.m);
    }
    if (st.m == 0 || st.n == 0) {
        *out = p.release();
        return DVS_OK;
    }
    uint64_t total = 0;
    const int rc = cross_within_walk(
        ctx, st, radius, flags & DVS_WITHIN_SKIP_SELF ? WITHIN_NOT_SELF : WITHIN_ALL, true, max_pairs, &total, [] { return DVS_OK; },
        [&](uint32_t q0, uint32_t mq, uint64_t base, uint64_t count, const uint64_t *d_row_off, const uint32_t *d_col,
            const double *d_dist) {
            try {  // (nothing is in flight into the vectors: the walk has waited for the copies of the strip before)
                p->col.resize(size_t(base + count));
                p->dist.resize(size_t(base + count));
            } catch (const std::exception &) {
                return dvs_set_error(ctx, DVS_ERR_NOMEM, "no host memory for %llu pairs", (unsigned long long)(base + count));
            }
            hipError_t e = hipMemcpyAsync(p->row_start.data() + q0, d_row_off, size_t(mq) * 8, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess && count)
                e = hipMemcpyAsync(p->col.data() + base, d_col, size_t(count) * 4, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess && count)
                e = hipMemcpyAsync(p->dist.data() + base, d_dist, size_t(count) * 8, hipMemcpyDeviceToHost, ctx->stream);
            return e == hipSuccess ? DVS_OK : dvs_hip_fail(ctx, e, "within pairs read-back");
        });
    if (rc) return rc;
    p->row_start[st.m] = total;
    *out = p.release();
    return DVS_OK;
}

// The connected components of the graph "distance <= radius" over a stage whose queries and references are the same n
// positions (include/dvs_hip.h "threshold clusters"): the edges of the upper triangle strip by strip through a
// union-find on the host (union by lower root index, path halving), a strip's edges dropped before the next strip's
// arrive; the labels by first appearance in position order -- a component's root is its lowest position.
int dvs_threshold_clusters_strips(dvs_ctx *ctx, const dvs_cross_stage &st, double radius, uint32_t *labels,
                                  uint32_t *n_clusters) {
    const uint32_t n = st.n;
    if (n == 0) return DVS_OK;
    if (!labels || !n_clusters) return dvs_set_error(ctx, DVS_ERR_VALUE, "null argument");
    if (radius != radius) return dvs_set_error(ctx, DVS_ERR_VALUE, "the radius cannot be NaN");
    std::vector<uint32_t> parent, h_col;
    std::vector<uint64_t> h_off;
    auto find = [&](uint32_t x) {
        while (parent[x] != x) {
            parent[x] = parent[parent[x]];
            x = parent[x];
        }
        return x;
    };
    uint64_t total = 0;
    const int rc = cross_within_walk(
        ctx, st, radius, WITHIN_ABOVE_SELF, false, 0, &total,
        [&] {
            try {
                parent.resize(n);
            } catch (const std::exception &) {
                return dvs_set_error(ctx, DVS_ERR_NOMEM, "no host memory for the union-find of %u positions", n);
            }
            for (uint32_t i = 0; i < n; i++) parent[i] = i;
            return DVS_OK;
        },
        [&](uint32_t q0, uint32_t mq, uint64_t base, uint64_t count, const uint64_t *d_row_off, const uint32_t *d_col,
            const double *) {
            if (!count) return DVS_OK;
            try {
                h_col.resize(size_t(count));
                h_off.resize(size_t(mq) + 1);
            } catch (const std::exception &) {
                return dvs_set_error(ctx, DVS_ERR_NOMEM, "no host memory for the %llu edges of a strip", (unsigned long long)count);
            }
            hipError_t e = hipMemcpyAsync(h_off.data(), d_row_off, size_t(mq) * 8, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(h_col.data(), d_col, size_t(count) * 4, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) return dvs_hip_fail(ctx, e, "threshold edges read-back");
            h_off[mq] = base + count;
            for (uint32_t r = 0; r < mq; r++)
                for (uint64_t p = h_off[r] - base; p < h_off[r + 1] - base; p++) {
                    const uint32_t a = find(q0 + r), b = find(h_col[size_t(p)]);
                    if (a != b) parent[a > b ? a : b] = a > b ? b : a;
                }
            return DVS_OK;
        });
    if (rc) return rc;
    uint32_t next = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t root = find(i);
        labels[i] = root == i ? next++ : labels[root];  // (root < i: it has its label)
    }
    *n_clusters = next;
    return DVS_OK;
}

extern "C" void dvs_pairs_destroy(dvs_pairs *p) { delete p; }

extern "C" int dvs_pairs_info(const dvs_pairs *p, uint32_t *n_rows, uint64_t *n_pairs) {
    if (!p) return DVS_ERR_VALUE;
    if (n_rows) *n_rows = uint32_t(p->row_start.size() - 1);
    if (n_pairs) *n_pairs = p->row_start.back();
    return DVS_OK;
}

extern "C" int dvs_pairs_get(const dvs_pairs *p, uint64_t *row_start, uint32_t *col, double *dist) {
    if (!p) return DVS_ERR_VALUE;
    if (row_start) std::copy(p->row_start.begin(), p->row_start.end(), row_start);
    if (col) std::copy(p->col.begin(), p->col.end(), col);
    if (dist) std::copy(p->dist.begin(), p->dist.end(), dist);
    return DVS_OK;
}

