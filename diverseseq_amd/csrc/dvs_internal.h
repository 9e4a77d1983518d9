// Internal declarations shared by the translation units of libdvs_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/dvs_hip.h"

#define DVS_EPS 2.220446049250313e-16  // f64::EPSILON
#define DVS_HEAD_ROWS 1024u            // rows of a split build's first launch (kmer_hist.hip)

// Every switch the library takes from the environment, read ONCE when a context is made (and again
// only on dvs_ctx_refresh_knobs, a measurement / test aid): nothing on a per-call path calls getenv.
// All of them are measurement aids or escape hatches; the defaults are the product.
struct dvs_knobs {
    // The library's environment switches, read once per context (and again by dvs_ctx_refresh_knobs).  Every one
    // is listed in INTEGRATION.md with the test or measurement that uses it; there are no others.
    // k-mer matrices (kmer_hist.hip, api.cpp)
    bool no_uniform_offsets = false;  // DVS_NO_UNIFORM_OFFSETS: sequences of one length still get an offsets array on the device
    bool no_offsets_cache = false;    // DVS_NO_OFFSETS_CACHE: every build validates and uploads its offsets
    bool counts_u32 = false;          // DVS_COUNTS_U32: never 16-bit rows
    bool build_wait = false;          // DVS_BUILD_WAIT: device-resident builds wait for their kernels (no split build)
    bool no_packed_upload = false;    // DVS_NO_PACKED_UPLOAD: host sequences cross PCIe one byte per base
    bool cu_mask_set = false;         // HSA_CU_MASK / ROC_GLOBAL_CU_MASK present: the device reports CUs it will not give
    // selection engines (select.hip, persist.hip)
    bool no_fast_step = false;        // DVS_NO_FAST_STEP: the stepwise (row-sharded) mode runs scan / resolve / leave-one-out / finalize per step, as rounds 1-4 did
    bool no_persist = false;          // DVS_NO_PERSIST: the multi-launch engine serves every selection
    bool no_head_phase = false;       // DVS_NO_HEAD_PHASE: no head phase on the CU-masked stream beside the histogram
    bool persist_no_seeded = false;   // DVS_PERSIST_NO_SEEDED: the set-up kernels build the initial set
    bool persist_no_small = false;    // DVS_PERSIST_NO_SMALL: small sets use the general instantiation
    bool persist_no_coarse = false;   // DVS_PERSIST_NO_COARSE: no all-f32 tier in front of the f32-log tier
    bool persist_no_events = false;   // DVS_PERSIST_NO_EVENTS: a threshold no row reaches, long windows (the pure-stream measurement)
    bool persist_debug = false;       // DVS_PERSIST_DEBUG: per-launch report on stderr (phase stamps of a -DDVS_PERSIST_STAMPS build)
    int persist_wg_rounds = -1;       // DVS_PERSIST_WG_ROUNDS: rounds of the grid up to which a window is scanned a row per workgroup (-1: default)
    // rectangular distances (crossdist.hip)
    uint32_t cross_strip_rows = 0;    // DVS_CROSS_STRIP_ROWS: query rows per strip of the rectangular drivers (0: from the strip's byte bound)
    // farthest-first selection (maxmin.hip)
    uint32_t maxmin_batch = 0;        // DVS_MAXMIN_BATCH: steps enqueued between two reads of the status word (0: 64)
    uint32_t kmedoids_batch = 0;      // DVS_KMEDOIDS_BATCH: swap rounds enqueued between two reads of the status word (0: 8)
    uint32_t permanova_batch = 0;     // DVS_PERMANOVA_BATCH: label vectors (the observed one and permutations) a pass over the matrix serves (0: 16; 32 at most)
    uint32_t mantel_batch = 0;        // DVS_MANTEL_BATCH: permutations (the identity among them) a scoring pass of the Mantel test serves (0: 32, which is also the most)
    bool maxmin_jsd_cross = false;    // DVS_MAXMIN_JSD_CROSS: the jsd traversal runs jsd_cross_kernel on one query row (the A/B of DESIGN.md 4.13)
    // ingest
    bool ingest_no_stream = false;    // DVS_INGEST_NO_STREAM: host files are uploaded whole before they are parsed
    // test-only (DVS_TEST_KNOBS=fake_persist_error): the first persistent launch's outcome is read as SEL_ERROR
    bool test_persist_fake_error = false;
    // test-only (DVS_TEST_KNOBS=long_tile_<n>): long rows are cut into tiles of n windows whatever the input's size
    // (the tiles only grow beyond 32768 windows for inputs of 2^27 bases and more: kmer_hist.hip dvs_hist_prepare)
    uint32_t test_long_tile = 0;
    // test-only (DVS_TEST_KNOBS=rowlog_ring_<n>): the stepwise selections' device-side ring of accepted rows holds n rows
    // (>= 4), so that a few dozen accepts wrap it several times before a tie is arbitrated
    uint32_t test_rowlog_ring = 0;
    // test-only (DVS_TEST_KNOBS=poison_blocks): every block dvs_dev_alloc hands out, cached or fresh, is filled with 0xFF
    // bytes over its whole rounded size and the fill waited for; dvs_pinned_get fills its 4 KiB host block likewise.  A
    // read before the first write then sees NaN / all-ones instead of zeros or the last call's values
    bool test_poison_blocks = false;
    // test-only (DVS_TEST_KNOBS=ingest_chunk_<n>): the streamed FASTA upload travels in chunks of n blocks of 128 KiB
    // (clamped to 1 .. 256) instead of 256, so that files of three chunks and more -- the streaming threshold keeps
    // its form -- are a few hundred KiB and every chunk seam can be reached with a small file (0: 256 blocks, 32 MiB)
    uint32_t test_ingest_chunk = 0;
    // test-only (DVS_TEST_KNOBS=ingest_reccap_<n>): the ingest's record arrays start with room for n >= 1 records
    // instead of nbytes / 256 + 2^20, so that a file of a few records overflows them and the last pass is repeated
    uint64_t test_ingest_reccap = 0;
    // test-only (DVS_TEST_KNOBS=refuse_block_<i>, i >= 1): request number i that the context makes of dvs_dev_alloc,
    // dvs_pinned_get or dvs_pinned_grow after it has read its knobs -- served from a cache or not -- is refused, once:
    // NULL and DVS_ERR_NOMEM, the message naming the block and the knob, the runtime not called and no cache touched
    // (0: nothing is refused).  tests/test_gpu_refused_blocks.py walks i over every request of every operation
    uint64_t test_refuse_block = 0;
};
void dvs_knobs_from_env(dvs_knobs *k);

struct dvs_ctx {
    dvs_knobs knobs;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t stream2 = nullptr;  // second stream (created on first use): a selection's set-up kernels beside
                                    // the histogram of the rest of the matrix
    // The CU split (created on first use, dvs_ctx_cu_split): `stream_head` may only use head_cus CUs
    // (the same number on every XCD), `stream_rest` only the others.  A split build runs the histogram
    // of everything behind the head rows on stream_rest while the selection's set-up and the HEAD
    // PHASE of its persistent engine -- the event-dense first rows of the stream, a chain of
    // hand-overs that keeps no CU busy -- run on stream_head beside it (kmer_hist.hip, select.hip).
    hipStream_t stream_head = nullptr, stream_rest = nullptr;
    int head_cus = 0;
    bool cu_split_tried = false;
    // persistent launches of this context that timed out at a grid barrier in a row (their workgroups
    // were not all resident): after three of them later selections go straight to the multi-launch
    // engine; one that runs to its end clears the count
    int persist_timeouts = 0;
    int n_cu = 0;
    size_t lds_per_block = 0;  // max dynamic LDS a block may ask for
    double *d_clog_tbl = nullptr;  // c log2 c, c < 256 (kmer_hist.hip)
    bool timing = false;
    std::string err;
    // device-memory cache: blocks released by dvs_dev_free are kept by size and
    // handed back by dvs_dev_alloc, so a steady-state loop (build matrix, select,
    // destroy) performs no hipMalloc / hipFree.  Released for real in
    // dvs_ctx_destroy, dvs_ctx_trim or when an allocation fails.
    std::multimap<size_t, void *> pool;
    std::vector<void *> pinned_pool;       // 4 KiB pinned host blocks (control-block mirrors)
    std::vector<hipEvent_t> event_pool;    // recycled HIP events
    std::map<void *, size_t> live;
    size_t pool_bytes = 0;
    // what dvs_ctx_block_stats reports beside `live`: the requests made of dvs_dev_alloc, dvs_pinned_get and
    // dvs_pinned_grow since the knobs were last read (refused ones too), and the 4 KiB pinned blocks handed out and not
    // yet put back
    uint64_t block_requests = 0;
    uint64_t pinned_out = 0;
    // one reference for the owner (dropped by dvs_ctx_destroy) and one per matrix, selection and
    // sequence batch made from this context: their destroy functions hand blocks back to the caches
    // above, so the context outlives them whatever order the caller tears things down in
    int refs = 1;
    bool owner_gone = false;
    std::map<const void *, size_t> lds_raised;  // kernels whose dynamic-LDS limit was raised, and to what
    std::map<std::pair<const void *, size_t>, bool> persist_fits;  // (kernel, LDS bytes) -> a 512-thread workgroup fits a CU
    // The offsets of the last histogram build, on both sides (kmer_hist.hip): a caller that builds
    // again over the same sequences -- same offsets, k, byte count, compared by content -- skips the
    // validation pass, the tile lists and their uploads (~0.1 ms of host time per 100k sequences,
    // during which the GPU would wait for its first launch).
    struct OffsetsCache {
        // the offsets on the host, in PINNED memory: the validation pass writes them there and the upload
        // reads them from there, so it is a real asynchronous copy (a pageable source is staged by the
        // runtime inside the call); ev_up marks the last upload that read the block
        uint64_t *h_off = nullptr;
        size_t h_cap = 0, n_off = 0;  // capacity / valid entries (nseq + 1)
        hipEvent_t ev_up = nullptr;
        // host sources of the other uploads: pageable memory an async copy may still read after the
        // call returned, so they live as long as the cache entry
        std::vector<uint32_t> h_long_rows;
        std::vector<unsigned char> h_tiles;
        uint64_t nbytes = 0;
        uint32_t k = 0;
        void *d_off = nullptr, *d_rows = nullptr, *d_tiles = nullptr;
        size_t d_off_cap = 0;
        size_t n_long = 0, n_tiles = 0;
        // the last build's sequences all had one length and lay end to end: no offsets on the device
        bool uniform = false;
        uint64_t uni_base = 0, uni_stride = 0;
        // a build that was not waited for may still read d_off / d_rows / d_tiles: the stream is drained before one of
        // them goes back to the block cache (dvs_hist_prepare)
        bool lists_in_flight = false;
    } off_cache;
    // packed upload of host sequences (pack.hip): the pinned staging block, kept between calls, and the
    // event behind the last copy that read it; PERMANOVA's label vectors travel through the same block (dvs_pinned_stage)
    void *h_pack = nullptr;
    size_t h_pack_cap = 0;
    hipEvent_t pack_ev = nullptr;
    // canonical fold (canon.hip): k -> the C(k) representatives min(idx, rc(idx)) on the device, uploaded on first use
    std::map<uint32_t, uint32_t *> canon_reps;
};
// hipFuncAttributeMaxDynamicSharedMemorySize >= bytes for kernel fn on this context's device
int dvs_raise_dyn_lds(dvs_ctx *ctx, const void *fn, size_t bytes);
void dvs_ctx_retain(dvs_ctx *ctx);
hipStream_t dvs_ctx_stream2(dvs_ctx *ctx);  // NULL when it cannot be created
bool dvs_ctx_cu_split(dvs_ctx *ctx);         // stream_head / stream_rest exist (false: no CU masks here)
void dvs_ctx_release(dvs_ctx *ctx);

// waits for a build that is still in flight (no-op otherwise) and moves the head totals to the vector
struct dvs_matrix;
int dvs_matrix_settle(dvs_ctx *ctx, const dvs_matrix *m);
int dvs_dev_alloc(dvs_ctx *ctx, void **ptr, size_t bytes, const char *what);
void dvs_dev_free(dvs_ctx *ctx, void *ptr);
void dvs_dev_trim(dvs_ctx *ctx);
// A block of that cache, handed back on scope exit.  dvs_dev_free gives the block to the next allocation at once:
// the scope ends only after the stream work that uses the block has been waited for.
struct PooledBuf {
    dvs_ctx *ctx;
    void *p = nullptr;
    ~PooledBuf() { dvs_dev_free(ctx, p); }
    template <typename T>
    T *as() { return static_cast<T *>(p); }
};
int dvs_pinned_get(dvs_ctx *ctx, void **ptr);  // 4 KiB pinned block from the ctx cache
// a pinned block of `bytes` of its own, for the two staging blocks that grow (ctx->h_pack, the offsets cache's h_off):
// counted and refusable like the others, not cached -- its owner keeps it and frees it with hipHostFree
int dvs_pinned_grow(dvs_ctx *ctx, void **ptr, size_t bytes, const char *what);
// pack.hip: ctx->h_pack, the context's large pinned staging block, with room for `bytes` and read by nobody any more; a
// user that does not wait for its last copy out of the block records ctx->pack_ev behind it
int dvs_pinned_stage(dvs_ctx *ctx, size_t bytes, const char *what);
void dvs_pinned_put(dvs_ctx *ctx, void *ptr);
hipEvent_t dvs_event_get(dvs_ctx *ctx);
void dvs_event_put(dvs_ctx *ctx, hipEvent_t e);

int dvs_set_error(dvs_ctx *ctx, int code, const char *fmt, ...);
int dvs_hip_fail(dvs_ctx *ctx, hipError_t e, const char *what);

#define DVS_HIP(ctx, call)                                        \
    do {                                                          \
        hipError_t e__ = (call);                                  \
        if (e__ != hipSuccess) return dvs_hip_fail(ctx, e__, #call); \
    } while (0)

// N x B matrix resident in HBM.  kind 0: uint32 counts; kind 1: f64 freqs; kind 2: uint16 counts
// (a build in which every sequence is a single tile of <= 32768 windows: no count can reach 2^16,
// and both streaming phases -- the build's write, the scan's read -- move half the bytes).
struct dvs_matrix {
    int kind = 0;
    uint16_t *d_counts16 = nullptr;  // kind 2
    uint32_t nrows = 0;
    uint64_t nbins = 0;
    uint32_t k = 0, num_states = 0;
    uint32_t *d_counts = nullptr;  // kind 0
    double *d_freqs = nullptr;     // kind 1
    uint32_t *d_totals = nullptr;  // valid k-mers per row (kind 1: 1 for every row)
    double *d_entropy = nullptr;   // H(row freq vector), bits
    uint32_t *d_src_row = nullptr; // kind 1 built from flagged device rows: row r came from input row d_src_row[r]
    // totals of the first rows as the builder left them (copied in the build's own stream sync):
    // the selectors need their seeds' totals on the host and would otherwise pay a round trip
    std::vector<uint32_t> h_head_totals;
    // ... or, for a build that did not wait for its kernels (device-resident input), still on their
    // way: a pinned block the copy lands in and the event recorded behind it
    uint32_t *h_head_pinned = nullptr;
    hipEvent_t ev_built = nullptr;
    hipEvent_t ev_join = nullptr;  // split build: recorded behind the rest-of-matrix launch, waited for by the context's stream
    uint32_t head_count = 0;
    // rows [0, head_rows_built) were built by a launch of their own, finished when ev_built fires; the
    // rest of the matrix may still be in flight on the context's stream after that (0: no such split)
    uint32_t head_rows_built = 0;
    // ... and that rest was launched on the context's stream_rest (CU split): the head CUs are free
    // for a selection's head phase until the context's stream, which waits for it, moves on
    bool rest_beside_head = false;
    // the build was not waited for and nothing has drained the context's stream behind it yet (a selection's poll does):
    // dvs_matrix_free_fields drains it before the rows, totals and entropies go back to the block cache, where a
    // selection's set-up may take them and write them on a side stream that nothing orders behind the histogram
    bool in_flight = false;
    // count rows folded onto the canonical bins of k (canon.hip): nbins = C(k), everything else as the source's kind
    bool canonical = false;
    int device = 0;
    dvs_ctx *ctx = nullptr;  // owner of the allocations
};
// api.cpp: a new matrix of that kind and shape (k, num_states: 0 for frequency rows) with its device blocks allocated
// and nothing written; nothing is left behind on failure.  A constructor that fails later hands it to dvs_matrix_destroy.
int dvs_matrix_new(dvs_ctx *ctx, int kind, uint32_t nrows, uint64_t nbins, uint32_t k, uint32_t num_states, dvs_matrix **out);
// kmer_hist.hip: what the constructors of api.cpp enqueue, and the release of a matrix's blocks
uint64_t dvs_pow_u64(uint32_t base, uint32_t exp, bool *overflow);
void dvs_matrix_free_fields(dvs_matrix *m);
int dvs_hist_prepare(dvs_ctx *ctx, const uint64_t *offsets, uint32_t nseq, uint32_t k, uint64_t nbins, uint64_t nbytes, size_t *n_long_out);
bool dvs_hist_rows_fit_u16(const dvs_ctx *ctx, uint64_t B, size_t n_long);
int dvs_matrix_fill_freq_entropy(dvs_ctx *ctx, dvs_matrix *m);
int dvs_matrix_fill_freq_totals(dvs_ctx *ctx, dvs_matrix *m, const double *d_meta);
int dvs_matrix_fill_compacted(dvs_ctx *ctx, dvs_matrix *m, const double *d_in, const double *d_meta);

// Four-state sequences in HBM at 3 bits per base (pack.hip, pack_host.cpp): positions index the
// concatenated buffer exactly as in the one-byte form, so a batch's offsets are the same in both.
//   d_codes[w]: bases 16 w .. 16 w + 15, two bits each, base 16 w in bits 31..30
//   d_mask[w]:  bit 15 - i set when base 16 w + i is invalid (>= 4, or behind the end of the buffer)
// nwords = ceil(nbases / 16) words of each plane are valid; the planes are allocated a little longer
// (a multiple of 16 bytes) so that vector loads near the end stay inside them.
struct dvs_packed {
    dvs_ctx *ctx = nullptr;
    uint32_t *d_codes = nullptr;
    uint16_t *d_mask = nullptr;
    uint64_t nbases = 0, nwords = 0;
    // kernels that read the planes were enqueued without being waited for (a build over the planes, dvs_seqs_bring
    // -- on the context's stream or, for a split build, its stream_rest): the planes go back to the block cache,
    // which orders reuse on the context's stream only, so dvs_packed_destroy drains those streams first
    mutable bool async_readers = false;
};
// An ingested file (ingest.hip): the encoded bases of its sequences in HBM, in byte form or packed in place.
struct dvs_seqbatch {
    dvs_ctx *ctx = nullptr;
    uint8_t *d_codes = nullptr;  // total + 16 bytes (the histogram kernel reads 16-byte chunks)
    uint64_t total = 0;
    uint32_t nseq = 0;
    std::vector<uint64_t> offsets;     // nseq + 1
    std::vector<uint64_t> header_pos;  // file offset of the '>' of every record of the file
    dvs_packed *packed = nullptr;      // after dvs_seqbatch_pack: the bases at 3 bits each (d_codes released)
    // the alphabet the batch was encoded with puts the four bases first (the library's own DNA / RNA table): only
    // then is "symbol >= 4" the same as "not a base" and the batch may be re-stated in the packed form
    bool four_state_alphabet = false;
    // builds over d_codes that were not waited for (dvs_seqs_bring: the context's stream or, for a split build,
    // its stream_rest): dvs_seqbatch_destroy drains those streams before the block goes back
    mutable bool async_readers = false;
};
// what the kernels take: either the byte form (seqs) or the packed planes
struct dvs_seq_view {
    const uint8_t *seqs = nullptr;  // one byte per base ...
    const uint32_t *codes = nullptr;  // ... or the packed planes (codes != NULL)
    const uint16_t *mask = nullptr;
    uint64_t nbytes = 0;  // readable bases
};
int dvs_packed_alloc(dvs_ctx *ctx, uint64_t nbases, dvs_packed **out);                       // pack.hip
int dvs_packed_fill_from_device(dvs_ctx *ctx, dvs_packed *p, const uint8_t *d_seqs);         // bytes in HBM -> planes
int dvs_packed_fill_from_host(dvs_ctx *ctx, dvs_packed *p, const uint8_t *seqs);             // host threads pack, chunks cross PCIe packed
bool dvs_packed_upload_wanted(const dvs_ctx *ctx, uint32_t num_states, uint64_t nbytes);
extern "C" void dvs_pack_bases(const uint8_t *src, size_t n, uint32_t *codes, uint16_t *mask);  // pack_host.cpp
unsigned dvs_host_threads();  // pack.hip: host cores this process may use (cgroup quota respected), at most 16

// ---- a build's sequences (include/dvs_hip.h dvs_seqs) on the device, as the histogram and the sketcher take them
// pack.hip.  What both build entries check before anything else, host work only: DVS_ERR_VALUE for a NULL context,
// source, offsets or handle (bytes: unless the batch has no bases), an unknown kind, and num_states != 4 over packed
// planes.
int dvs_seqs_check(dvs_ctx *ctx, const dvs_seqs *src, uint32_t num_states);
inline uint32_t dvs_seqs_count(const dvs_seqs *src) {  // of a checked source
    return src->kind == DVS_SEQ_BATCH ? static_cast<const dvs_seqbatch *>(src->handle)->nseq : src->nseq;
}
// The view of a checked source, with whatever was made for the call: host bytes are uploaded -- packed (k <= 32 and
// dvs_packed_upload_wanted) or as they are, in a buffer padded to a multiple of 16 bytes plus 16 whose tail is 0xFF --
// and everything else is used where it lies.  When the object goes it waits for the context's stream and hands the
// upload's blocks back to the cache: a consumer only enqueues.
struct dvs_seqs_held {
    dvs_seq_view view;
    const uint64_t *offsets = nullptr;  // host, nseq + 1
    uint32_t nseq = 0;
    bool resident = false;  // the sequences were in HBM already: nothing here makes a build wait for its kernels
    PooledBuf bytes;                // HOST: the upload buffer ...
    dvs_packed *planes = nullptr;   // ... or the planes of the packed upload
    explicit dvs_seqs_held(dvs_ctx *ctx) : bytes{ctx} {}
    dvs_seqs_held(const dvs_seqs_held &) = delete;
    ~dvs_seqs_held();
};
// pack.hip, the only maker of that view.  A PACKED or BATCH source is marked as read by kernels nobody waits for
// (async_readers), so it is called only when something will be enqueued.
int dvs_seqs_bring(dvs_ctx *ctx, const dvs_seqs *src, uint32_t k, uint32_t num_states, dvs_seqs_held *held);
int dvs_matrix_fill_counts(dvs_ctx *ctx, dvs_matrix *m, const dvs_seq_view &sv, bool no_wait);  // kmer_hist.hip

// linkage.hip's prepare pass on its own, enqueued on the context's stream: every entry of the n x n matrix checked and
// the upper triangle copied over the lower one; the bits below are OR-ed into the device word *d_status (`sign`: a
// negative entry above the diagonal is flagged too)
constexpr uint32_t DVS_LNK_NONFINITE = 1, DVS_LNK_NEGATIVE = 4;
hipError_t dvs_linkage_enqueue_prepare(dvs_ctx *ctx, double *d_dist, uint32_t n, bool sign, uint32_t *d_status);

// linkage.hip, host only: the in-order walk of the tree behind dvs_linkage's outputs (include/dvs_hip.h "cophenetic
// distances"): order[n] the leaves in dendrogram order, pos[n] its inverse, gap[n - 1] the merge between positions p
// and p + 1, *c_bar the mean of all cophenetic distances.  DVS_ERR_VALUE for n < 2 or a pair that names a cluster not
// yet made or already merged; the heights need not be monotone.
int dvs_cophenet_walk(dvs_ctx *ctx, uint32_t n, const uint32_t *pairs, const double *heights, uint32_t *order,
                      uint32_t *pos, uint32_t *gap, double *c_bar);

// One consumer of a whole n x n f64 distance matrix in HBM, as the square driver of rowdist.hip takes it: what differs
// between the linkage tree, the neighbour-joining tree, the principal coordinates, k-medoids and PERMANOVA.  The driver brings the
// matrix -- a MASH, EUCLIDEAN or JSD source's kernels enqueued, a caller's host matrix uploaded, a caller's device
// matrix where it is -- and calls run.  On entry to run: check has passed, the context's device is set, the matrix and
// extra_bytes() beside it have been found to fit, and the matrix is resident or enqueued on the context's stream.  run
// enqueues behind it, returns once the host outputs are written, and may return an error with work still queued: the
// driver drains the stream before the matrix goes back to the block cache.
struct dvs_square_consumer {
    const char *name;                     // the entry, in front of the driver's own messages: "dvs_kmedoids"
    std::function<int()> check;           // the arguments, then n: DVS_OK, or the error it set
    std::function<bool()> early;          // optional, staged sources only: true when it has answered with no cell computed
    std::function<size_t()> extra_bytes;  // what run allocates beside the matrix (asked once check has passed) ...
    char extra_what[48];                  // ... and its noun phrase in the DVS_ERR_NOMEM message: "its tree"
    bool writes_matrix;                   // run overwrites the matrix (a caller's device matrix is used in place either way)
    // d_zerodiv (may be NULL): a word the distance kernels set where the reference divides by zero, reported as
    // DVS_ERR_ZERODIV before anything else
    std::function<int(double *d_dist, const uint32_t *d_zerodiv)> run;
};
// the consumers, built by their entries (n: the source's; given: a DVS_SRC_GIVEN source, where the wording or the
// early answer differs)
struct dvs_kmedoids_out {
    uint32_t *medoids, *labels;
    double *dist, *second;
    uint32_t *swaps;
    double *td;
    dvs_kmedoids_info *info;
};
dvs_square_consumer dvs_linkage_consumer(dvs_ctx *ctx, uint32_t n, bool given, int method, uint32_t *pairs, double *heights,
                                         uint32_t *sizes);                                                     // linkage.hip
dvs_square_consumer dvs_nj_consumer(dvs_ctx *ctx, uint32_t n, uint32_t *joins, double *lengths);                // nj.hip
dvs_square_consumer dvs_pcoa_consumer(dvs_ctx *ctx, uint32_t n, const dvs_pcoa_params *p, double *values, double *vectors,
                                      double *residuals, double *row_means, dvs_pcoa_info *info);              // pcoa.hip
dvs_square_consumer dvs_kmedoids_consumer(dvs_ctx *ctx, uint32_t n, bool given, const dvs_kmedoids_params *p,
                                          const dvs_kmedoids_out &out);                                        // kmedoids.hip
struct dvs_permanova_args {  // dvs_permanova's, behind the source
    const uint32_t *labels;
    uint32_t n_groups;
    const uint32_t *perm_labels;
    uint32_t n_perm;
    double *ss_total, *ss_within, *group_ss;
    dvs_permanova_info *info;
};
dvs_square_consumer dvs_permanova_consumer(dvs_ctx *ctx, uint32_t n, const dvs_permanova_args &a);           // permanova.hip
// mantel.hip: dvs_mantel's arguments behind the two sources, the bytes of a run's state, and the run itself over the two
// matrices in HBM (rowdist.hip's entry brings them)
struct dvs_mantel_args {
    const uint32_t *perms;
    uint32_t n_perm;
    double *moments, *z;
    dvs_mantel_info *info;
};
size_t dvs_mantel_state_bytes(const dvs_ctx *ctx, uint32_t n, uint32_t n_perm);
int dvs_mantel_run(dvs_ctx *ctx, uint32_t n, const double *d_x, double *d_y, bool y_owned, const uint32_t *d_zerodiv_x,
                   const uint32_t *d_zerodiv_y, const dvs_mantel_args &a);
// A run's status words: `bytes` of them zeroed on the context's stream, then the distance kernels' zero-division word
// (d_zerodiv, may be NULL) copied into word `at`.
inline hipError_t dvs_status_begin(dvs_ctx *ctx, uint32_t *d_status, size_t bytes, uint32_t at, const uint32_t *d_zerodiv) {
    hipError_t e = hipMemsetAsync(d_status, 0, bytes, ctx->stream);
    if (e == hipSuccess && d_zerodiv) e = hipMemcpyAsync(d_status + at, d_zerodiv, 4, hipMemcpyDeviceToDevice, ctx->stream);
    return e;
}

// rowdist.hip, what every operation over a whole n x n matrix shares (op, may be NULL: the entry's name, put in front
// of the message as "<op>: ").
// DVS_ERR_NOMEM unless the matrix (need_matrix: it is still to be allocated) and extra_bytes beside it fit the device
// with the context's cached blocks counted as free; extra_what: the noun phrase for what the extra bytes hold.
int dvs_square_fits(dvs_ctx *ctx, const char *op, uint32_t n, bool need_matrix, size_t extra_bytes, const char *extra_what);
// DVS_ERR_VALUE unless a caller's matrix that claims to be on the device is device memory of the context's device
int dvs_given_on_device(dvs_ctx *ctx, const char *op, const void *dist);
// a caller's n x n host matrix into a block of the cache, the copy enqueued on the context's stream (an error: drained)
int dvs_given_upload(dvs_ctx *ctx, const double *dist, uint32_t n, PooledBuf *d_dist);

// One distance mode of ctree, as the drivers of rowdist.hip take it: "fill this device n x n f64 matrix" on the
// context's stream, with what differs from mode to mode beside it.
struct dvs_dist_stage {
    const char *label;                // what a failed launch is reported as
    uint32_t n;                       // rows and columns of the matrix
    std::function<int()> check;       // the mode's own precondition: DVS_OK, or the error it set
    size_t scratch_bytes;             // extra device scratch of the kernels (0: none) ...
    const char *scratch_what;         // ... and its name in an allocation error
    bool scratch_is_zerodiv;          // the scratch is a word the kernel sets where the reference divides by zero
    bool zero_diagonal;               // the kernels do not write the diagonal: it is zeroed in front of them
    std::function<hipError_t(double *d_dist, void *d_scratch)> enqueue;
};
dvs_dist_stage dvs_mash_stage(dvs_ctx *ctx, const dvs_sketches *sk, uint32_t k, uint32_t sketch_size);  // mash.hip

// One distance mode between two collections, as the drivers of crossdist.hip take it: "fill rows [q0, q0 + mq) of the
// m x n f64 matrix into this device buffer (mq x n, row-major)" on the context's stream.  The matrix never has to
// exist whole: the drivers walk the queries in strips.
struct dvs_cross_stage {
    const char *label;                // what a failed launch is reported as
    uint32_t m, n;                    // query rows and reference columns of the matrix
    std::function<int()> check;       // the mode's own preconditions: DVS_OK, or the error it set
    size_t scratch_bytes;             // device scratch shared by every strip ...
    const char *scratch_what;         // ... and its name in an allocation error
    bool scratch_is_zerodiv;          // its first word is set by the kernel where the reference divides by zero
    std::function<hipError_t(void *d_scratch)> prepare;  // once, in front of the first strip
    std::function<hipError_t(uint32_t q0, uint32_t mq, double *d_strip, void *d_scratch)> enqueue;
};
// d_q_rows (may be NULL) here and below: the query list already on the device -- nq entries that the kernels of a
// strip read when they run, so that a kernel enqueued in front of them may still write them (maxmin.hip); q_rows is
// then not looked at
dvs_cross_stage dvs_mash_cross_stage(dvs_ctx *ctx, const dvs_sketches *q, const uint32_t *q_rows, uint32_t nq,
                                     const dvs_sketches *r, const uint32_t *r_rows, uint32_t nr, uint32_t k,
                                     uint32_t sketch_size, const uint32_t *d_q_rows = nullptr);  // mash.hip
dvs_cross_stage dvs_euclid_cross_stage(dvs_ctx *ctx, const dvs_matrix *q, const uint32_t *q_rows, uint32_t nq,
                                       const dvs_matrix *r, const uint32_t *r_rows, uint32_t nr,
                                       const uint32_t *d_q_rows = nullptr);  // crossdist.hip
// crossdist.hip: jsd_entropy_kernel over the rows d_rows[p] (NULL: p), p < count, of m into d_h, on the context's stream
hipError_t dvs_jsd_entropies_enqueue(dvs_ctx *ctx, const dvs_matrix *m, const uint32_t *d_rows, uint32_t count, double *d_h);
// crossdist.hip: jsd_cross_kernel on ONE query row -- row d_q_rows[q0] of m, entropy d_hq[q0] -- against rows 0 .. n - 1 of
// m (entropies d_hr) into d_row[n], on the context's stream
hipError_t dvs_jsd_cross_row_enqueue(dvs_ctx *ctx, const dvs_matrix *m, const uint32_t *d_q_rows, uint32_t q0, uint32_t n,
                                     const double *d_hq, const double *d_hr, double *d_row);
int dvs_rows_check(dvs_ctx *ctx, uint32_t n);  // rowdist.hip: the square path's own row limit
// a side's optional row list (host; NULL: rows 0 .. nrows - 1) against the `limit` rows its handle holds
int dvs_cross_rows_check(dvs_ctx *ctx, const uint32_t *rows, uint32_t nrows, uint32_t limit, const char *side);
// The two optional row lists of a stage in its scratch, behind `head` bytes of the stage's own: uploaded once, read by
// the kernels of every strip.  (The host lists are the caller's and outlive the call, which waits for the stream.)
struct dvs_cross_lists {
    size_t head;
    const uint32_t *q_rows, *r_rows;
    uint32_t nq, nr;
    const uint32_t *d_q_rows = nullptr;  // the query list where it already is on the device: used as it is, q_rows ignored
    size_t bytes() const { return head + (up_q() ? size_t(nq) * 4 : 0) + (r_rows ? size_t(nr) * 4 : 0); }
    bool up_q() const { return q_rows && !d_q_rows; }
    const uint32_t *dq(void *scratch) const {
        if (d_q_rows) return d_q_rows;
        return q_rows ? reinterpret_cast<const uint32_t *>(static_cast<char *>(scratch) + head) : nullptr;
    }
    const uint32_t *dr(void *scratch) const {
        return r_rows ? reinterpret_cast<const uint32_t *>(static_cast<char *>(scratch) + head) + (up_q() ? nq : 0) : nullptr;
    }
    hipError_t upload(dvs_ctx *ctx, void *scratch) const {
        hipError_t e = hipSuccess;
        if (up_q() && nq)
            e = hipMemcpyAsync(const_cast<uint32_t *>(dq(scratch)), q_rows, size_t(nq) * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && r_rows && nr)
            e = hipMemcpyAsync(const_cast<uint32_t *>(dr(scratch)), r_rows, size_t(nr) * 4, hipMemcpyHostToDevice, ctx->stream);
        return e;
    }
};

// One consumer of an m x n f64 distance matrix that arrives strip by strip, as the strip driver of crossdist.hip
// (dvs_strip_run) takes it.  An operation checks its own arguments, fills one of these in with lambdas that capture its
// locals by reference, and calls the driver: the stage's check, the device, the strip height, the strip and the
// stage's scratch, the stage's prepare, begin, strip behind each strip's distance kernels, the zero-division word, ONE
// hipStreamSynchronize, then the errors (begin's; an enqueue's; the synchronisation's; DVS_ERR_ZERODIV).  THE DRAIN
// IS THE DRIVER'S: whatever begin or strip return, the stream is waited for before the driver returns -- so an
// operation never synchronises on account of an error, and its PooledBufs and the host memory its uploads read need
// only be locals of the function that calls the driver.  The host work behind the drain follows the call.
struct dvs_strip_consumer {
    // optional: the blocks beside the strip (`rows`: the strip's height) and the uploads; DVS_OK, or the error it set
    std::function<int(uint32_t rows)> begin;
    std::function<hipError_t(uint32_t q0, uint32_t mq, double *d_strip)> strip;  // enqueued behind rows [q0, q0 + mq)
    const bool *stop;  // optional: set by strip when no further strip is wanted
};
int dvs_strip_run(dvs_ctx *ctx, const dvs_cross_stage &st, const dvs_strip_consumer &c);  // crossdist.hip
constexpr uint32_t DVS_NONE = 0xFFFFFFFFu;  // no row, no column, no cluster
constexpr uint32_t DVS_TOPK_MAX = 64;       // the most nearest references, and axes of a projection, per query
// the operations over a stage, called by the entries of crossdist.hip
int dvs_nearest_strips(dvs_ctx *ctx, const dvs_cross_stage &st, uint32_t kk, uint32_t *idx, double *dist);  // nearest.hip
int dvs_pcoa_project_strips(dvs_ctx *ctx, const dvs_cross_stage &st, uint32_t n_axes, const double *values,
                            const double *vectors, const double *row_means, double *coords);  // pcoa.hip
int dvs_cluster_scores_strips(dvs_ctx *ctx, const dvs_cross_stage &st, const uint32_t *labels, uint32_t n_clusters,
                              double *within, double *a, double *b, uint32_t *neighbour, double *silhouette,
                              uint32_t *medoids);  // clusters.hip
int dvs_cophenet_strips(dvs_ctx *ctx, const dvs_cross_stage &st, const uint32_t *pairs, const double *heights, double *corr,
                        double *row_sums, double *coph);  // cophenet.hip
int dvs_within_strips(dvs_ctx *ctx, const dvs_cross_stage &st, double radius, uint32_t flags, uint64_t max_pairs,
                      dvs_pairs **out);  // within.hip
int dvs_threshold_clusters_strips(dvs_ctx *ctx, const dvs_cross_stage &st, double radius, uint32_t *labels,
                                  uint32_t *n_clusters);  // within.hip
int dvs_mst_strips(dvs_ctx *ctx, const dvs_cross_stage &st, const double *core, uint32_t *edges, double *weights,
                   uint32_t *n_edges, uint32_t *n_rounds);  // mst.hip

// ---- an operation's source (include/dvs_hip.h dvs_source): the tag in front of the stages above
uint32_t dvs_sketches_nseq(const dvs_sketches *sk);  // mash.hip, whose struct it is
inline const dvs_matrix *dvs_src_matrix(const dvs_source *s) { return static_cast<const dvs_matrix *>(s->handle); }
inline const dvs_sketches *dvs_src_sketches(const dvs_source *s) { return static_cast<const dvs_sketches *>(s->handle); }
// rowdist.hip.  What every entry checks before anything else, in place of what typed handles used to guarantee (r ==
// q for an operation over one source): DVS_ERR_VALUE for a NULL context, source or handle, an unknown kind, a row
// list with GIVEN, two sides of different kinds, two MASH sides of different k or sketch size
int dvs_source_check(dvs_ctx *ctx, const dvs_source *q, const dvs_source *r);
// DVS_ERR_UNSUPPORTED, "<op>: <what> of a <kind> source": a combination no entry has served
int dvs_source_refuse(dvs_ctx *ctx, const char *op, const dvs_source *src, const char *what);
// ... for a row list, or n other than the handle's rows (the square drivers take a handle whole)
int dvs_source_whole(dvs_ctx *ctx, const char *op, const dvs_source *src);

// f(typed row pointer) for the matrix's element type
template <typename F>
auto dvs_mat_dispatch(const dvs_matrix *m, F &&f) {
    if (m->kind == 0) return f(static_cast<const uint32_t *>(m->d_counts));
    if (m->kind == 2) return f(static_cast<const uint16_t *>(m->d_counts16));
    return f(static_cast<const double *>(m->d_freqs));
}

// ---- device helpers -------------------------------------------------------
#ifdef __HIPCC__
// 4 bases (little-endian bytes, earliest base in the low byte) -> 8 bits, the earliest base in the TOP two bits
__device__ __forceinline__ uint32_t dvs_pack4(uint32_t w) {
    const uint32_t x = w & 0x03030303u;
    return ((x << 6) | (x >> 4) | (x >> 14) | (x >> 24)) & 0xFFu;
}
// 4 bases -> 4 bits, bit set where the byte is >= 4, earliest base in bit 3
__device__ __forceinline__ uint32_t dvs_inv4(uint32_t w) {
    uint32_t t = w & 0xFCFCFCFCu;
    t |= t >> 4;
    t |= t >> 2;
    t |= t >> 1;
    t &= 0x01010101u;
    return ((t << 3) | (t >> 6) | (t >> 15) | (t >> 24)) & 0xFu;
}
// 16 bases -> a code word / a mask word of the packed form (dvs_packed)
__device__ __forceinline__ uint32_t dvs_pack16(uint4 v) {
    return (dvs_pack4(v.x) << 24) | (dvs_pack4(v.y) << 16) | (dvs_pack4(v.z) << 8) | dvs_pack4(v.w);
}
__device__ __forceinline__ uint32_t dvs_inv16(uint4 v) {
    return (dvs_inv4(v.x) << 12) | (dvs_inv4(v.y) << 8) | (dvs_inv4(v.z) << 4) | dvs_inv4(v.w);
}
__device__ __forceinline__ double dvs_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the same sum by DPP (register cross-lane moves, no LDS crossbar): ~23 instructions where the
// shuffle form needs 12 ds_bpermute round trips; every lane gets the total
template <int CTRL>
__device__ __forceinline__ double dvs_dpp_mov(double v) {
    const long long b = __double_as_longlong(v);
    int lo = int(b), hi = int(b >> 32);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
__device__ __forceinline__ double dvs_wave_sum_dpp(double v) {
    v += dvs_dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dvs_dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dvs_dpp_mov<0x141>(v);  // row_half_mirror
    v += dvs_dpp_mov<0x140>(v);  // row_mirror: every lane holds the sum of its row of 16
    const long long b = __double_as_longlong(v);
    const int lo = int(b), hi = int(b >> 32);
    auto row = [&](int l) {
        return __longlong_as_double((long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, l) << 32) |
                                                (unsigned)__builtin_amdgcn_readlane(lo, l)));
    };
    return (row(0) + row(16)) + (row(32) + row(48));
}
__device__ __forceinline__ double dvs_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
// the same minimum by DPP (the minimum does not depend on the order it is taken in: the same bits)
__device__ __forceinline__ double dvs_wave_min_dpp(double v) {
    v = fmin(v, dvs_dpp_mov<0xB1>(v));
    v = fmin(v, dvs_dpp_mov<0x4E>(v));
    v = fmin(v, dvs_dpp_mov<0x141>(v));
    v = fmin(v, dvs_dpp_mov<0x140>(v));
    const long long b = __double_as_longlong(v);
    const int lo = int(b), hi = int(b >> 32);
    auto row = [&](int l) {
        return __longlong_as_double((long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, l) << 32) |
                                                (unsigned)__builtin_amdgcn_readlane(lo, l)));
    };
    return fmin(fmin(row(0), row(16)), fmin(row(32), row(48)));
}
__device__ __forceinline__ unsigned long long dvs_wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// Sum over the block; every thread gets the result.  scratch: >= 17 doubles of LDS.
// Fixed tree -> the same inputs always give the same bits.
__device__ __forceinline__ double dvs_block_sum(double v, double *scratch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nwave = (blockDim.x + 63) >> 6;
    v = dvs_wave_sum(v);
    __syncthreads();  // scratch may still be read from a previous call
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < nwave; i++) t += scratch[i];
    return t;
}
__device__ __forceinline__ double dvs_block_min(double v, double *scratch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nwave = (blockDim.x + 63) >> 6;
    v = dvs_wave_min(v);
    __syncthreads();
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    double t = scratch[0];
    for (int i = 1; i < nwave; i++) t = fmin(t, scratch[i]);
    return t;
}
#endif
