/*
 * dvs_hip.h -- C ABI of libdvs_hip.so: the MI355X (gfx950) implementation of
 * DiverseSeq's k-mer / delta-JSD / mash hot path.
 *
 * This is the drop-in boundary.  It replaces the PyO3 extension module
 * `diverse_seq._dvs` (reference src/lib.rs:175-189): every entry point below
 * names the reference interface it stands in for.  Plain pointers and sizes
 * only; no torch / HIP types in the signatures (a HIP stream crosses as
 * void*).  All functions return 0 (DVS_OK) or a DVS_ERR_* code;
 * dvs_last_error() returns the message (for DVS_ERR_VALUE it is the
 * reference's panic text, which src/lib.rs:36-57 turns into ValueError).
 *
 * Data convention (reference diverse_seq/util.py:41-45, src/distance.rs:6-8):
 * a sequence is one byte per base holding the cogent3 alphabet index
 * (DNA: T0 C1 A2 G3); any byte >= num_states is a gap/ambiguity and
 * invalidates every k-mer window that contains it.  A batch of sequences is
 * one concatenated byte buffer plus nseq+1 uint64 offsets.
 *
 * Threading: one dvs_ctx per process per GPU; a ctx is not thread-safe.
 */
#ifndef DVS_HIP_H
#define DVS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVS_ABI_VERSION 5

#define DVS_OK 0
#define DVS_ERR_VALUE 1       /* the reference would panic -> python ValueError */
#define DVS_ERR_RUNTIME 2     /* HIP failure / no device */
#define DVS_ERR_NOMEM 3
#define DVS_ERR_UNSUPPORTED 4 /* shape outside what the device path handles */
#define DVS_ERR_ZERODIV 5     /* python ZeroDivisionError (distance.py:283) */

typedef struct dvs_ctx dvs_ctx;       /* device, stream, scratch */
typedef struct dvs_matrix dvs_matrix; /* N x num_states^k count (or freq) matrix in HBM */
typedef struct dvs_select dvs_select; /* a SummedRecords set + the greedy engine */

/* ---- context ------------------------------------------------------------ */
int dvs_abi_version(void);
/* device < 0: current device.  stream: a hipStream_t to launch on, or NULL for
 * a stream owned by the ctx. */
int dvs_ctx_create(int device, void *stream, dvs_ctx **out);
/* Drops the caller's reference.  Matrices, selections and sequence batches made from ctx hold
 * one each, so they may be destroyed after it, in any order (a garbage-collected host language
 * gives none); the caches and the stream go when the last reference does.  ctx itself must not
 * be passed to another call afterwards. */
void dvs_ctx_destroy(dvs_ctx *ctx);
/* message of the last failing call on ctx (ctx == NULL: last ctx_create failure) */
const char *dvs_last_error(const dvs_ctx *ctx);
int dvs_ctx_sync(dvs_ctx *ctx);
/* the ctx caches device allocations released by *_destroy for reuse; this frees them */
int dvs_ctx_trim(dvs_ctx *ctx);
/* name, CU count and HBM bytes of the ctx's device */
int dvs_ctx_device_info(dvs_ctx *ctx, char *name, size_t name_len, int *n_cu,
                        uint64_t *hbm_bytes);

/* ---- k-mer count matrix ------------------------------------------------- *
 * replaces SeqRecord::to_kcounts / to_kmerseq (src/record.rs:124-141),
 * count_kmers (:41-84), count_monomers (:31-39), entropy (:86-106) and
 * LazySeq.get_kcounts / get_kfreqs (:247-262).
 *
 * Builds, on the device, row r = the k-mer histogram of sequence r (uint32),
 * plus per-row total (number of valid k-mers) and Shannon entropy (bits) of
 * the row's frequency vector.
 *
 * Where the sequences of a build come from: the counterpart, on the build side, of dvs_source below.  A plain value
 * the caller fills per call; the library keeps no pointer to it once the call has returned.  `offsets` is always a
 * HOST array of nseq + 1 entries (DVS_SEQ_BATCH: the batch's own, both fields ignored).  Who waits, and how long a
 * buffer must live: a build from DVS_SEQ_HOST copies the bytes to HBM (four-state sequences of 32 MiB and more cross
 * PCIe packed, 3/8 of the bytes) and returns when its kernels have finished, the caller's buffer free again.  A
 * matrix build from a source that is in HBM already -- DEVICE, PACKED, BATCH -- does NOT wait for its kernels: they
 * are ordered on the ctx stream in front of everything that uses the matrix, and the first call that needs host-side
 * data of it (a selection's seeds, dvs_matrix_get_*, dvs_ctx_sync) waits for them -- so a DEVICE buffer must stay
 * valid, and unmodified, until then, and a dvs_packed or dvs_seqbatch must outlive them (their destroy functions
 * drain the streams such a build was enqueued on).  DVS_BUILD_WAIT=1 in the environment restores a build that
 * returns only when its kernels have finished.  A DEVICE pointer must be 16-byte aligned for dvs_matrix_build;
 * dvs_sketches_build takes any.  PACKED, and a BATCH after dvs_seqbatch_pack, hold four-state sequences:
 * DVS_ERR_VALUE for another num_states; they are sketched with k <= 32.  Every build checks its source before
 * anything else: DVS_ERR_VALUE for a NULL source, handle (unless the batch has no bases) or offsets, or an unknown
 * kind. */
#define DVS_SEQ_HOST 0   /* handle: const uint8_t *, host, one byte per base */
#define DVS_SEQ_DEVICE 1 /* handle: const uint8_t *, device */
#define DVS_SEQ_PACKED 2 /* handle: const dvs_packed * */
#define DVS_SEQ_BATCH 3  /* handle: const dvs_seqbatch * (offsets, nseq: its own) */
typedef struct dvs_seqs {
    uint32_t kind;
    const void *handle;
    const uint64_t *offsets;
    uint32_t nseq;
} dvs_seqs;
int dvs_matrix_build(dvs_ctx *ctx, const dvs_seqs *seqs, uint32_t k, uint32_t num_states, dvs_matrix **out);
/* rows are frequency vectors (the members of SummedRecordsResult objects being
 * merged: get_kmerseqs_and_init_summed_records, src/records.rs:344-360).
 * DVS_ERR_VALUE if a row fails the reference's sum-to-one check
 * (src/record.rs:99-104). */
int dvs_matrix_from_freqs(dvs_ctx *ctx, const double *freqs, uint32_t nrows,
                          uint64_t nbins, dvs_matrix **out);
/* the same for rows already in HBM (the all-gathered winners of a chunked multi-GPU run);
 * d_meta may be NULL, else d_meta[2 r + 1] == 0 marks input row r as padding.  Rows are copied, no
 * host round trip; with d_meta the real rows come first in their input order and the padding
 * rows behind them (skipped like sequences without valid k-mers), so that the first n stream
 * positions are the first n real records of the concatenated results, as
 * get_kmerseqs_and_init_summed_records takes them (src/records.rs:344-360);
 * dvs_matrix_get_source_rows gives the input row of every matrix row. */
int dvs_matrix_from_device_freqs(dvs_ctx *ctx, const double *d_freqs, const double *d_meta,
                                 uint32_t nrows, uint64_t nbins, dvs_matrix **out);
int dvs_matrix_get_source_rows(dvs_ctx *ctx, const dvs_matrix *m, uint32_t *out); /* [nrows] */
void dvs_matrix_destroy(dvs_matrix *m);
uint32_t dvs_matrix_nrows(const dvs_matrix *m);
uint64_t dvs_matrix_nbins(const dvs_matrix *m);
/* device pointers (for zero-copy hand-off to the host framework) */
/* counts [nrows x nbins], or NULL for a frequency matrix.  The elements are uint32, or uint16 when
 * every sequence of the build was at most 32768 k-mer windows long and there are at most 4096 bins
 * (no count can reach 2^16; the build's write and the scan's read move half the bytes): dvs_matrix_count_bytes says which (4, 2;
 * 0 for a frequency matrix).  DVS_COUNTS_U32=1 in the environment keeps every build at uint32. */
const void *dvs_matrix_dev_counts(const dvs_matrix *m);
uint32_t dvs_matrix_count_bytes(const dvs_matrix *m);
const void *dvs_matrix_dev_totals(const dvs_matrix *m);  /* uint32 [nrows] */
const void *dvs_matrix_dev_entropy(const dvs_matrix *m); /* double [nrows] */
/* copies to host: counts rows [row0, row0+nrows), widened to uint32 whatever the device width */
int dvs_matrix_get_counts(dvs_ctx *ctx, const dvs_matrix *m, uint32_t row0,
                          uint32_t nrows, uint32_t *out);
int dvs_matrix_get_totals(dvs_ctx *ctx, const dvs_matrix *m, uint32_t *out);
int dvs_matrix_get_entropy(dvs_ctx *ctx, const dvs_matrix *m, double *out);
/* host one-shot: counts for a batch of host sequences (LazySeq.get_kcounts) */
int dvs_kmer_counts(dvs_ctx *ctx, const uint8_t *seqs, const uint64_t *offsets,
                    uint32_t nseq, uint32_t k, uint32_t num_states,
                    uint32_t *counts_out, uint32_t *totals_out, double *entropy_out);

/* ---- canonical k-mer count rows (strand-independent selection and distances) ---------------------- *
 * A sequence and its reverse complement have different count rows, so every count-based operation tells the two
 * strands apart.  Folding a k-mer's bin with its reverse complement's removes that.  (No counterpart in the reference:
 * its only canonical form is the mash sketch's, src/distance.rs:17-19,65-87.)  Four states only, in the project's
 * alphabet order T0 C1 A2 G3 (RNA: U C A G):
 *   complement      of a digit d is d ^ 2: (base + 2) % 4 of src/distance.rs:18
 *   rc(idx)         of a k-mer index (first base most significant, src/record.rs:18-29): its k base-4 digits
 *                   reversed, each complemented
 *   representative  min(idx, rc(idx)): the lexicographic choice hash_kmer makes (src/distance.rs:65-87)
 *   canonical bins  the representatives in ascending order, C(k) of them: 4^k / 2 for odd k, (4^k + 4^(k/2)) / 2 for
 *                   even k (2, 10, 32, 136, 512, 2 080, 8 192, 32 896 for k = 1 .. 8)
 *   folded row      out[c] = in[rep_c] + in[rc(rep_c)]; for a palindrome (rc(rep_c) == rep_c, even k only) in[rep_c]
 *                   alone.  The total is the source row's; the entropy is the Shannon entropy (bits) of out / total,
 *                   0.0 for a row of total 0, which stays an all-zero row
 * dvs_canonical_bins (host only, no context): *n_out = C(k) and, unless reps_out is NULL, reps_out[C(k)] the
 * representatives.  DVS_ERR_VALUE: k outside 1 .. 16, both outputs NULL.
 * dvs_matrix_fold_canonical makes a new count matrix of m's rows x C(k) bins with m's element width (16-bit rows stay
 * 16-bit: a folded count is at most the row's total), k and num_states, flagged canonical (dvs_matrix_is_canonical).  It is
 * a count matrix like any other for every selection, accessor and jsd / euclidean entry; m is left as it is.  The fold
 * is enqueued on the context's stream behind m's build -- the call waits for that build if it is still in flight -- and
 * returns when the folded rows are written.
 *   DVS_ERR_VALUE, before any device work: a NULL argument; a frequency matrix (it has no k); num_states != 4; a matrix
 *                  that is already canonical
 *   DVS_ERR_NOMEM: the folded matrix does not fit
 * A matrix without rows gives an empty folded matrix. */
int dvs_canonical_bins(uint32_t k, uint32_t *reps_out, uint64_t *n_out);
int dvs_matrix_fold_canonical(dvs_ctx *ctx, const dvs_matrix *m, dvs_matrix **out);
uint32_t dvs_matrix_is_canonical(const dvs_matrix *m);

/* ---- packed sequences ------------------------------------------------------ *
 * Four-state sequences at 3 bits per base instead of the reference's one byte per base
 * (src/record.rs:205-209, diverse_seq/util.py:32-45): the form the histogram (count_kmers,
 * src/record.rs:41-84) and sketch (get_kmer_hashes, src/distance.rs:101-134) kernels read from HBM
 * as it is.  Two planes over the CONCATENATED buffer -- positions, and therefore a batch's offsets,
 * are the same as in the byte form:
 *   codes: one uint32 per 16 bases; base 16 w + i in bits (31 - 2 i)..(30 - 2 i), value = index & 3
 *          (the first base of a k-mer is its most significant digit, src/record.rs:18-29)
 *   mask:  one uint16 per 16 bases; bit 15 - i set when base 16 w + i is >= 4 (gap / ambiguity /
 *          behind the end): every window holding such a base is skipped (src/record.rs:47-64)
 * dvs_pack_sequences packs nbases symbols -- a HOST buffer (host threads pack 4 Mi-base chunks beside
 * their copies: 3/8 of the bytes cross PCIe; returns when the buffer may be reused) or a 16-byte-aligned
 * DEVICE buffer (one kernel on the ctx stream, not waited for: keep the buffer until the next sync).
 * Symbols of an alphabet with more than four states cannot be packed: use the byte form. */
typedef struct dvs_packed dvs_packed;
int dvs_pack_sequences(dvs_ctx *ctx, const uint8_t *seqs, int seqs_on_device, uint64_t nbases,
                       dvs_packed **out);
void dvs_packed_destroy(dvs_packed *p);
int dvs_packed_info(const dvs_packed *p, uint64_t *nbases, uint64_t *nwords); /* nwords = ceil(nbases / 16) */
const void *dvs_packed_dev_codes(const dvs_packed *p); /* uint32 [nwords] in HBM */
const void *dvs_packed_dev_mask(const dvs_packed *p);  /* uint16 [nwords] in HBM */
int dvs_packed_get(dvs_ctx *ctx, const dvs_packed *p, uint32_t *codes_out, uint16_t *mask_out);

/* ---- ingest -------------------------------------- *
 * FASTA file bytes -> the data convention above, on the device: replaces, for the hot path's
 * input, the host-side parse + encode of diverse_seq/io.py:75-104 (dvs_load_seqs.main: records
 * parsed, their sequences joined with "-") and diverse_seq/util.py:32-45 (str2arr:
 * alphabet.to_indices).  `raw` is the file as it is (host pointer, or device pointer when
 * raw_on_device != 0); lut256 maps a file byte to its alphabet index (NULL: the cogent3 "dna"
 * table, dvs_default_alphabet_lut).  join_records != 0: one sequence per file, a gap symbol
 * between adjacent records (io.py:100); 0: one sequence per record.  The encoded bases stay in HBM
 * and feed dvs_matrix_build (a DVS_SEQ_BATCH source) directly. */
typedef struct dvs_seqbatch dvs_seqbatch;
void dvs_default_alphabet_lut(int rna, uint8_t lut[256]);
int dvs_seqbatch_from_fasta(dvs_ctx *ctx, const uint8_t *raw, int raw_on_device, uint64_t nbytes,
                            const uint8_t *lut256, int join_records, dvs_seqbatch **out);
void dvs_seqbatch_destroy(dvs_seqbatch *b);
/* nseq sequences (1 when joined), total encoded symbols, records ('>' lines) in the file */
int dvs_seqbatch_info(const dvs_seqbatch *b, uint32_t *nseq, uint64_t *total_bases, uint32_t *nrecords);
int dvs_seqbatch_offsets(const dvs_seqbatch *b, uint64_t *offsets_out);        /* nseq + 1 */
int dvs_seqbatch_header_positions(const dvs_seqbatch *b, uint64_t *pos_out);   /* nrecords: offset of each '>' */
const void *dvs_seqbatch_dev_codes(const dvs_seqbatch *b);                     /* uint8 [total] in HBM */
int dvs_seqbatch_get_codes(dvs_ctx *ctx, const dvs_seqbatch *b, uint8_t *codes_out);
/* The batch's encoded bases re-stated in the packed form above and the byte form released: a genome
 * collection then sits in HBM at 3/8 of the bytes, and dvs_matrix_build / dvs_sketches_build over the batch
 * (num_states 4) read the packed words.  dvs_seqbatch_dev_codes returns
 * NULL afterwards, dvs_seqbatch_get_codes unpacks (invalid symbols come back as 255), and
 * dvs_seqbatch_packed hands out the planes (NULL before).  DVS_ERR_VALUE for a batch that was encoded
 * with a caller's alphabet table instead of the library's DNA / RNA one (its symbols >= 4 are states, not
 * "invalid"). */
int dvs_seqbatch_pack(dvs_ctx *ctx, dvs_seqbatch *b);
const dvs_packed *dvs_seqbatch_packed(const dvs_seqbatch *b);

/* ---- greedy delta-JSD selection ------------------------------------------ *
 * replaces SummedRecords (src/records.rs:10-216), get_lowest_record_index
 * (:220-252) and the selectors select_nmost_divergent (:311-342),
 * select_nmost_divergent_final (:363-382), select_max_divergent (:390-454),
 * select_max_divergent_final (:456-507), make_summed_records (:509-524), i.e.
 * the bodies of _dvs.nmost_divergent / final_nmost / max_divergent /
 * final_max / get_delta_jsd_calculator (src/lib.rs:59-171).
 *
 * The candidate stream is `npos` positions; position p refers to matrix row
 * order[p] (order == NULL: row p) and carries identity label labels[p]
 * (labels == NULL: label = row index; equal labels == equal seqid, which the
 * reference ignores when already in the set, src/records.rs:71-73,87-89).
 * The first `n_seed` positions seed the set (rows without valid k-mers are
 * skipped, src/records.rs:299-306); the rest are streamed in order. */
#define DVS_MODE_NMOST 0 /* fixed size: replace_lowest on every JSD increase */
#define DVS_MODE_MAX 1   /* grow to max_size while std/cov of delta-JSD rises */
#define DVS_MODE_SET 2   /* build the set from all positions, stream nothing */
#define DVS_STAT_STDEV 0
#define DVS_STAT_COV 1

typedef struct dvs_select_params {
    uint32_t mode;     /* DVS_MODE_* */
    uint32_t n_seed;   /* n (nmost) or min_size (max); ignored for MODE_SET */
    uint32_t max_size; /* MODE_MAX only (already capped to npos by the caller or not) */
    uint32_t stat;     /* DVS_STAT_*, MODE_MAX only */
    uint32_t window;   /* rows scored per scan launch; 0 = library default */
    uint32_t flags;    /* DVS_SELECT_* */
} dvs_select_params;
#define DVS_SELECT_NO_ARBITER 1u /* fail with DVS_ERR_UNSUPPORTED instead of host tie arbitration */
#define DVS_SELECT_STEPWISE 2u   /* dvs_select_run builds the initial set and returns; the caller drives
                                    dvs_select_step_* (row-sharded multi-GPU runs, see below) */
#define DVS_ROW_REMOTE 0xFFFFFFFFu /* order[p]: the row of stream position p lives on another rank */

typedef struct dvs_select_summary {
    uint32_t size;
    uint32_t lowest_index;
    double total_jsd, mean_delta_jsd, std_delta_jsd, cov_delta_jsd, summed_entropies;
    /* engine statistics */
    uint64_t rows_scored;    /* candidate rows read by the scan kernel (re-scans included) */
    uint64_t rows_rechecked; /* rows the scan re-evaluated in full f64 */
    uint32_t n_windows, n_events, n_accepts, n_arbitrated;
    double scan_ms;          /* sum of scan-kernel durations (HIP events) when timing is on, else 0 */
    uint64_t scan_launches;  /* scan-kernel launches the events bracket (no-op launches included) */
    uint32_t engine;         /* 0: one scan launch per window + state kernels; 1: persistent single launch */
    uint32_t rows_coarse_passed; /* persistent engine: rows its all-f32 tier could not decide (scored again by the f32-log tier) */
    /* the LAST scan launch on its own (a selection that starts with a head phase has two very different launches:
     * the event-dense head of the stream on the head CUs, then the full grid): its duration when timing is on, and the
     * rows it scored; the launches in front of it are scan_ms - scan_ms_last and rows_scored - rows_scored_last */
    double scan_ms_last;
    uint64_t rows_scored_last;
    double arbiter_ms;       /* host time spent in tie arbitration (n_arbitrated calls), wall clock */
} dvs_select_summary;

int dvs_select_run(dvs_ctx *ctx, const dvs_matrix *m, const uint32_t *order,
                   const uint32_t *labels, uint64_t npos,
                   const dvs_select_params *params, dvs_select **out);
void dvs_select_destroy(dvs_select *s);
int dvs_select_get_summary(dvs_ctx *ctx, const dvs_select *s, dvs_select_summary *out);
/* members in set order (SummedRecords::get_raw_kseqs, src/records.rs:175-180):
 * stream position, label, delta_jsd, entropy and (if freqs != NULL) the
 * size x nbins frequency rows.  Any output pointer may be NULL. */
int dvs_select_get_members(dvs_ctx *ctx, const dvs_select *s, uint64_t *positions,
                           uint32_t *labels, double *delta_jsd, double *entropy,
                           double *freqs);
/* the same members into caller-provided DEVICE buffers, enqueued on the ctx stream:
 * d_rows[cap_rows x nbins] frequency rows, d_meta[cap_rows x 2] = (stream position, 1.0);
 * rows beyond the set's size are zeroed with meta (0, 0). */
int dvs_select_gather_members(dvs_ctx *ctx, const dvs_select *s, double *d_rows, double *d_meta,
                              uint32_t cap_rows);
/* SummedRecords::delta_jsd (src/records.rs:70-84) for every row of `queries`
 * against the set: 0.0 when qlabels[i] is a member's label, NaN for a row
 * without valid k-mers (the python layer raises, src/records_py.rs:111-120). */
int dvs_select_delta_jsd(dvs_ctx *ctx, const dvs_select *s, const dvs_matrix *queries,
                         const uint32_t *qlabels, double *out);
/* ---- stepwise driving: rows sharded over ranks, set state replicated -------- *
 * The exact multi-GPU form of select_nmost_divergent / select_max_divergent: every
 * rank holds the rows of its share of the stream (order[p] = DVS_ROW_REMOTE for the others; the
 * first n_seed rows replicated everywhere) and an identical copy of the set.  ONE collective per
 * greedy step, everything enqueued on the ctx stream with no host sync:
 *   dvs_select_step_pack   scan this rank's rows of the current window and pack its first local
 *                          event into d_slot[nbins + 2]: position (as a double; < 0: none), the
 *                          row's entropy, the candidate's frequency row
 *   [host framework: all_gather of the slots -- RCCL; world x (nbins + 2) doubles, 8 x 32 KB at k=6]
 *   dvs_select_step_apply  the earliest event among the gathered slots d_all[world][nbins + 2] is the
 *                          step's event (a position is scored by one rank only): resolve +
 *                          leave-one-out + finalize with that candidate, identical arithmetic on
 *                          every rank so the replicas stay bit-identical
 * dvs_select_step_poll syncs and returns the status (0 running, 1 done) / cursor; it must be called at least every 16
 * steps (it also drains the device-side ring of accepted rows, once that is half full, into the host-side log the
 * arbiter replays from, so that log has no cap: dvs_select_step_apply returns DVS_ERR_VALUE when more steps than half
 * the ring holds -- 16 at least -- have passed since the last poll).  When the engine has
 * stopped at a decision inside the rounding band (src/records.rs:86-92,231,246-249) the poll runs the host
 * tie arbiter -- on every rank alike: same seeds, same row log of accepted candidates, same pending
 * candidate, hence the same verdict with no exchange -- and re-enters the step kernels; steps enqueued in
 * between were no-ops.  (DVS_SELECT_NO_ARBITER turns that into an error.) */
int dvs_select_step_pack(dvs_ctx *ctx, dvs_select *s, double *d_slot);
int dvs_select_step_apply(dvs_ctx *ctx, dvs_select *s, const double *d_all, uint32_t world);
int dvs_select_step_poll(dvs_ctx *ctx, dvs_select *s, uint32_t *status, uint64_t *cursor);
/* A look at the status that neither syncs nor drains the queue: *status is the engine's status behind the apply launch
 * `lag` launches before the last one enqueued (0 running while there is none that far back), read from a history the step
 * kernel keeps in pinned host memory.  Every rank sees the same word for the same launch, so a driver that peeks at the same
 * step counts on every rank takes the same decisions (the number of collectives must not depend on timing).  When *status
 * is not 0, or *must_poll is set (half the accepted rows' ring would fill before the next look), call dvs_select_step_poll.
 * DVS_ERR_UNSUPPORTED: this selection keeps no history (not the fast step): poll instead.  (No counterpart in the reference:
 * its greedy loop is one thread, src/records.rs:311-342.) */
int dvs_select_step_peek(dvs_ctx *ctx, dvs_select *s, uint32_t lag, uint32_t *status, int *must_poll);

/* when on, every scan launch is bracketed by a pair of HIP events recorded on the
 * ctx stream (no extra host sync); they are read once the selection has finished
 * and summed into dvs_select_summary.scan_ms / scan_launches */
int dvs_ctx_set_timing(dvs_ctx *ctx, int on);
/* The library's environment switches (DVS_*: measurement aids and escape hatches) are
 * read once, when a context is created; nothing on a per-call path looks at the environment.  This
 * re-reads them for an existing context (tests and A/B measurements that flip a switch in between). */
int dvs_ctx_refresh_knobs(dvs_ctx *ctx);
/* test aid: what the context's memory gates have seen.  out[0]: requests for a device block or a pinned host block
 * since the switches were last read (dvs_ctx_create, dvs_ctx_refresh_knobs), served or not; out[1]: device blocks
 * handed out and not yet given back; out[2]: their bytes; out[3]: 4 KiB pinned blocks handed out and not yet given
 * back.  Host only.  (An addition to ABI 5.) */
int dvs_ctx_block_stats(const dvs_ctx *ctx, uint64_t out[4]);
/* measurement aid: average duration of ONE scan_kernel launch over every streamed row of
 * the selection's stream against its current state, with an unreachable threshold (no
 * events, state untouched): the steady-state streaming rate of the scan arithmetic */
int dvs_select_bench_scan(dvs_ctx *ctx, const dvs_select *s, int repeats, double *ms_out,
                          uint64_t *rows_out);
/* diagnostic: max |v_log_f32(m) - log2(m)| over every f32 m in [0.5, 1), the
 * hardware term of the scan kernel's fast-tier error bound (select.hip FAST_BAND) */
int dvs_selftest_fast_log2(dvs_ctx *ctx, double *max_abs_err);
/* diagnostic: max |log2_acc(x) - log2(x)| / max(1, |log2 x|) of the f64 log2 the precise
 * evaluations use (select_dev.h), over 2^17 mantissas x 80 binades */
int dvs_selftest_log2_acc(dvs_ctx *ctx, double *max_rel_err);
/* diagnostic: the hardware term of the persistent engine's coarse (f32) tier: max over every
 * f32 y in [2^-101, 2) of |v_log_f32(y) - log2 y| in units of 2^-23 max(1, |log2 y|) */
int dvs_selftest_log2_f32(dvs_ctx *ctx, double *max_ulps);
/* diagnostic: count / total by the fma sequence the selection kernels use in place of the f64
 * division (select_dev.h exact_div_u32) against the division itself: every count <= total <=
 * 8192 and 2^32 random pairs; reports the number of mismatches (must be 0) */
int dvs_selftest_exact_div(dvs_ctx *ctx, uint64_t *mismatches);
/* The persistent engine's hand-over words on their own (csrc/persist.hip): `rounds` synthetic windows
 * -- arrival records, hints, listed candidates, the gathering block's release, a use of the never-cleared
 * leave-one-out accumulators -- with contributions every workgroup can recompute and pseudo-random pauses in front of
 * every step; one workgroup per CU.  *failures = workgroup-rounds in which a word read was not the word it must be
 * (+ 2^32 when a bounded spin ran out). */
int dvs_selftest_handover(dvs_ctx *ctx, uint32_t rounds, uint64_t *failures);

/* ---- mash ----------------------------------------------------------------- *
 * dvs_mash_sketch replaces _dvs.mash_sketch (src/distance.rs:136-182) for a
 * batch: sketches_out is nseq x sketch_size (ascending, first lens_out[i]
 * entries valid).  dvs_mash_distances (sketch i at sketches + i * sketch_stride;
 * sketch_size is the value the distance formula uses) replaces diverse_seq/distance.py
 * mash_distance (:230-291) over the pairs (i, j<i) for i = row_start,
 * row_start+row_stride, ... (compute_mash_chunk_distances,
 * diverse_seq/cluster.py:640-644); dist is nseq x nseq row-major, only the
 * visited lower-triangle cells (and their mirror when symmetric != 0) are
 * written.  DVS_ERR_ZERODIV when a visited pair has two empty sketches. */
int dvs_mash_sketch(dvs_ctx *ctx, const uint8_t *seqs, int seqs_on_device,
                    const uint64_t *offsets, uint32_t nseq, uint32_t k,
                    uint32_t sketch_size, uint32_t num_states, int mash_canonical,
                    uint32_t *sketches_out, uint32_t *lens_out);
int dvs_mash_distances(dvs_ctx *ctx, const uint32_t *sketches, uint32_t sketch_stride,
                       const uint32_t *lens, uint32_t nseq, uint32_t k, uint32_t sketch_size,
                       uint32_t row_start, uint32_t row_stride, int symmetric,
                       double *dist);
/* The two stages of ctree (diverse_seq/cluster.py:241-297: sketches, then the N x N distances) with
 * the sketches left in HBM between them: dvs_sketches_build = dvs_mash_sketch without the copy to
 * the host, dvs_sketches_distances = dvs_mash_distances on that handle, dvs_sketches_get copies
 * sketches (may be NULL) and lengths out (what _dvs.mash_sketch returns).  dvs_sketches_build takes its sequences
 * as dvs_matrix_build does (dvs_seqs, above) and returns with its sketches written, whatever the source. */
typedef struct dvs_sketches dvs_sketches;
int dvs_sketches_build(dvs_ctx *ctx, const dvs_seqs *seqs, uint32_t k, uint32_t sketch_size, uint32_t num_states,
                       int mash_canonical, dvs_sketches **out);
void dvs_sketches_destroy(dvs_sketches *sk);
int dvs_sketches_get(dvs_ctx *ctx, const dvs_sketches *sk, uint32_t *sketches_out, uint32_t *lens_out);
const void *dvs_sketches_dev(const dvs_sketches *sk);      /* uint32 [nseq x sketch_size] in HBM */
const void *dvs_sketches_dev_lens(const dvs_sketches *sk); /* uint32 [nseq] */
int dvs_sketches_distances(dvs_ctx *ctx, const dvs_sketches *sk, uint32_t k, uint32_t sketch_size,
                           uint32_t row_start, uint32_t row_stride, int symmetric, double *dist);
/* The distance stage of the sharded ctree (`dvs_par_ctree`, diverse_seq/cluster.py:607-644: worker g takes rows g,
 * g + G, ... of the lower triangle of ALL sketches) with everything left in HBM: a rank's own sketches are copied
 * into its send buffer (dvs_sketches_copy_to_device: rows dst_stride words apart), the gathered N sketches are
 * wrapped without a copy (dvs_sketches_from_device: the caller's buffers, which must outlive the handle) and the
 * strided rows are written into a device matrix (dvs_sketches_distances_device: enqueued on the context's stream and
 * not waited for; *d_zerodiv is set where dvs_sketches_distances would return DVS_ERR_ZERODIV). */
int dvs_sketches_from_device(dvs_ctx *ctx, const uint32_t *d_sketches, const uint32_t *d_lens, uint32_t nseq,
                             uint32_t stride, dvs_sketches **out);
int dvs_sketches_copy_to_device(dvs_ctx *ctx, const dvs_sketches *sk, uint32_t *d_dst, uint32_t dst_stride,
                                uint32_t *d_dst_lens);
int dvs_sketches_distances_device(dvs_ctx *ctx, const dvs_sketches *sk, uint32_t k, uint32_t sketch_size,
                                  uint32_t row_start, uint32_t row_stride, int symmetric, double *d_dist,
                                  uint32_t *d_zerodiv);

/* ---- where an operation's distances come from ------------------------------------------------------ *
 * Every operation below over "the distances of a collection" has ONE entry, which takes a dvs_source: the mode and
 * what the mode keeps in HBM, or a caller's own matrix.  A source is a plain value the caller fills per call; the
 * library keeps no pointer to it (or to `rows`) once the call has returned.
 *   DVS_SRC_MASH       handle: a dvs_sketches; k and sketch_size as dvs_sketches_distances takes them
 *   DVS_SRC_EUCLIDEAN  handle: a dvs_matrix (count rows of either width, or frequency rows)
 *   DVS_SRC_JSD        handle: a dvs_matrix likewise
 *   DVS_SRC_GIVEN      handle: the caller's n x n matrix, row-major float64; a HOST array, or with on_device != 0
 *                      DEVICE memory on the context's device.  Only read, except by the two trees (dvs_linkage, dvs_nj),
 *                      whose working buffer a device matrix is: they OVERWRITE it
 * rows (host, optional; NULL: rows 0 .. n - 1 of the handle) and n say which rows of the handle take part, in which
 * order; position i of a result is rows[i].
 * Every entry checks its source or sources before anything else, DVS_ERR_VALUE for each of: a NULL source or handle
 * (a GIVEN matrix of order 0 may be NULL); an unknown kind; a row list with DVS_SRC_GIVEN; two sides of different
 * kinds; two MASH sides whose k or sketch_size differ.  A combination an operation does not serve is
 * DVS_ERR_UNSUPPORTED with a message that names the operation and the kind; each operation lists its own below. */
enum { DVS_SRC_MASH = 0, DVS_SRC_EUCLIDEAN = 1, DVS_SRC_JSD = 2, DVS_SRC_GIVEN = 3 };
typedef struct dvs_source {
    uint32_t kind;           /* DVS_SRC_* */
    void *handle;            /* dvs_sketches* | dvs_matrix* | the n x n float64 matrix */
    const uint32_t *rows;    /* optional host row list; NULL for DVS_SRC_GIVEN */
    uint32_t n;              /* rows taken (GIVEN: the matrix's order) */
    uint32_t k, sketch_size; /* MASH only */
    int on_device;           /* GIVEN only */
} dvs_source;
/* The whole symmetric n x n matrix of a source into the host array dist.  MASH: exactly
 * dvs_sketches_distances(sk, k, sketch_size, 0, 1, 1, dist) (mash_distances, diverse_seq/distance.py:119-175).
 * EUCLIDEAN: ||f_i - f_j||_2 over the rows of the matrix (euclidean_distances, diverse_seq/distance.py:294-336).  JSD:
 * "pairwise Jensen-Shannon divergence" below.  n == 0 writes nothing, n == 1 a zero.  DVS_ERR_UNSUPPORTED: a GIVEN
 * source (the matrix is the caller's already); a row list, or n other than the handle's rows; (EUCLIDEAN, JSD) more
 * than 524 280 rows, the row limit of the square entries.  DVS_ERR_ZERODIV: (MASH) as dvs_sketches_distances. */
int dvs_distances(dvs_ctx *ctx, const dvs_source *src, double *dist);

/* ---- linkage trees (the tree stage of ctree) ----------------------------------------------------- *
 * dvs_linkage is scipy.cluster.hierarchy.linkage(X[triu_indices(n, 1)], method) on the device over the n x n distances
 * of a source; with DVS_LINKAGE_AVERAGE it replaces the clustering of make_cluster_tree (diverse_seq/cluster.py:216-230:
 * sklearn AgglomerativeClustering(metric="precomputed", linkage="average")).  The n - 1 merges of scipy's linkage
 * matrix Z bit for bit, row j = (pairs[2 j], pairs[2 j + 1], heights[j], sizes[j]), cluster ids n, n + 1, ... in merge
 * order.  Only D[i][j] with i < j counts (the diagonal and the lower triangle are checked, not used).  Returns when
 * the host outputs are written.  `method` is scipy's _LINKAGE_METHODS code:
 *   DVS_LINKAGE_SINGLE    restates scipy's _hierarchy.mst_single_linkage (Prim's minimum spanning tree)
 *   DVS_LINKAGE_COMPLETE, DVS_LINKAGE_AVERAGE, DVS_LINKAGE_WEIGHTED, DVS_LINKAGE_WARD
 *                         restate scipy's _hierarchy.nn_chain (nearest-neighbour chain) with the updates
 *                         of _hierarchy_distance_update.pxi
 * and both end in scipy's stable sort by height and `label` relabelling.
 * The sources: MASH, EUCLIDEAN and JSD are ctree end to end with the N x N matrix left in HBM (it never crosses PCIe):
 * the cells of dvs_distances for the source, written into the context's scratch, then the tree.  A GIVEN host matrix is
 * uploaded into the context's scratch and left as it is; a GIVEN device matrix is the working buffer and is
 * OVERWRITTEN.
 *   DVS_ERR_UNSUPPORTED: 3 (centroid) and 4 (median), which scipy builds by _hierarchy.fast_linkage (not built here); a
 *                  row list, or n other than the handle's rows
 *   DVS_ERR_VALUE: any other method code; n < 2; a NaN or +-inf entry anywhere (sklearn's check_array; a row without
 *                  valid k-mers gives NaN euclidean and jsd distances); for ward, a negative entry above the diagonal
 *                  (scipy's heights would be NaN); a device matrix on another device
 *   DVS_ERR_ZERODIV: (MASH) as dvs_sketches_distances, when two sketches are empty
 *   DVS_ERR_NOMEM: the matrix does not fit in HBM
 * The checks come in one order for every source: the method, n < 2, the source's own, the device, the fit in HBM. */
#define DVS_LINKAGE_SINGLE 0
#define DVS_LINKAGE_COMPLETE 1
#define DVS_LINKAGE_AVERAGE 2
#define DVS_LINKAGE_WARD 5
#define DVS_LINKAGE_WEIGHTED 6
int dvs_linkage(dvs_ctx *ctx, const dvs_source *src, int method, uint32_t *pairs, double *heights, uint32_t *sizes);

/* ---- pairwise Jensen-Shannon divergence: the cells of a DVS_SRC_JSD source ------------------------ *
 * D[i][j] = H((f_i + f_j) / 2) - (H(f_i) + H(f_j)) / 2 over the rows of the matrix, f = counts / total, H in bits: the
 * total_jsd of the two-member set SummedRecords::new([i, j]) (src/records.rs:27-68), the measure of paper/paper.md
 * Table 1 (identical sequences 0.0, no k-mer in common 1.0); the divergence, not its square root.  Full symmetric
 * nrows x nrows float64 matrix, every cell in [0, 1], exactly 0 on the diagonal and between rows of equal
 * counts; a row without a valid k-mer has NaN off the diagonal.  This is what a DVS_SRC_JSD source means to every
 * operation: dvs_distances writes this matrix, dvs_linkage and dvs_nj build their trees over the same bits left in HBM. */

/* ---- distances between two collections, and the k nearest references ------------------------------ *
 * The rectangular counterpart of the N x N entries above: cell (i, j) of an nq x nr float64 matrix is the distance
 * between row q->rows[i] of source q and row r->rows[j] of source r (a NULL list: rows 0 .. n - 1 of its handle).
 * (No counterpart in the reference: its distance functions fill the square matrix of one collection,
 * diverse_seq/distance.py:119-175, 294-336.)  The two handles may be one and the same, so "every row against the
 * selected rows of the same matrix" copies nothing; for the JSD and EUCLIDEAN kinds they may differ in element
 * type (16-bit counts, 32-bit counts, frequency rows, in any combination) but not in nbins.  A cell is the same bits
 * as the cell dvs_distances writes for the same two rows of a source of that kind (JSD: in [0, 1], exactly 0
 * between rows of equal counts, NaN where either row has no valid k-mer -- a rectangular matrix has no diagonal, so
 * also for such a row against itself; MASH: with the sources' k and sketch_size).
 * The matrix is computed in strips of query rows whose device buffer is bounded (256 MiB, one tile row of 32 queries
 * at least; DVS_CROSS_STRIP_ROWS overrides the strip height), so nq is not limited by a grid dimension; dist is the
 * host array, nq x nr row-major.  Return when the host outputs are written.
 *   DVS_OK with nothing written: nq == 0 or nr == 0
 *   DVS_ERR_VALUE: a row index beyond its handle (or, with a NULL list, nq / nr beyond its rows), handles of
 *                  different contexts or devices, unequal nbins
 *   DVS_ERR_UNSUPPORTED: nr beyond the row limit of the square entries; GIVEN sources (the matrix is the caller's)
 *   DVS_ERR_ZERODIV: (MASH) k == 0, or a visited pair has two empty sketches */
int dvs_cross_distances(dvs_ctx *ctx, const dvs_source *q, const dvs_source *r, double *dist);
/* The kk nearest references of every query over those cells, the matrix never leaving the device: idx and dist are
 * host arrays nq x kk; row i lists the kk smallest cells of matrix row i in ascending order of (distance, position
 * in the reference list 0 .. nr - 1 -- not the matrix row): a tie goes to the lower position, so the result is unique
 * and the same on every run and for every strip height.  NaN cells are never listed; a row with fewer than kk other
 * cells ends in slots of position 0xFFFFFFFF and distance NaN.  (No counterpart in the reference.)  Errors as above, and
 *   DVS_ERR_VALUE: kk == 0 or kk > nr (hence always for nr == 0)
 *   DVS_ERR_UNSUPPORTED: kk > 64 (a full ranking takes the matrix) */
int dvs_nearest(dvs_ctx *ctx, const dvs_source *q, const dvs_source *r, uint32_t kk, uint32_t *idx, double *dist);

/* ---- flat clusters of a tree: the cut, and the scores of a labelling ------------------------------- *
 * dvs_linkage_cut turns dvs_linkage's outputs (pairs[2 (n - 1)], heights[n - 1], as they are) into flat clusters on
 * the host (no device work; ctx only takes the error text and may be NULL):
 *   DVS_CUT_HEIGHT, value t     every merge j with heights[j] <= t is applied: the partition of scipy's
 *                               fcluster(Z, t, "distance")
 *   DVS_CUT_NCLUSTERS, value K  the first m = max(n - K, 0) merges, and every following merge of the same height as
 *                               merge m - 1 (a cut never separates merges of equal height, so fewer than K clusters
 *                               may come back): the partition of scipy's fcluster(Z, K, "maxclust")
 * labels_out[n]: the cluster of every leaf, in [0, *n_clusters_out), numbered by first appearance in leaf order (leaf
 * 0 is in cluster 0): scipy's partition, not its label numbers.  (No counterpart in the reference.)
 *   DVS_ERR_VALUE: n < 2, K < 1 or not an integer value, NaN t, any other criterion, heights that are not
 *                  non-decreasing (the five methods built here are monotone; a foreign Z may not be), a pair that
 *                  names a cluster not yet made or already merged */
#define DVS_CUT_HEIGHT 0
#define DVS_CUT_NCLUSTERS 1
int dvs_linkage_cut(dvs_ctx *ctx, uint32_t n, const uint32_t *pairs, const double *heights, int criterion, double value,
                    uint32_t *labels_out, uint32_t *n_clusters_out);
/* The scores of a labelling of the n rows of a source over their n x n distances D, computed strip by strip as the
 * cross entries above compute them (queries = references = the source; the same cells bit for bit), the matrix never
 * existing whole.  labels[n] in [0, n_clusters); a label nobody carries is an empty cluster
 * and is skipped.  With n_c the size of cluster c, for every row i of cluster l:
 *   within[i]      sum of D(i, j) over the other members j of l.  Cell (i, i) is never read into a sum, whatever it holds
 *   a[i]           within[i] / (n_l - 1); 0 when i is alone in l
 *   b[i], neighbour[i]  the least mean distance S(i, c) / n_c to the members of another non-empty cluster c, and that c;
 *                  a tie goes to the lower c, a NaN mean is never taken; nothing to take: NaN and 0xFFFFFFFF
 *   silhouette[i]  0 when i is alone in l (sklearn's rule) or a == b == 0, else (b - a) / max(a, b); NaN where a or b is
 *   medoids[c]     the member of c with the least within, a tie to the lowest row, NaN never taken; 0xFFFFFFFF for a
 *                  cluster without such a member (empty, or every member's within NaN)
 * The order in which the terms of a sum are added depends on (n, labels) alone: the same bits on every run and for
 * every strip height (DVS_CROSS_STRIP_ROWS).  All outputs are host arrays ([n]; medoids [n_clusters]); any may be NULL
 * except within.  Return when they are written.  (No counterpart in the reference.)
 * A GIVEN matrix is only read, rows [q0, q0 + mq) at a time.
 *   DVS_OK with nothing written: n == 0
 *   DVS_ERR_VALUE: a label >= n_clusters (hence n_clusters == 0 with n > 0), a row index beyond the handle, a device
 *                  mismatch, a matrix that is not device memory where it is said to be
 *   DVS_ERR_UNSUPPORTED: n beyond the row limit of the square entries
 *   DVS_ERR_ZERODIV: (MASH) as dvs_cross_distances over the same rows on both sides: the strips hold every
 *                  cell, a row against itself included, so one empty sketch among the rows is enough */
int dvs_cluster_scores(dvs_ctx *ctx, const dvs_source *src, const uint32_t *labels, uint32_t n_clusters, double *within,
                       double *a, double *b, uint32_t *neighbour, double *silhouette, uint32_t *medoids);

/* ---- neighbours within a radius, and threshold clusters ------------------------------------------- *
 * The sparse product of the cross entries above: for every query, the references whose cell is <= radius, the nq x nr
 * matrix never existing whole and never leaving the device -- only the listed pairs come back.  (No counterpart in
 * the reference.)  A cell is the bits dvs_distances gives the same two rows, computed strip by strip as
 * dvs_cross_distances computes it (same sources, strip bound and DVS_CROSS_STRIP_ROWS).  The result is a
 * dvs_pairs: a CSR list on the host, row_start[nq + 1] (row_start[0] == 0, row_start[nq] == the number of pairs) and,
 * for query i, col / dist [row_start[i], row_start[i + 1]): col is the position in the reference list 0 .. nr - 1 --
 * not the matrix row --, dist that cell.  Within a query the entries are in ascending position.  radius is inclusive
 * (a cell equal to it is listed); a NaN cell compares false and is never listed; -inf or any negative radius gives
 * empty lists, +inf lists every non-NaN cell.  The same pairs in the same order on every run and for every strip
 * height: no position depends on an atomic.  flags: DVS_WITHIN_SKIP_SELF drops cell (i, i), whatever it holds -- it is
 * never read -- for a call whose two sides list the same positions (i against position i of the reference list).
 * max_pairs (0: no limit): as soon as the pairs of the strips so far exceed it the call stops and fails; the context
 * stays usable.  A dvs_pairs lives on the host and holds no reference to the context: it may outlive it, and is freed
 * by dvs_pairs_destroy (NULL is fine).  A GIVEN q is the caller's n x n matrix against itself, only read as
 * dvs_cluster_scores reads it: r is then NULL or the same matrix (any other: DVS_ERR_UNSUPPORTED).  *out is NULL after
 * an error.  Errors of the arguments, all before any device work:
 *   DVS_OK with an empty list (nq rows, no pairs): nq == 0 or nr == 0 -- as for dvs_cross_distances, nothing else
 *                  about the handles and the row lists is looked at then, so a bad row list passes unnoticed
 *   DVS_ERR_VALUE: NULL arguments, NaN radius, unknown flag bits (checked first); a row index beyond its handle, handles of different
 *                  contexts or devices, unequal nbins, a matrix that is not device memory where it is said to be
 *   DVS_ERR_UNSUPPORTED: nr (n) beyond the row limit of the square entries
 *   DVS_ERR_ZERODIV: (MASH) k == 0
 * and those that show while the strips are walked:
 *   DVS_ERR_UNSUPPORTED: more than max_pairs pairs (the message names both numbers)
 *   DVS_ERR_NOMEM: the host lists do not fit
 *   DVS_ERR_ZERODIV: (MASH) a visited pair has two empty sketches: exactly where dvs_cross_distances raises it */
typedef struct dvs_pairs dvs_pairs;
#define DVS_WITHIN_SKIP_SELF 1u /* drop cell (i, i): both sides list the same positions */
int dvs_within(dvs_ctx *ctx, const dvs_source *q, const dvs_source *r, double radius, uint32_t flags, uint64_t max_pairs,
               dvs_pairs **out);
void dvs_pairs_destroy(dvs_pairs *p);
int dvs_pairs_info(const dvs_pairs *p, uint32_t *n_rows, uint64_t *n_pairs); /* either may be NULL */
/* row_start[n_rows + 1], col[n_pairs], dist[n_pairs]: host arrays, any may be NULL */
int dvs_pairs_get(const dvs_pairs *p, uint64_t *row_start, uint32_t *col, double *dist);
/* Threshold clusters: the connected components of the graph that joins positions i and j when D(i, j) <= radius, over
 * the n x n distances of a source (queries = references = its rows), computed strip by strip as above.  They are the
 * flat clusters of the single-linkage tree cut at height radius -- dvs_linkage_cut with DVS_CUT_HEIGHT over
 * dvs_linkage's DVS_LINKAGE_SINGLE tree -- without the n x n matrix and without the tree.  Only the cells above the
 * diagonal (j > i) are read: a GIVEN matrix need not be symmetric, and its diagonal may hold anything.  A strip's edges go through a union-find on the host and are dropped before the next strip's arrive.
 * labels[n]: the cluster of every position, in [0, *n_clusters), numbered by first appearance in position order
 * (position 0 is in cluster 0), as dvs_linkage_cut numbers them.  A position whose every cell is NaN or beyond the
 * radius is a cluster of its own; a negative radius joins nothing.  (No counterpart in the reference.)
 *   DVS_OK with nothing written: n == 0.  n == 1: label 0, one cluster
 *   DVS_ERR_VALUE, DVS_ERR_UNSUPPORTED, DVS_ERR_NOMEM: as above
 *   DVS_ERR_ZERODIV: (MASH) exactly as dvs_cluster_scores */
int dvs_threshold_clusters(dvs_ctx *ctx, const dvs_source *src, double radius, uint32_t *labels, uint32_t *n_clusters);

/* ---- minimum spanning tree: single linkage without the matrix -------------------------------------- *
 * The minimum spanning tree of the n x n distances of a source (queries = references = its rows), computed strip by
 * strip as above: the n x n matrix never exists, the device holds one strip and O(n) beside it.  Edges are ordered by
 * (weight, lower position, higher position); under that order the tree is unique -- the one Kruskal's algorithm
 * builds when it visits the upper triangle in that order -- and so are the outputs, on every run and for every strip
 * height.  It is built by Boruvka rounds: in a round every position finds, on the device, its nearest position of
 * another component (a tie to the lower position), every component takes the least of its positions' finds, and the
 * picks are merged on the host; a round is one pass over all n x n cells, and there are ceil(log2 n) rounds at most.
 * A NaN cell is no edge: where NaN cells disconnect the positions the result is a spanning FOREST.
 * core (host, n, or NULL): with it the weight of cell (i, j) is max(D(i, j), core[i], core[j]), the mutual-reachability
 * distance of HDBSCAN / robust single linkage, and the tree is the minimum spanning tree of those weights.
 * edges[2 (n - 1)], weights[n - 1]: edge e joins positions edges[2 e] < edges[2 e + 1] at weights[e]; the edges come in
 * ascending (weight, lower, higher).  *n_edges = n - the number of components: n - 1 for a tree; the slots behind are
 * left as they were.  *n_rounds (may be NULL): the passes over the strips that were made.  The sorted weights are the
 * heights of dvs_linkage's DVS_LINKAGE_SINGLE tree, bit for bit.
 * A GIVEN matrix, host or device, is only read, rows [q0, q0 + mq) at a time, the diagonal included (position i is in
 * its own component: the cell is never taken).  It must be symmetric, which is not checked: for an asymmetric matrix
 * some spanning tree (forest) of the graph of its non-NaN cells is returned, and nothing more is promised.
 * (No counterpart in the reference.)  Errors, all before any device work:
 *   DVS_OK with nothing written: n == 0.  n == 1: no edge, no round
 *   DVS_ERR_VALUE: a NULL output; a core entry that is NaN, infinite or negative (the message names the position); a
 *                  row index beyond the handle, a device mismatch, a matrix that is not device memory where it is
 *                  said to be
 *   DVS_ERR_UNSUPPORTED: n beyond the row limit of the square entries
 *   DVS_ERR_NOMEM: the host arrays of the merge do not fit
 * and DVS_ERR_ZERODIV: (MASH) exactly as dvs_cluster_scores.
 * dvs_linkage_from_mst turns the n - 1 edges of a spanning tree, in ascending weight, into the outputs of dvs_linkage
 * for the single-linkage tree (pairs, heights, sizes: scipy's ids, merge j makes cluster n + j, the lower id first), on
 * the host (no device work; ctx only takes the error text and may be NULL).  Where no two weights are equal that is
 * scipy's linkage(..., "single") bit for bit; among equal weights the merges follow the order of the edges.
 *   DVS_ERR_VALUE: a NULL argument, n < 2, a weight that is NaN or below the one before it, an edge that closes a
 *                  cycle, an end that is no position -- a forest has fewer than n - 1 edges and no tree: a caller
 *                  who passes one fills the slots behind *n_edges with 0xFFFFFFFF and gets this error */
int dvs_mst(dvs_ctx *ctx, const dvs_source *src, const double *core, uint32_t *edges, double *weights, uint32_t *n_edges,
            uint32_t *n_rounds);
int dvs_linkage_from_mst(dvs_ctx *ctx, uint32_t n, const uint32_t *edges, const double *weights, uint32_t *pairs,
                         double *heights, uint32_t *sizes);

/* ---- cophenetic distances of a tree, and their correlation with the distances it was built from ---- *
 * scipy.cluster.hierarchy.cophenet.  The cophenetic distance coph(i, j) of two leaves is the height of the merge at
 * which they first share a cluster.  Over dvs_linkage's outputs (pairs[2 (n - 1)], heights[n - 1], scipy's ids: leaves
 * 0 .. n - 1, merge j makes n + j) it is found without a search for the lowest common ancestor: the in-order walk of
 * the tree (left child, merge, right child) lists the leaves in dendrogram order, order[n], and the merges between
 * them, gap[n - 1] -- gap[p] is the merge that joins the subtree ending at position p to the one starting at p + 1;
 * every merge owns exactly one gap, and a parent's index is above its children's, so with pos the inverse of order and
 * pos[i] < pos[j]
 *     coph(i, j) = heights[max(gap[pos[i] .. pos[j] - 1])]
 * an integer range maximum and a lookup: exact, and valid for any well-formed tree -- the heights need not be
 * monotone (scipy's centroid and median trees are not), unlike dvs_linkage_cut.
 * dvs_linkage_cophenet is scipy's cophenet(Z) as the square matrix (squareform of its result, bit for bit): coph is a
 * host array n x n, zero on the diagonal; host only, ctx only takes the error text and may be NULL.
 * dvs_cophenet is scipy's cophenet(Z, Y)[0], Pearson's r between D(i, j) and coph(i, j) over the n (n - 1) ordered
 * pairs i != j, with the n x n distances D of a source computed strip by strip as for the cluster scores above (queries =
 * references = the source; leaf i of the tree is rows[i]); the matrix never exists whole.  Cell (i, i) is never read.
 * Both variables are shifted by c_bar, the mean of all cophenetic distances (known from the tree alone: a merge of
 * clusters of sizes s_a and s_b at height h holds s_a s_b pairs at h), which leaves r as it is and keeps the moments
 * free of cancellation where the distances crowd near one value.  With x = D(i, j) - c_bar and y = coph(i, j) - c_bar:
 *   row_sums  [5][n], optional: per row i the sums over j != i of x, y, x x, y y and x y.  The order in which a sum's
 *             terms are added depends on (n, the tree) alone: the same bits on every run and for every strip height
 *   *corr     r = Sxy / sqrt(Sxx Syy) from the 5 n sums in long double on the host (Sxy = sum xy - sum x sum y / M, M =
 *             n (n - 1), likewise Sxx, Syy); NaN when either variance is zero (n = 2, a constant matrix), as scipy
 *             gives -- zero meaning not above the rounding error of its own terms, 2 (n + 8) 2^-52 sum xx
 *   coph      n x n host array, optional: the cophenetic rows the kernel used, copied out strip by strip (N^2
 *             doubles over PCIe: ask for it only when it is wanted)
 * A GIVEN matrix is only read, as dvs_cluster_scores reads it.
 *   DVS_OK with nothing written: n == 0
 *   DVS_ERR_VALUE: n == 1, a pair that names a cluster not yet made or already merged, a row index beyond the handle,
 *                  a device mismatch, a matrix that is not device memory where it is said to be
 *   DVS_ERR_UNSUPPORTED: n beyond the row limit of the square entries
 *   DVS_ERR_ZERODIV: (MASH) one empty sketch among the rows, as dvs_cluster_scores
 * All argument checks come before any device work.  (No counterpart in the reference.) */
int dvs_linkage_cophenet(dvs_ctx *ctx, uint32_t n, const uint32_t *pairs, const double *heights, double *coph);
int dvs_cophenet(dvs_ctx *ctx, const dvs_source *src, const uint32_t *pairs, const double *heights, double *corr,
                 double *row_sums, double *coph);

/* ---- neighbour-joining tree (the tree of additive distances) ------------------------------------- *
 * Canonical Saitou-Nei / Studier-Keppler neighbour joining of an n x n distance matrix, n >= 3, on the device.  As for
 * the linkage trees only the upper triangle counts (the diagonal counts as 0) and every entry is checked.  Unlike a
 * linkage tree the result is unrooted, assumes no molecular clock and carries branch lengths; on additive distances it
 * is the tree that generated them.  The algorithm (f64, no fma, real divisions), with slots 0 .. n - 1, leaf i in slot
 * i as node i, r active slots and R[s] the sum of D[s][t] over the other active t:
 *   while r > 3: the least Q(i, j) = double(r - 2) * D[i][j] - R[i] - R[j] over active i < j, equal values to the
 *     lowest (i, j) in lexicographic slot order; record t joins node[i] and node[j] with the lengths
 *     li = D[i][j] / 2 + (R[i] - R[j]) / (2 * double(r - 2)) and lj = D[i][j] - li; the new node n + t takes slot i,
 *     slot j is retired; for every other active k: du = (D[i][k] + D[j][k] - D[i][j]) / 2,
 *     R[k] = R[k] - D[i][k] - D[j][k] + du, D[i][k] = D[k][i] = du; R[i] is summed afresh;
 *   at r = 3 (slots x < y < z) the last record joins the three nodes with (Dxy + Dxz - Dyz) / 2,
 *     (Dxy + Dyz - Dxz) / 2 and (Dxz + Dyz - Dxy) / 2.
 * The row sums may be added in any order, so the records are defined bit for bit only where the arithmetic is exact;
 * elsewhere two results are compared as unrooted trees (their splits and lengths).
 *   joins    uint32 [3 (n - 2)]: record t = (joins[3 t], joins[3 t + 1], joins[3 t + 2]), node ids (leaves 0 .. n - 1,
 *            record t makes n + t); the third child is 0xFFFFFFFF except in the last record
 *   lengths  double [3 (n - 2)]: the branch above each child (0.0 in an unused third slot); a negative length is
 *            neighbour joining's answer on distances that are not additive and is returned as it is
 * The sources as for dvs_linkage: a GIVEN host matrix is copied to the device and left unchanged, a GIVEN device matrix
 * is the working buffer and is OVERWRITTEN; MASH, EUCLIDEAN and JSD compute their distances into the context's scratch
 * and build the tree there: the matrix never leaves HBM.
 *   DVS_ERR_VALUE: n < 3, a NaN or +-inf entry anywhere, a device matrix on another device (and a row without a valid
 *                  k-mer, EUCLIDEAN and JSD: NaN distances); DVS_ERR_ZERODIV: (MASH) two empty sketches;
 *                  DVS_ERR_NOMEM: the matrix and the tree's scratch (a quarter of the matrix) do not fit;
 *                  DVS_ERR_UNSUPPORTED: a row list, or n other than the handle's rows
 * dvs_nj_patristic (host only, ctx may be NULL): out, n x n, the path length between every two leaves of such a tree;
 * O(n^2).  DVS_ERR_VALUE: n < 3, a record that names a node not yet made or already joined, a third child outside
 * the last record.  (No counterpart in the reference.) */
int dvs_nj(dvs_ctx *ctx, const dvs_source *src, uint32_t *joins, double *lengths);
int dvs_nj_patristic(dvs_ctx *ctx, uint32_t n, const uint32_t *joins, const double *lengths, double *out);

/* ---- farthest-first selection (max-min diversity, Gonzalez' greedy for k-center) ------------------- *
 * Representatives by distance: from one or more seeds on, the item whose distance to the nearest item already taken
 * is largest, until n_select items are taken or every item lies within min_distance of one.  A pick costs one row of
 * distances; the n x n matrix of a mode never exists.  (No counterpart in the reference.)  The algorithm:
 *   items and distances  items 0 .. n - 1; d(p, j) is the source's cell for rows p and j (the bits dvs_distances
 *       writes for a source of that kind), on a GIVEN matrix dist[p * n + j]: a row is read as it stands, the
 *       diagonal never
 *   state per item  mind[j], +inf at first; owner[j], the position in the pick list of the nearest pick, NONE
 *       (0xFFFFFFFF) at first; a flag `taken`; a flag `out`
 *   take(p, r)  p is appended to the picks with radius r; mind[p] = 0, owner[p] = its own position; for every other j
 *       that is neither taken nor out, with c = d(p, j): if c is NaN, j goes out for good (mind[j] = NaN, owner[j] =
 *       NONE; never picked); else if c < mind[j] (strict: a tie stays with the earlier pick) mind[j] = c and owner[j] =
 *       p's position
 *   seeds   one or more distinct rows, taken in the given order with radius NaN
 *   picking while fewer than n_select picks exist: the candidate is the j, neither taken nor out, of the largest
 *       mind[j], equal values to the lowest j; no candidate: stop; use_min_distance and not mind[j] > min_distance:
 *       stop (a row exactly at min_distance counts as covered); else take(j, mind[j])
 *   result  picks[*n_picked] in pick order, the seeds first; radius[*n_picked]; owner[n] and dist_to_owner[n] (the
 *       final mind); *cover, the largest mind over the items neither taken nor out, 0.0 when there are none
 * A seed that is NaN against everything puts every other row out and the picks are the seeds: no special case.  An item
 * at +inf from every pick keeps owner NONE and is the next candidate.  Everything is a comparison or a copy of a cell,
 * so the result is exact and the same on every run and for every batch length (DVS_MAXMIN_BATCH: the steps enqueued
 * between two reads of the device's status word, 64 by default).
 * MASH, EUCLIDEAN and JSD sources take rows 0 .. n - 1 of their handle (n <= its rows; a row list:
 * DVS_ERR_UNSUPPORTED).  A GIVEN host matrix is uploaded whole and left unchanged, a GIVEN device matrix only read.  picks and radius hold n_select entries, owner and dist_to_owner n; all are host
 * arrays.  Return when they are written.
 *   DVS_ERR_VALUE, before any device work: no seed, a seed >= n, a repeated seed, n_select < n_seeds or > n, NaN
 *                  min_distance (with use_min_distance), n beyond the handle's rows; a device mismatch
 *   DVS_ERR_ZERODIV: (MASH) k == 0, or a pair the traversal visits -- (p, j) with p a pick and j neither taken nor
 *                  out at that point -- has two empty sketches, exactly where dvs_sketches_distances divides by zero
 *                  for the same pair.  A pick's own cell is not a pair: one empty sketch among the rows does not raise
 *   DVS_ERR_UNSUPPORTED: (EUCLIDEAN) n beyond 524 280, the grid of the distance kernel
 * The row limit of the square entries does not apply otherwise: nothing here is n x n but a caller's matrix. */
int dvs_maxmin(dvs_ctx *ctx, const dvs_source *src, const uint32_t *seeds, uint32_t n_seeds, uint32_t n_select,
               int use_min_distance, double min_distance, uint32_t *picks, double *radius, uint32_t *n_picked,
               uint32_t *owner, double *dist_to_owner, double *cover);

/* ---- principal coordinates (PCoA, classical MDS), with projection of further rows ----------------- *
 * The ordination of a collection's distances: coordinates in a few dimensions whose Euclidean distances approximate
 * the given ones.  (No counterpart in the reference.)  The matrix is D, n x n: the entries of a MASH, EUCLIDEAN or JSD
 * source or of a caller's GIVEN matrix as they are, no square root taken; the diagonal counts as 0 and is never read.
 *   A = -1/2 D o D               the element-wise square times -1/2
 *   B = J A J, J = I - 11^T / n  Gower's double centring
 *   mu_i = (1/n) sum_j d_ij^2    the row means of the squared distances
 *   trace(B) = (1/2n) sum_ij d_ij^2   the total inertia, known from mu alone, without any eigenvalue
 * The result is the n_axes algebraically largest eigenpairs (lambda_a, v_a) of B, ||v_a||_2 = 1 and v_a orthogonal to
 * 1, in descending lambda; the sign of v_a is fixed so that its component of largest magnitude (the lowest index on a
 * tie) is positive.  Coordinates: X[i, a] = v_a[i] sqrt(lambda_a) for lambda_a > 0, else 0; proportion:
 * lambda_a / trace(B).  A JSD or mash matrix is not Euclidean: B then has negative eigenvalues, which are never among
 * the returned axes unless n_axes reaches into them.
 * B is never formed: the iteration keeps every vector orthogonal to 1, so B x = A x - mean(A x) 1, and the kernel
 * squares the cells as it reads them.  The n x n matrix is only READ, a GIVEN device matrix as well as the scratch a
 * mode wrote -- unlike the two trees, which overwrite their working buffer.  The solver is a block Krylov iteration
 * (blocks of 16 columns, start vectors from a counter-based hash of (row, column)) with full orthogonalisation and
 * Rayleigh-Ritz on the host; it stops when the n_axes leading Ritz pairs all have residual <= tol * lambda_1, or when
 * the basis holds max_basis columns (0: min(n - 1, 512); never more than n - 1, at which it spans the whole
 * complement of 1 and the pairs are exact).
 *   values[n_axes], vectors[n x n_axes] row-major, row_means[n] (mu)
 *   residuals[n_axes]   the true ||B v_a - lambda_a v_a||_2 of the vectors returned
 *   info: trace; converged, the number of axes with residual <= tol * lambda_1; basis, the columns of the basis at the
 *         end; steps, the passes over the matrix; products, the matrix-vector products they held
 * A call that runs out of basis returns DVS_OK with what it has: info->converged < n_axes.  A spectrum without gaps is a
 * property of the data, not an error of the call.  Every sum is added in an order that n and the block shape fix: the
 * same bits on every run, and for a GIVEN host matrix and the same matrix in device memory.
 * The sources as for dvs_nj: whole, no row list; MASH, EUCLIDEAN and JSD write their matrix into the context's scratch,
 * where it stays; a GIVEN host matrix is uploaded, a GIVEN device matrix read where it is.  The checks come in this
 * order, all before any device work: the arguments, n, the source's own, the device, the fit in HBM.
 *   DVS_ERR_VALUE: n < 2; n_axes == 0 or n_axes > n - 1; tol < 0 or NaN; max_basis < n_axes when not 0; a device
 *                  matrix on another device; and, found by the pass in front of the first step, a NaN or +-inf entry
 *                  off the diagonal (the text the trees give) or D[i][j] and D[j][i] that differ in a bit
 *   DVS_ERR_UNSUPPORTED: n_axes > 64; max_basis > 4096; a row list, or n other than the handle's rows
 *   DVS_ERR_ZERODIV: (MASH) as dvs_nj
 *   DVS_ERR_NOMEM: the matrix, the basis with B times the basis beside it (2 n max_basis doubles) and the small blocks
 *                  do not fit in HBM
 * dvs_pcoa_project (Gower 1968) gives further rows their coordinates in a fitted ordination: for a query with distances
 * delta_j to the n fitted rows
 *   x_a = -1/2 v_a^T (delta o delta - mu) / sqrt(lambda_a)    for lambda_a > 0, else 0
 * which needs only (values, vectors, row_means) of the fit because v_a is orthogonal to 1; a fitted row projected
 * against its own collection gets its own coordinates back.  q and r as dvs_cross_distances takes them, row lists on
 * both sides included; r's n rows are the fitted rows in the fit's order.  The cells are computed in the same strips
 * (the same bound, the same DVS_CROSS_STRIP_ROWS) and never leave the device: only coords, nq x n_axes row-major, comes
 * back, the same bits for every strip height.  A NaN cell (a row without valid k-mers) makes that query's coordinates
 * NaN.
 *   DVS_ERR_VALUE: r->n == 0, n_axes == 0, a NULL table; DVS_ERR_UNSUPPORTED: n_axes > 64, GIVEN sources; everything
 *                  else as dvs_cross_distances */
typedef struct dvs_pcoa_params {
    uint32_t n_axes, max_basis;
    double tol;
} dvs_pcoa_params;
typedef struct dvs_pcoa_info {
    double trace;
    uint32_t converged, basis, steps;
    uint64_t products;
} dvs_pcoa_info;
int dvs_pcoa(dvs_ctx *ctx, const dvs_source *src, const dvs_pcoa_params *params, double *values, double *vectors,
             double *residuals, double *row_means, dvs_pcoa_info *info);
int dvs_pcoa_project(dvs_ctx *ctx, const dvs_source *q, const dvs_source *r, uint32_t n_axes, const double *values,
                     const double *vectors, const double *row_means, double *coords);

/* ---- k-medoids (PAM): the k items that lie closest, in total, to everything else ------------------- *
 * Representatives that minimise the total distance TD = sum_o d(o, nearest medoid), with the partition they make.  (No
 * counterpart in the reference.)  Items are 0 .. n - 1, D is the n x n matrix of the source: the distance between a
 * medoid or candidate x and an item o is D[x][o] -- a row is read as it stands, so the matrix need not be symmetric;
 * the diagonal counts as 0 and is never read.  Every off-diagonal entry must be finite and >= 0 (DVS_ERR_VALUE; for NaN
 * or +-inf with the text the trees give), so a row without valid k-mers raises as it does for dvs_nj.
 *   state    med[0 .. k), distinct items; slot order is part of the result.  Per item o: near[o], the slot of its
 *       nearest medoid, equal distances to the lowest slot; dn[o], that distance; ds[o], the least distance to a medoid
 *       in any OTHER slot, +inf when k = 1.  A medoid, taken as an item, has near = its own slot and dn = 0 whatever the
 *       other medoids' distances; its ds is the least distance over the other slots.  near, dn and ds are comparisons
 *       and copies of cells, hence exact.  td = sum_o dn[o].
 *   init     DVS_KMEDOIDS_INIT_GIVEN: the caller's k distinct items in their order.  DVS_KMEDOIDS_INIT_BUILD, PAM's
 *       BUILD: slot 0 takes the x with the least sum_{o != x} D[x][o], ties to the lowest x; each following slot takes
 *       the non-medoid x with the largest gain sum_o max(dn[o] - D[x][o], 0), the term for o = x being dn[x], ties to
 *       the lowest x -- a gain of 0 everywhere still takes the lowest non-medoid.
 *   swap     steepest-descent PAM SWAP with FastPAM1's shared evaluation (Schubert & Rousseeuw 2021), at most
 *       max_swaps rounds.  A round scores every non-medoid x with d = D[x][o], d = 0 for o = x.  For k >= 2:
 *         R[l]     = sum_{near[o] = l} (ds[o] - dn[o])     the loss of removing slot l, once per round
 *         shared_x = sum_o min(d - dn[o], 0)
 *         C_x[l]   = sum_{near[o] = l} c(o),  c(o) = dn[o] - ds[o] if d < dn[o], else d - ds[o] if d < ds[o], else 0
 *         Delta_x[l] = (R[l] + C_x[l]) + shared_x
 *       for k = 1: Delta_x[0] = sum_o (d - dn[o]); no infinity enters a sum.  The round's exchange is the (x, l) of the
 *       least Delta, ties to the lowest x, then to the lowest l.  If that Delta is not < -noise the search has
 *       converged and stops (stop = 1); else med[l] = x, the state is rebuilt from the k medoid rows, td summed afresh
 *       and the exchange recorded.  noise = 4 (n + 8) 2^-52 n d_max, d_max the largest entry off the diagonal (as a
 *       float64 product in that order): what a float64 Delta may be off by -- three sums of <= n terms each <= d_max
 *       and two additions.  A Delta within the noise of 0 lowers td by nothing that can be told from rounding, and
 *       taking it lets the search cycle: a symmetric matrix has exchanges of Delta = 0 by its structure (the two
 *       members of a cluster of two), which evaluate to -1e-17 as easily as to 0.  An accepted Delta is truly < 0, td
 *       truly falls with every exchange, and no set of medoids comes twice.  k == n: no candidate, converged at once (stop = 1, whatever max_swaps).  max_swaps rounds
 *       done, each with an exchange: stop = 0 -- max_swaps == 0 evaluates a set as it is.
 * Each sum (R, C, shared, the gains, the row sums, td) is added in an order that (n, k) and the state fix, without
 * floating-point atomics: the same bits on every run, for every batch length (DVS_KMEDOIDS_BATCH: the rounds enqueued
 * between two reads of the device's status word, 8 by default) and for a host matrix and the same matrix in device
 * memory.
 *   medoids[k]  in (INIT_GIVEN) and out; labels[n] near; dist[n] dn; second[n] ds (optional: NULL)
 *   swaps[2 max_swaps]  (x, slot) per exchange, optional; td[max_swaps + 1]  td after init and after every exchange,
 *       optional; both filled up to info->n_swaps, the rest left as it was
 *   info: td_init, td; n_swaps; stop (0: max_swaps reached, 1: no exchange lowers td); passes, the reads of the whole
 *       matrix: the entry check (which holds slot 0's row sums), one per further BUILD slot, one per scored round
 * The sources as for dvs_pcoa: whole, no row list; MASH, EUCLIDEAN and JSD write their matrix into the context's
 * scratch, where it stays; a GIVEN host matrix is uploaded and left as it is, a GIVEN device matrix only read.  The
 * checks come in dvs_pcoa's order: the arguments, n, the source's own, the device, the fit in HBM; the arguments and n
 * before any device work.
 *   DVS_ERR_VALUE: a NULL argument; k == 0 or k > n; n == 0; an unknown init; non-zero flags; an initial medoid >= n or
 *                  repeated; a non-finite or negative entry off the diagonal
 *   DVS_ERR_UNSUPPORTED: k > 1024 (the per-candidate accumulators live in LDS); max_swaps > 65 535; a row list, or n
 *                  other than the handle's rows
 *   DVS_ERR_ZERODIV: (MASH) as dvs_nj
 *   DVS_ERR_NOMEM: the matrix and the state do not fit in HBM */
#define DVS_KMEDOIDS_INIT_BUILD 0
#define DVS_KMEDOIDS_INIT_GIVEN 1
typedef struct dvs_kmedoids_params {
    uint32_t k, init, max_swaps, flags /* 0 */;
} dvs_kmedoids_params;
typedef struct dvs_kmedoids_info {
    double td_init, td;
    uint32_t n_swaps, stop, passes;
} dvs_kmedoids_info;
int dvs_kmedoids(dvs_ctx *ctx, const dvs_source *src, const dvs_kmedoids_params *params, uint32_t *medoids,
                 uint32_t *labels, double *dist, double *second, uint32_t *swaps, double *td, dvs_kmedoids_info *info);

/* ---- PERMANOVA (Anderson 2001): do the groups explain the distances? -------------------------------- *
 * A pseudo-F statistic from the sums of squared distances within the groups of a labelling, and what the same sum
 * is under permutations of the labels.  (No counterpart in the reference.)  Items are 0 .. n - 1 with labels g[i] in
 * [0, a), a = n_groups, group sizes n_g; D is the n x n matrix of the source.  Only D[i][j] with i < j counts, as in
 * dvs_linkage: the matrix need not be symmetric, and the diagonal and the lower triangle are never read.  Every entry
 * above the diagonal must be finite and >= 0 (DVS_ERR_VALUE; for NaN or +-inf with the text the trees give).
 *   q_ij    = D[i][j] * D[i][j]
 *   SS_T    = (1/n) sum_{i<j} q_ij
 *   SS_W(g) = sum_{i<j, g_i = g_j} q_ij / n_{g_i}
 *   SS_A = SS_T - SS_W;  F = (SS_A / (a - 1)) / (SS_W / (n - a));  R^2 = SS_A / SS_T
 *   p = (1 + #{pi : SS_W(g o pi) <= SS_W(g)}) / (1 + P)
 * SS_T and the group sizes do not change under a permutation and F falls strictly as SS_W rises: the count is taken
 * on SS_W, in float64, and the library returns the sums -- SS_T, SS_W of the observed labels and of every permutation,
 * the observed term of each group -- from which a caller derives F, R^2 and p.  The caller makes the permutations
 * (the library carries no random numbers; permuting inside strata is the caller's choice): perm_labels[p][i] is the
 * label of item i after permutation p.
 * The order of every sum (w[g] = 1.0 / n_g, rounded once; x (+) y: a float64 addition; no fused multiply-add):
 *   a tile is 128 rows x 256 columns of the matrix, tile (rb, cb) holding rows 128 rb .. and columns 256 cb ..;
 *   C_j(tile) = the q_ij of the tile's rows i < j with g_i = g_j, added in ascending i from +0.0 (a cell that does not
 *       match adds +0.0 in its place);
 *   S(tile)  = w[g_j] * C_j(tile) over the tile's columns: each of the four runs of 64 columns by the xor tree (lanes
 *       l and l ^ 32, then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1), the four runs added in ascending order;
 *   SS_W     = S over all tiles (rb * ceil(n / 256) + cb = t): 256 strided chains t = k, k + 256, ... in ascending
 *       order, chain k in lane k & 63 of run k >> 6, the lanes by the same tree, the runs in ascending order.
 *   T_i = sum_{j>i} q_ij and, for the observed labels, R_i = sum_{j>i, g_j = g_i} q_ij: 64 strided chains over the
 *       columns from 64 floor((i + 1) / 64) in ascending order (a column <= i adds +0.0), met by the same tree;
 *   SS_T = (T_0 (+) T_1 (+) ... (+) T_{n-1}) / n;  group_ss[g] = w[g] * (the R_i of the group's items in ascending i).
 * Every order depends on positions and n only, never on the label values, and there is no floating-point atomic.  So
 * the same bits come back on every run, for every batch length (DVS_PERMANOVA_BATCH: the label vectors, the observed
 * one among them, that one pass over the matrix serves: 16 by default, 32 at most), for a host matrix and the same
 * matrix in device memory; and SS_W is a function of the PARTITION and its sizes alone: two label vectors that induce
 * the same partition -- renamed groups, the identity permutation, a permutation that maps every group onto itself --
 * give the same bits, and all of these count towards p.  Two DISTINCT partitions whose sums are equal in exact
 * arithmetic (the quantised distances of mash) may still differ in the last bit.  Each of ss_total, ss_within[p] and
 * group_ss[g] lies within (n + 8) 2^-52 of its exact value, relatively (two levels of sums of at most n terms).
 *   labels[n]  the observed labels; perm_labels[n_perm][n] row-major, NULL exactly when n_perm == 0
 *   ss_total[1]; ss_within[n_perm + 1], [0] the observed labels'; group_ss[n_groups] (optional: NULL), the observed
 *       within-group term of each group: their sum is SS_W(g) up to rounding
 *   info (optional: NULL): n_le, the count in p's numerator (without the 1); passes, the reads of the matrix's upper
 *       triangle: the entry check and one per batch; batch, the batch length used
 * The sources as for dvs_kmedoids: whole, no row list; MASH, EUCLIDEAN and JSD write their matrix into the context's
 * scratch, where it stays; a GIVEN host matrix is uploaded and left as it is, a GIVEN device matrix only read.  The
 * checks come in dvs_kmedoids's order: the arguments, n, the source's own, the device, the fit in HBM; the arguments
 * and n before any device work.
 *   DVS_ERR_VALUE: a NULL labels, ss_total or ss_within; perm_labels NULL with n_perm > 0 or not NULL with n_perm == 0;
 *                  n < 3; n_groups < 2 or >= n; a label >= n_groups; an empty group; a row of perm_labels whose group
 *                  sizes are not the observed ones (the message names the first); a non-finite or negative entry
 *                  above the diagonal; a device matrix on another device
 *   DVS_ERR_UNSUPPORTED: a row list, or n other than the handle's rows; n_groups > 65 535 (a label travels in 8 or 16
 *                  bits)
 *   DVS_ERR_ZERODIV: (MASH) as dvs_nj
 *   DVS_ERR_NOMEM: the matrix and the sums' state do not fit in HBM */
typedef struct dvs_permanova_info {
    uint32_t n_le, passes, batch;
} dvs_permanova_info;
int dvs_permanova(dvs_ctx *ctx, const dvs_source *src, const uint32_t *labels, uint32_t n_groups,
                  const uint32_t *perm_labels, uint32_t n_perm, double *ss_total, double *ss_within, double *group_ss,
                  dvs_permanova_info *info);

/* ---- the Mantel test: do two distance matrices agree? -------------------------------------------------- *
 * The Pearson correlation of the cells of two n x n distance matrices, and what the same correlation is after the
 * items of one of them are permuted.  (No counterpart in the reference.)  Items are 0 .. n - 1, n >= 3, and
 * m = n (n - 1) / 2.  X and Y are the matrices of the two sources, which may be of different kinds.
 * What is read: only the cells above the diagonal, in both: x_ij = X[i][j] for i < j, and y(a, b) = Y[min(a, b)][max(a,
 * b)].  The diagonal and the lower triangle of either matrix are never read.  Every counted cell must be finite and
 * >= 0 (DVS_ERR_VALUE; for NaN or +-inf with the text the trees give, for a negative cell a message that says which
 * matrix).
 * Both variables are shifted, as dvs_cophenet shifts its own, which keeps the moments free of cancellation where
 * the distances crowd near one value (fl: rounded to float64 once; r does not depend on the shifts):
 *   s_x = fl(S_x / m), S_x the sum of the counted cells of X in the order below; s_y likewise
 *   u_ij = fl(x_ij - s_x);  v(a, b) = fl(y(a, b) - s_y)
 *   A = sum u,  B = sum v,  S_uu = sum fl(u * u),  S_vv = sum fl(v * v)            (the same under every permutation)
 *   Z(pi) = sum_{i<j} fl(u_ij * v(pi[i], pi[j]))        pi[i]: the item of Y that stands at position i; Z(id) observed
 *   r(pi) = (Z(pi) - A B / m) / sqrt((S_uu - A^2 / m) (S_vv - B^2 / m)),  NaN when either factor is <= 0 (a constant
 *           matrix)
 * r rises strictly with Z, so every count is taken on Z, in float64:
 *   n_ge = #{pi : Z(pi) >= Z(id)},  n_le = #{pi : Z(pi) <= Z(id)},
 *   n_abs_ge = #{pi : |fl(Z(pi) - c0)| >= |fl(Z(id) - c0)|},  c0 = fl(fl(A * B) / m);   p = (1 + count) / (1 + P)
 * The library returns the sums and the counts; r and p are derived by the caller, who also makes the permutations
 * (the library carries no random numbers).
 * The order of every sum (x (+) y: a float64 addition; every product is rounded before it is added, no fused
 * multiply-add; a chain starts from +0.0):
 *   the row sums of X, Y, u, fl(u * u), v, fl(v * v): row i's cells j > i in 64 strided chains over the columns from
 *       64 floor((i + 1) / 64) in ascending order (a column <= i adds +0.0), chain k in lane k, the lanes met by the xor
 *       tree (lanes l and l ^ 32, then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1);
 *   S_x, S_y, A, B, S_uu, S_vv: the n row sums, row_0 (+) row_1 (+) ... (+) row_{n-1};
 *   zpart(pi, i) = row i's products fl(u_ij * v(pi[i], pi[j])), j > i, in 256 strided chains over the columns from
 *       256 floor((i + 1) / 256) in ascending order, chain k in lane k & 63 of run k >> 6, each run by the same tree,
 *       the four runs added in ascending order; zpart(pi, n - 1) = +0.0;
 *   Z(pi) = the n zpart(pi, i): 256 strided chains i = k, k + 256, ... in ascending order, met as above.
 * Every order is a function of n and of positions only, never of pi or of the values, and there is no floating-point
 * atomic.  So the same bits come back on every run, for every batch length (DVS_MANTEL_BATCH: the permutations, the
 * identity among them, that one scoring pass serves: 32 by default and at most), wherever a permutation sits in its
 * batch, and for a host matrix and the same matrix in device memory.  The identity permutation gives z[0]'s bits and counts towards p.
 * Each of A, B, S_uu, S_vv and Z(pi) lies within band(n) = (n + 8) 2^-52 of its exact value over the u and v,
 * relative to the sum of its terms' magnitudes (two levels of sums of at most n terms); r within 2 band(n) (1 + |r|) of
 * Pearson's r of the original cells.
 *   perms[n_perm][n] row-major, NULL exactly when n_perm == 0;  moments[6]: s_x, s_y, A, B, S_uu, S_vv
 *   z[n_perm + 1], [0] the observed;  info (optional: NULL): the three counts (without the 1); passes, the reads of a
 *       matrix's upper triangle by the longest chain: the entry pass, the centre pass and one per batch; batch, the
 *       batch length used
 * The sources: each whole, no row list, checked against itself; both of the same n.  MASH, EUCLIDEAN and JSD write
 * their matrices into the context's blocks; a GIVEN host matrix is uploaded; a GIVEN device X is only read.  Y is
 * always worked on in a block the library owns -- v is written over both [a][b] and [b][a] -- so a GIVEN device Y is
 * copied first and the caller's matrix stays as it was.  The checks come in this order: the arguments and n (before
 * any device work), x's own, y's own, the device, the pointers, the fit in HBM (asked once for both matrices, Y's copy
 * and the state); the rows of perms are checked batch by batch while the device works on the batch before.
 *   DVS_ERR_VALUE: a NULL argument; perms NULL with n_perm > 0 or not NULL with n_perm == 0; n < 3; x->n != y->n; a
 *                  row of perms that is not a permutation of 0 .. n - 1 (the message names the first); a non-finite
 *                  or negative counted cell; a device matrix on another device
 *   DVS_ERR_UNSUPPORTED: a row list, or n other than the handle's rows
 *   DVS_ERR_ZERODIV: (either MASH source) as dvs_nj
 *   DVS_ERR_NOMEM: the matrices, Y's copy and the state do not fit in HBM */
typedef struct dvs_mantel_info {
    uint32_t n_ge, n_le, n_abs_ge, passes, batch;
} dvs_mantel_info;
int dvs_mantel(dvs_ctx *ctx, const dvs_source *x, const dvs_source *y,
               const uint32_t *perms /* [n_perm][n], NULL exactly when n_perm == 0 */, uint32_t n_perm,
               double moments[6] /* s_x, s_y, A, B, S_uu, S_vv */,
               double *z /* [n_perm + 1], [0] the observed */, dvs_mantel_info *info /* optional */);

#ifdef __cplusplus
}
#endif
#endif /* DVS_HIP_H */
