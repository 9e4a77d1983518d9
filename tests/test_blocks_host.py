"""What a block of device memory holds when an operation receives it, without a GPU: the case table, the error cases
and the schedules that tests/test_gpu_poisoned_blocks.py (every block handed out full of 0xFF bytes:
DVS_TEST_KNOBS=poison_blocks) and tests/test_gpu_mixed_workload.py (one context serving an interleaved workload) run,
pinned here with their preconditions: every case's CPU reference can be computed, every operation that enqueues GPU
work is named by some case, every schedule runs every case at least twice and every error case at least once.

A case is one small call sequence of one operation family on a context it is given.  run(ctx, keep) returns its outputs
as named numpy arrays (results only: no work counters, no timings); check(out) holds them to the family's existing CPU
reference with the comparison the family's own test file uses; ref() computes that reference.  keep: a list that
receives the handles the case made instead of their being closed (the mixed workload closes them later, in another
order)."""
import functools
from typing import Callable, NamedTuple

import numpy as np
import pytest

import oracle
from conftest import pack_reference, synth_seqs
from diverseseq_amd import _lib, cluster, distance, engine
from test_clusters_host import first_appearance, truth_cluster_scores
from test_cophenet_host import truth_correlation
from test_cross_host import expected_nearest
from test_distance_truth_host import EUCLID_RTOL, tol_derived
from test_ingest import GENBANK, _random_fasta
from test_jsd_host import oracle_jsd_matrix
from test_linkage_host import tie_matrices
from test_linkage_methods_host import METHODS, scipy_z
from test_maxmin_host import maxmin_ref, same_bits
from test_nj_host import (dyadic_tree, general_yardstick, length_tolerance, restated, same_tree, split_lengths, tie_case,
                          truth)

POISON = "poison_blocks"   # the word of DVS_TEST_KNOBS
REFUSE = "refuse_block_"   # ... and the one tests/test_gpu_refused_blocks.py walks: refuse_block_<i>
N = 257                    # rows of every square matrix: the N x N x 8-byte block (528 392 -> 528 384 + 4 096 bytes,
                           # rounded to 4 KiB: 532 480) passes between mash, jsd, euclidean, linkage, nj, cophenet, max-min
MASH_RTOL = 1e-13          # a mash cell against the oracle (tests/test_gpu_cross.py, test_gpu_parity.py)
RTOL, TIGHT = 1e-6, 1e-11  # tests/test_gpu_parity.py: selections against the oracle / what the f64 kernels deliver
MASH_TILE = 8192           # windows of a hash-kernel tile (csrc/mash.hip)
Q_ROWS = np.r_[7, np.arange(100, 164)]  # 65 query rows (row 7 of `seqs257` has no valid k-mer) ...
R_ROWS = np.arange(200, 231)            # ... against 31 reference rows, 5 nearest of them
SELECT_SHAPES = ((3000, 400, 3, 10), (2000, 600, 6, 20))  # (nseq, length, k, n) of tests/test_gpu_parity.py


class Case(NamedTuple):
    name: str
    family: str
    ops: tuple          # the operations it runs, as the completeness check names them
    reference: str      # the existing CPU reference it is checked against
    run: Callable       # run(ctx, keep=None) -> {name: ndarray}
    check: Callable     # check(out): against ref()
    ref: Callable       # ref(): the CPU reference (cached)
    env: dict           # environment switches of the case


class ErrorCase(NamedTuple):
    name: str
    family: str
    run: Callable       # run(ctx): raises
    raises: type
    follower: str       # the case that runs right behind it in schedule (c): it asks for blocks of the same sizes
    host: Callable      # host(): the same refusal from the reference's side, or None where it has none
    setup: Callable = lambda ctx: None  # setup(ctx): what run makes before the refused call, made and closed again


FAMILIES = ("distances", "trees", "cophenet_clusters", "maxmin", "sketches", "histograms", "ingest", "selections", "neighbours",
            "ordination", "medoids", "spanning", "groups")


def _done(keep, *handles):
    for h in handles:
        if keep is None:
            h.close()
        else:
            keep.append(h)


def bits(a) -> np.ndarray:
    """an output as the integers of its bits: NaN compares equal to the same NaN"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    return a


def assert_same_outputs(got: dict, want: dict, what=""):
    assert list(got) == list(want), (what, list(got), list(want))
    for key in want:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
        same = bits(g) == bits(w)
        assert same.all(), (what, key, int((~same).sum()), "cells differ; first at", np.argwhere(~same)[0].tolist())


# ------------------------------------------------------------------ inputs (seeded)

@functools.lru_cache(maxsize=None)
def ragged97(states: int = 4) -> tuple:
    """97 ragged sequences of 300-900 symbols: one empty, one shorter than any k, one all-invalid, one an exact copy of
    another, one with invalid symbols at both ends"""
    rng = np.random.default_rng(97 + states)
    seqs = [rng.integers(0, states, size=int(rng.integers(300, 901)), dtype=np.uint8) for _ in range(97)]
    seqs[0] = np.zeros(0, dtype=np.uint8)
    seqs[1] = seqs[1][:1].copy()
    seqs[2] = np.full(400, states, dtype=np.uint8)
    seqs[3] = seqs[4].copy()
    seqs[5][:3] = states
    seqs[5][-3:] = states
    return tuple(seqs)


@functools.lru_cache(maxsize=None)
def ragged97_long() -> tuple:
    """the 97 and one row of 70 001 bases: a tile list, zero_rows_kernel, row_stats_kernel"""
    rng = np.random.default_rng(70_001)
    long_row = rng.integers(0, 4, size=70_001, dtype=np.uint8)
    long_row[rng.integers(0, 70_001, size=40)] = 4
    return ragged97() + (long_row,)


@functools.lru_cache(maxsize=None)
def seqs257(clean: bool = False) -> tuple:
    """257 sequences of 300-900 bases; row 11 a copy of row 5; unless `clean`, row 7 without a valid k-mer"""
    rng = np.random.default_rng(N)
    seqs = [rng.integers(0, 4, size=int(rng.integers(300, 901)), dtype=np.uint8) for _ in range(N)]
    seqs[11] = seqs[5].copy()
    if not clean:
        seqs[7] = np.full(60, 4, dtype=np.uint8)
    return tuple(seqs)


@functools.lru_cache(maxsize=None)
def seqs65(states: int = 4) -> tuple:
    """65 sequences for the sketch builds: one shorter than k (an empty sketch), one longer than two hash tiles, invalid
    symbols, a copy"""
    rng = np.random.default_rng(65 + states)
    seqs = [rng.integers(0, states, size=int(rng.integers(200, 3000)), dtype=np.uint8) for _ in range(65)]
    seqs[0] = seqs[0][:2].copy()
    seqs[1] = rng.integers(0, states, size=2 * MASH_TILE + 777, dtype=np.uint8)
    seqs[1][[MASH_TILE - 1, MASH_TILE + 5]] = states
    seqs[2][rng.random(seqs[2].size) < 0.02] = states
    seqs[9] = seqs[8].copy()
    return tuple(seqs)


@functools.lru_cache(maxsize=None)
def two_empty_sketches() -> tuple:
    """the clean 257 with two sequences shorter than k = 12: 0 / 0 between them"""
    seqs = list(seqs257(True))
    seqs[3], seqs[40] = seqs[3][:5].copy(), seqs[40][:7].copy()
    return tuple(seqs)


@functools.lru_cache(maxsize=None)
def random257() -> np.ndarray:
    d = np.random.default_rng(N).random((N, N))
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def symmetric257() -> np.ndarray:
    u = np.triu(random257(), 1)
    d = u + u.T
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def ties257() -> np.ndarray:
    d = np.random.default_rng(N + 2).integers(0, 4, (N, N)).astype(np.float64)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def ties120() -> np.ndarray:
    return dict(tie_matrices(0))["int120"]


@functools.lru_cache(maxsize=None)
def labels257() -> np.ndarray:
    return np.random.default_rng(6).integers(0, 6, N).astype(np.int64)


@functools.lru_cache(maxsize=None)
def tree257() -> np.ndarray:
    from scipy.cluster.hierarchy import linkage as scipy_linkage

    return scipy_linkage(symmetric257()[np.triu_indices(N, 1)], "average")


@functools.lru_cache(maxsize=None)
def ingest_fasta() -> bytes:
    """about 300 KB: CRLF, two empty records in the middle, blank lines, no trailing newline; more than two 128 KiB scan
    blocks"""
    rng = np.random.default_rng(300)
    head = _random_fasta(rng, 390, crlf=True)
    tail = _random_fasta(rng, 390, crlf=True, trailing_newline=False)
    return head + b">empty one\r\n>empty two\r\n\r\n" + tail


def fasta_of(seqs) -> bytes:
    return "".join(f">s{i} row {i}\n" + "".join("TCAGN"[min(int(c), 4)] for c in q) + "\n" for i, q in enumerate(seqs)).encode()


@functools.lru_cache(maxsize=None)
def select_seqs(shape: int) -> tuple:
    nseq, length, k, _ = SELECT_SHAPES[shape]
    return tuple(synth_seqs(nseq, length, nseq + k, invalid_frac=0.001, ragged=True))


# ------------------------------------------------------------------ references (cached; every one runs on the CPU)

@functools.lru_cache(maxsize=None)
def counts_ref(which: str, k: int, states: int):
    seqs = ragged97_long() if which == "long" else ragged97(states)
    counts = np.stack([oracle.count_kmers(s, states, k) for s in seqs]).astype(np.uint32)
    ent = np.array([oracle.to_kfreqs(s, states, k)[1] if c.sum() else 0.0 for s, c in zip(seqs, counts)])
    return counts, counts.sum(axis=1).astype(np.uint32), ent


@functools.lru_cache(maxsize=None)
def jsd_ref(clean: bool) -> np.ndarray:
    return oracle_jsd_matrix(list(seqs257(clean)), 3, 4)


@functools.lru_cache(maxsize=None)
def euclid_ref(clean: bool) -> np.ndarray:
    c = np.stack([oracle.count_kmers(s, 4, 3) for s in seqs257(clean)]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = c / c.sum(axis=1, keepdims=True)
        return np.sqrt(((f[:, None, :] - f[None, :, :]) ** 2).sum(-1))


@functools.lru_cache(maxsize=None)
def members_ref(clean: bool, from_freqs: bool) -> np.ndarray:
    """the rows nmost(10) keeps of the 257 at k = 3, in member order"""
    seqs = list(seqs257(clean))
    if from_freqs:
        return oracle.final_nmost(np.stack([oracle.to_kfreqs(s, 4, 3)[0] for s in seqs]), 10).members()[0].astype(np.int64)
    return oracle.nmost(seqs, 10, 3, 4).members()[0].astype(np.int64)


def expected_sketch(seq, k, s, states, canonical):
    w = max(len(seq) - k + 1, 1)
    return oracle.mash_sketch(seq, k, min(s, w), states, canonical)  # (no sketch is longer than its windows)


@functools.lru_cache(maxsize=None)
def sketch_ref(which: str, k: int, s: int, states: int, canonical: bool):
    seqs = {"seqs65": lambda: seqs65(states), "clean257": lambda: seqs257(True)}[which]()
    sk = [expected_sketch(q, k, s, states, canonical) for q in seqs]
    return sk, oracle.mash_distances(sk, k, s)


@functools.lru_cache(maxsize=None)
def select_ref(shape: int, what: str):
    nseq, length, k, n = SELECT_SHAPES[shape]
    seqs = list(select_seqs(shape))
    if what == "nmost":
        return oracle.nmost(seqs, n, k, 4)
    if what in ("stdev", "cov"):
        return oracle.max_divergent(seqs, n, 3 * n, k, 4, what)
    if what == "order":
        order = select_order(shape)
        return oracle.nmost([seqs[i] for i in order], n, k, 4, labels=order)
    if what == "resident":
        return oracle.nmost(list(resident_seqs(shape)), n, k, 4)
    raise KeyError(what)


@functools.lru_cache(maxsize=None)
def select_order(shape: int) -> np.ndarray:
    nseq = SELECT_SHAPES[shape][0]
    order = np.random.default_rng(shape).permutation(nseq).astype(np.uint32)
    return np.concatenate([order, order[:40]])  # ids repeated later in the stream


@functools.lru_cache(maxsize=None)
def resident_seqs(shape: int) -> tuple:
    """the shape's sequences with two seed rows that have no valid k-mer (skipped, as records.rs:299-306 does)"""
    seqs = list(select_seqs(shape))
    seqs[0], seqs[3] = seqs[0][:2].copy(), np.full(40, 4, dtype=np.uint8)
    return tuple(seqs)


@functools.lru_cache(maxsize=None)
def query_seqs(shape: int) -> tuple:
    _, length, k, _ = SELECT_SHAPES[shape]
    q = synth_seqs(6, length, 999 + k, ragged=True)
    q[4] = np.full(30, 4, dtype=np.uint8)  # a query without a valid k-mer: NaN
    return tuple(q)


# ------------------------------------------------------------------ the families

def _matrix_out(m, prefix="") -> dict:
    return {prefix + "counts": m.counts(), prefix + "totals": m.totals(), prefix + "entropy": m.entropy(),
            prefix + "count_bytes": np.array([m.count_bytes])}


def _check_matrix_out(out, ref, width, prefix=""):
    counts, totals, ent = ref
    assert out[prefix + "count_bytes"][0] == width
    assert np.array_equal(out[prefix + "counts"], counts), "k-mer counts differ"
    assert np.array_equal(out[prefix + "totals"], totals)
    live = totals > 0
    assert (np.abs(out[prefix + "entropy"][live] - ent[live]) <= TIGHT * np.maximum(1.0, np.abs(ent[live]))).all()


def histogram_cases():
    def counts(name, which, k, states, width, env=None, extra_ops=()):
        seqs = list(ragged97_long() if which == "long" else ragged97(states))

        def run(ctx, keep=None):
            m = ctx.build_matrix(seqs, k, states)
            out = _matrix_out(m)
            _done(keep, m)
            if extra_ops:
                c, t, h = ctx.kmer_counts(seqs[:8], k, states)
                out.update(kc_counts=c, kc_totals=t, kc_entropy=h)
            return out

        def check(out):
            ref = counts_ref(which, k, states)
            _check_matrix_out(out, ref, width)
            if extra_ops:
                assert np.array_equal(out["kc_counts"], ref[0][:8]) and np.array_equal(out["kc_totals"], ref[1][:8])

        return Case(name, "histograms", ("Context.build_matrix", "Context.build_matrix_concat") + tuple(extra_ops),
                    "oracle counts, totals, entropies", run, check, lambda: counts_ref(which, k, states), env or {})

    yield counts("counts_k3_u16", "ragged97", 3, 4, 2, extra_ops=("Context.kmer_counts",))
    yield counts("counts_k3_u32", "ragged97", 3, 4, 4, env={"DVS_COUNTS_U32": "1"})
    yield counts("counts_20states_k2", "ragged97", 2, 20, 2)
    yield counts("counts_k8_global_atomics", "ragged97", 8, 4, 4)
    yield counts("counts_long_row", "long", 3, 4, 4)

    seqs = list(ragged97())

    def run_packed(ctx, keep=None):
        import torch

        data, offs = engine.concat(seqs)
        p = ctx.pack_host(data)
        codes, mask = p.planes()
        m = ctx.build_matrix_packed(p, offs, 3)
        out = dict(codes=codes, mask=mask, **_matrix_out(m))
        t = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to("cuda:0")
        torch.cuda.synchronize()
        pd = ctx.pack_device(t.data_ptr(), data.size)
        out["dev_codes"], out["dev_mask"] = pd.planes()
        ctx.sync()
        _done(keep, m, p, pd)
        return out

    def check_packed(out):
        data, _ = engine.concat(seqs)
        codes, mask = pack_reference(data)
        for pre in ("", "dev_"):
            assert np.array_equal(out[pre + "codes"], codes) and np.array_equal(out[pre + "mask"], mask)
        _check_matrix_out(out, counts_ref("ragged97", 3, 4), 2)

    yield Case("counts_packed", "histograms", ("Context.pack_host", "Context.pack_device", "Context.build_matrix_packed"),
               "oracle counts; conftest.pack_reference", run_packed, check_packed, lambda: counts_ref("ragged97", 3, 4), {})

    def run_batch(ctx, keep=None):
        b = ctx.encode_fasta(fasta_of(seqs))
        m = b.build_matrix(3)
        out = _matrix_out(m)
        _done(keep, m, b)
        return out

    yield Case("counts_seqbatch", "histograms", ("Context.encode_fasta", "SeqBatch.build_matrix"), "oracle counts",
               run_batch, lambda out: _check_matrix_out(out, counts_ref("ragged97", 3, 4), 2),
               lambda: counts_ref("ragged97", 3, 4), {})


def ingest_cases():
    def batch_out(b, prefix):
        return {prefix + "codes": b.codes(), prefix + "offsets": b.offsets.copy(),
                prefix + "header_positions": b.header_positions.copy()}

    def check_batch(out, prefix, labels_seqs):
        _, seqs = labels_seqs
        exp = np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)
        off = np.concatenate([[0], np.cumsum([s.size for s in seqs])]).astype(np.uint64)
        assert np.array_equal(out[prefix + "codes"], exp) and np.array_equal(out[prefix + "offsets"], off)

    def run_fasta(ctx, keep=None):
        raw = ingest_fasta()
        b = ctx.encode_fasta(raw)
        out = batch_out(b, "")
        out["labels"] = np.frombuffer("\n".join(b.labels).encode(), dtype=np.uint8).copy()
        j = ctx.encode_fasta(raw, join_records=True)
        out.update(batch_out(j, "joined_"))
        b.pack()
        out["packed_codes"], out["packed_mask"] = b.packed.planes()
        _done(keep, j, b)
        return out

    @functools.lru_cache(maxsize=None)
    def ref_fasta():
        raw = ingest_fasta()
        return oracle.load_fasta(raw), oracle.load_fasta(raw, join_records=True)

    def check_fasta(out):
        plain, joined = ref_fasta()
        check_batch(out, "", plain)
        check_batch(out, "joined_", joined)
        assert out["labels"].tobytes().decode() == "\n".join(plain[0])
        raw = np.frombuffer(ingest_fasta(), dtype=np.uint8)
        assert (raw[out["header_positions"].astype(np.int64)] == ord(">")).all() and out["header_positions"].size == len(plain[0])
        codes, mask = pack_reference(out["codes"])
        assert np.array_equal(out["packed_codes"], codes) and np.array_equal(out["packed_mask"], mask)

    yield Case("ingest_fasta_300k", "ingest", ("Context.encode_fasta", "SeqBatch.codes", "SeqBatch.pack"),
               "oracle.load_fasta", run_fasta, check_fasta, ref_fasta, {})

    def run_genbank(ctx, keep=None):
        b = ctx.encode_genbank(GENBANK)
        out = batch_out(b, "")
        _done(keep, b)
        return out

    yield Case("ingest_genbank", "ingest", ("Context.encode_genbank",), "oracle.load_genbank", run_genbank,
               lambda out: check_batch(out, "", oracle.load_genbank(GENBANK)), lambda: oracle.load_genbank(GENBANK), {})


def _strided_expect(d, fill, symmetric):
    """what a call over rows 1, 3, 5, ... of the lower triangle leaves in a matrix that held `fill`"""
    exp = np.full(d.shape, fill)
    for i in range(1, d.shape[0], 2):
        exp[i, :i] = d[i, :i]
        if symmetric:
            exp[:i, i] = d[i, :i]
    return exp


def sketch_cases():
    def sketches(name, states, k, s, canonical, entries):
        seqs = list(seqs65(states))
        n = len(seqs)

        def run(ctx, keep=None):
            sk, lens = distance.sketch_batch(seqs, k, s, states, canonical, ctx=ctx)
            h = distance.Sketches(seqs, k, s, states, canonical, ctx=ctx)
            hsk, hlens = h.to_host()
            out = dict(sketches=sk, lens=lens, handle_sketches=hsk, handle_lens=hlens, distances=h.distances())
            out["strided"] = h.distances(row_start=1, row_stride=2, out=np.full((n, n), 7.0))
            out["uploaded"] = distance.distances_from_sketches(sk, lens, k, s, ctx=ctx)
            out["uploaded_strided"] = distance.distances_from_sketches(sk, lens, k, s, row_start=1, row_stride=2,
                                                                       symmetric=False, out=np.full((n, n), 7.0), ctx=ctx)
            _done(keep, h)
            if entries:  # the same rows from the packed planes and from an ingested batch
                data, offs = engine.concat(seqs)
                p = ctx.pack_host(data)
                hp = distance.Sketches(None, k, s, 4, canonical, ctx=ctx, packed=p, offsets=offs)
                out["packed_sketches"], out["packed_lens"] = hp.to_host()
                b = ctx.encode_fasta(fasta_of(seqs))
                hb = distance.Sketches(None, k, s, 4, canonical, batch=b)
                out["batch_sketches"], out["batch_lens"] = hb.to_host()
                _done(keep, hp, p, hb, b)
            return out

        def check(out):
            exp, dist = sketch_ref("seqs65", k, s, states, canonical)
            for pre in ("", "handle_") + (("packed_", "batch_") if entries else ()):
                sk, lens = out[pre + "sketches"], out[pre + "lens"]
                assert lens.tolist() == [e.size for e in exp], pre
                assert all((sk[i, : lens[i]] == e).all() for i, e in enumerate(exp)), pre
            d = out["distances"]
            assert (np.diag(d) == 0).all() and np.array_equal(d, d.T) and (d[0, 1:] == 1.0).all()  # (an empty sketch)
            np.testing.assert_allclose(d, dist, rtol=MASH_RTOL, atol=0)
            assert same_bits(out["uploaded"], d)
            assert same_bits(out["strided"], _strided_expect(d, 7.0, True))
            assert same_bits(out["uploaded_strided"], _strided_expect(d, 7.0, False))

        ops = ("distance.sketch_batch", "Sketches.build", "Sketches.to_host", "Sketches.distances",
               "distance.distances_from_sketches") + (("Sketches.build_packed", "Sketches.build_batch") if entries else ())
        return Case(name, "sketches", ops, "oracle.mash_sketch, oracle.mash_distances", run, check,
                    lambda: sketch_ref("seqs65", k, s, states, canonical), {})

    yield sketches("sketch_s400_plain", 4, 12, 400, False, True)
    yield sketches("sketch_s400_canonical", 4, 12, 400, True, False)
    yield sketches("sketch_s16_plain", 4, 12, 16, False, False)
    yield sketches("sketch_s16_canonical", 4, 12, 16, True, False)
    yield sketches("sketch_20states_k3_generic", 20, 3, 50, False, False)


def _nearest_out(out, name, got):
    out[name + "_idx"], out[name + "_val"] = got


def _check_nearest(out, name, cross, kk):
    idx, val = out[name + "_idx"], out[name + "_val"]
    eidx, eval_ = expected_nearest(cross, kk)
    assert np.array_equal(idx, eidx) and same_bits(val, eval_) and np.array_equal(np.isnan(val), idx < 0)


def distance_cases():
    def count_modes(name, form, env):
        clean = form == "freq"  # (a frequency row must sum to one: no row without a valid k-mer)
        seqs = list(seqs257(clean))

        def run(ctx, keep=None):
            if form == "freq":
                m = ctx.matrix_from_freqs(np.stack([oracle.to_kfreqs(s, 4, 3)[0] for s in seqs]))
            else:
                m = ctx.build_matrix(seqs, 3, 4)
            out = {"count_bytes": np.array([m.count_bytes])}
            for mode in ("jsd", "euclidean"):
                side = distance.DeviceSide(m, mode)
                out[mode] = side.distances()
                out[mode + "_cross"] = side.cross_distances(side, Q_ROWS, R_ROWS)
                _nearest_out(out, mode + "_nearest", side.nearest(side, 5, Q_ROWS, R_ROWS))
            sel = m.nmost(10)  # Selection.assign over this element type: the two nearest members of every row
            out["member_rows"] = sel.member_rows()
            for mode in ("jsd", "euclidean"):
                _nearest_out(out, f"assign_{mode}", sel.assign(2, mode))
            _done(keep, sel, m)
            return out

        def check(out):
            assert out["count_bytes"][0] == {"u16": 2, "u32": 4, "freq": 0}[form]
            off = ~np.eye(N, dtype=bool)
            nan = np.zeros((N, N), dtype=bool)
            if not clean:
                nan[7, :] = nan[:, 7] = True
            for mode, exp in (("jsd", jsd_ref(clean)), ("euclidean", euclid_ref(clean))):
                d = out[mode]
                assert (np.diag(d) == 0).all() and same_bits(d, d.T) and np.array_equal(np.isnan(d), nan & off)
                ok = off & ~nan
                if mode == "jsd":
                    assert np.abs(d[ok] - exp[ok]).max() <= tol_derived(64) and d[11, 5] == 0.0
                else:
                    np.testing.assert_allclose(d[ok], exp[ok], rtol=EUCLID_RTOL, atol=0)
                assert same_bits(out[mode + "_cross"], d[np.ix_(Q_ROWS, R_ROWS)])
                _check_nearest(out, mode + "_nearest", out[mode + "_cross"], 5)
                # (a member's own row: the square matrix's 0 on the diagonal is the rectangular cell of a row with k-mers)
                _check_nearest(out, f"assign_{mode}", d[:, out["member_rows"]], 2)
            assert out["member_rows"].tolist() == members_ref(clean, form == "freq").tolist()

        ops = ("Selection.assign", "Selection.member_rows") + tuple(f"DeviceSide.{op}:{mode}" for op in ("distances", "cross_distances", "nearest") for mode in ("jsd", "euclidean"))
        ops += ("Context.matrix_from_freqs",) if form == "freq" else ()
        return Case(name, "distances", ops, "oracle_jsd_matrix (tol_derived), numpy euclidean (EUCLID_RTOL), expected_nearest",
                    run, check, lambda: (jsd_ref(clean), euclid_ref(clean), members_ref(clean, form == "freq")), env)

    yield count_modes("distances_u16", "u16", {})
    yield count_modes("distances_u32", "u32", {"DVS_COUNTS_U32": "1"})
    yield count_modes("distances_freq", "freq", {})

    seqs = list(seqs257(True))

    def run_mash(ctx, keep=None):
        side = distance.device_side(seqs, "mash", 12, 400, 4, False, ctx=ctx)
        out = {"mash": side.distances(), "mash_cross": side.cross_distances(side, Q_ROWS, R_ROWS)}
        _nearest_out(out, "mash_nearest", side.nearest(side, 5, Q_ROWS, R_ROWS))
        _done(keep, side)
        return out

    def check_mash(out):
        d = out["mash"]
        assert (np.diag(d) == 0).all() and np.array_equal(d, d.T) and d[11, 5] == 0.0
        np.testing.assert_allclose(d, sketch_ref("clean257", 12, 400, 4, False)[1], rtol=MASH_RTOL, atol=0)
        assert same_bits(out["mash_cross"], d[np.ix_(Q_ROWS, R_ROWS)])
        _check_nearest(out, "mash_nearest", out["mash_cross"], 5)

    yield Case("distances_mash", "distances", tuple(f"DeviceSide.{op}:mash" for op in ("distances", "cross_distances", "nearest")),
               "oracle.mash_distances (MASH_RTOL), expected_nearest", run_mash, check_mash,
               lambda: sketch_ref("clean257", 12, 400, 4, False), {})


def tree_cases():
    def linkage(name, matrix):
        def run(ctx, keep=None):
            return {method: cluster.linkage(matrix(), method, ctx=ctx) for method in METHODS}

        def ref():
            return {method: scipy_z(matrix(), method) for method in METHODS}

        def check(out):
            for method, z in ref().items():
                assert np.array_equal(out[method], z), method

        return Case(name, "trees", ("cluster.linkage",), "scipy_z, bit for bit", run, check, functools.lru_cache(None)(ref), {})

    yield linkage("linkage_random257", random257)
    yield linkage("linkage_ties257", ties257)
    yield linkage("linkage_ties120", ties120)

    seqs = list(seqs257(True))
    fused_methods = ("average", "single", "ward")

    def sides(ctx):
        return (distance.device_side(seqs, "mash", 12, 400, 4, False, ctx=ctx), distance.device_side(seqs, "euclidean", 3, 4, ctx=ctx),
                distance.device_side(seqs, "jsd", 3, 4, ctx=ctx))

    def run_fused(ctx, keep=None):
        out = {}
        for side in sides(ctx):
            out[side.mode] = side.distances()
            for method in fused_methods:
                out[f"{side.mode}_{method}"] = side.linkage(method)
            _done(keep, side)
        return out

    def check_fused(out):
        for mode in distance.DeviceSide.MODE_NAMES:
            for method in fused_methods:  # the fused matrix is the standalone one: scipy over the device's own matrix
                assert np.array_equal(out[f"{mode}_{method}"], scipy_z(out[mode], method)), (mode, method)
        assert np.abs(out["jsd"] - jsd_ref(True)).max() <= tol_derived(64)

    yield Case("linkage_fused", "trees", tuple(f"DeviceSide.linkage:{m}" for m in distance.DeviceSide.MODE_NAMES),
               "scipy_z over the mode's own matrix; oracle_jsd_matrix", run_fused, check_fused, lambda: jsd_ref(True), {})

    def run_nj(ctx, keep=None):
        out = {}
        for label, d in (("dyadic", dyadic_tree(N, "random")[1]), ("general", general_yardstick("noisy0.1", N)[0]),
                         ("ties", tie_case("small-integer", N))):
            t = cluster.neighbor_joining(d, ctx=ctx)
            out[label + "_children"], out[label + "_lengths"] = t.children, t.lengths
        return out

    @functools.lru_cache(maxsize=None)
    def ref_nj():
        return dyadic_tree(N, "random"), general_yardstick("noisy0.1", N), restated(tie_case("small-integer", N))

    def check_nj(out):
        (tree, A), (d, want, _, err), ties = ref_nj()
        got = (out["dyadic_children"], out["dyadic_lengths"])
        assert split_lengths(got, N) == split_lengths(tree, N) and np.array_equal(cluster.patristic(got), A)
        got = split_lengths((out["general_children"], out["general_lengths"]), N)
        assert set(got) == set(want)
        same_tree(got, want, length_tolerance(N, d, err))
        assert np.array_equal(out["ties_children"], ties.children) and np.array_equal(out["ties_lengths"], ties.lengths)

    yield Case("nj_matrices257", "trees", ("cluster.neighbor_joining",), "dyadic_tree, general_yardstick, restated", run_nj,
               check_nj, ref_nj, {})

    def run_nj_fused(ctx, keep=None):
        out = {}
        for side in sides(ctx):
            out[side.mode] = side.distances()
            t = side.nj()
            out[side.mode + "_children"], out[side.mode + "_lengths"] = t.children, t.lengths
            _done(keep, side)
        return out

    def check_nj_fused(out):
        for mode in distance.DeviceSide.MODE_NAMES:  # (test_gpu_nj.py _fused_check; duplicates: zero-length edges merged)
            d = out[mode]
            tc, tl, _ = truth(d)
            want, ref = split_lengths((tc, tl), N), split_lengths(restated(d), N)
            err = max(abs(float(ref[k] - want[k])) for k in want if k in ref)
            same_tree(split_lengths((out[mode + "_children"], out[mode + "_lengths"]), N), want, length_tolerance(N, d, err),
                      merge_zero=True)

    yield Case("nj_fused", "trees", tuple(f"DeviceSide.nj:{m}" for m in distance.DeviceSide.MODE_NAMES),
               "truth / restated over the mode's own matrix", run_nj_fused, check_nj_fused,
               lambda: truth(jsd_ref(True)), {})  # (the check: over the device's own matrix; here: over the oracle's)


def cophenet_cluster_cases():
    env = {"DVS_CROSS_STRIP_ROWS": "7"}  # 37 strips reuse one strip block
    seqs = list(seqs257(True))

    def scores_out(out, name, sc):
        for f in sc._fields:
            if getattr(sc, f) is not None:
                out[f"{name}_{f}"] = np.asarray(getattr(sc, f))

    def scores_in(out, name, cls):
        vals = {f: out.get(f"{name}_{f}") for f in cls._fields}
        if cls is distance.ClusterScores:
            vals["mean_silhouette"] = float(vals["mean_silhouette"])
        else:
            vals["correlation"] = float(vals["correlation"])
        return cls(**vals)

    def run_matrix(ctx, keep=None):
        out = {}
        scores_out(out, "cophenet", cluster.cophenet(tree257(), symmetric257(), matrix=True, ctx=ctx))
        scores_out(out, "clusters", cluster.cluster_scores(symmetric257(), labels257(), ctx=ctx))
        out["cut"] = cluster.cut_tree(tree257(), n_clusters=6)
        return out

    def check_matrix(out):
        from scipy.cluster.hierarchy import fcluster
        from test_gpu_clusters import assert_scores as assert_cluster_scores
        from test_gpu_cophenet import assert_scores as assert_cophenet_scores

        assert_cophenet_scores(scores_in(out, "cophenet", distance.CopheneticScores), symmetric257(), tree257())
        assert_cluster_scores(scores_in(out, "clusters", distance.ClusterScores), symmetric257(), labels257(), with_sklearn=False)
        assert np.array_equal(out["cut"], first_appearance(fcluster(tree257(), 6, "maxclust")))

    yield Case("scores_matrix257", "cophenet_clusters", ("cluster.cophenet", "cluster.cluster_scores", "cluster.cut_tree"),
               "truth_correlation / truth_row_sums, truth_cluster_scores, scipy fcluster", run_matrix, check_matrix,
               lambda: (truth_correlation(symmetric257(), tree257()), truth_cluster_scores(symmetric257(), labels257())), env)

    def run_modes(ctx, keep=None):
        out = {}
        for side in (distance.device_side(seqs, "mash", 12, 400, 4, False, ctx=ctx), distance.device_side(seqs, "euclidean", 3, 4, ctx=ctx),
                     distance.device_side(seqs, "jsd", 3, 4, ctx=ctx)):
            out[side.mode] = side.distances()
            scores_out(out, side.mode + "_cophenet", side.cophenet(tree257()))
            scores_out(out, side.mode + "_clusters", side.cluster_scores(labels257()))
            _done(keep, side)
        return out

    def check_modes(out):
        from test_gpu_clusters import assert_scores as assert_cluster_scores
        from test_gpu_cophenet import assert_scores as assert_cophenet_scores

        for mode in distance.DeviceSide.MODE_NAMES:
            d = out[mode]
            got = scores_in(out, mode + "_cophenet", distance.CopheneticScores)
            assert_cophenet_scores(got, d, tree257(), mode)
            assert_cluster_scores(scores_in(out, mode + "_clusters", distance.ClusterScores), d, labels257(), mode, with_sklearn=False)

    ops = tuple(f"DeviceSide.{op}:{m}" for op in ("cophenet", "cluster_scores") for m in distance.DeviceSide.MODE_NAMES)
    yield Case("scores_modes257", "cophenet_clusters", ops, "the yardsticks over the mode's own matrix", run_modes, check_modes,
               lambda: tree257(), env)


def maxmin_cases():
    env = {"DVS_MAXMIN_BATCH": "3"}
    seed_sets = ((0,), (5, 200, 33))

    def mm_out(out, name, got):
        out[name + "_picks"], out[name + "_radius"], out[name + "_owner"] = got.picks, got.radius, got.owner
        out[name + "_dist"], out[name + "_cover"] = got.dist, np.array([got.cover])

    def mm_check(out, name, d, seeds):
        exp = maxmin_ref(d, 20, seeds)
        assert np.array_equal(out[name + "_picks"], exp.picks) and np.array_equal(out[name + "_owner"], exp.owner), name
        assert same_bits(out[name + "_radius"], exp.radius) and same_bits(out[name + "_dist"], exp.dist), name
        assert same_bits(out[name + "_cover"], [exp.cover]), name

    def mode_case(mode):
        seqs = list(seqs257(mode == "mash"))  # (two empty sketches would divide by zero: the clean rows for mash)
        args = (12, 400, 4, False) if mode == "mash" else (3, 4)

        def run(ctx, keep=None):
            side = distance.device_side(seqs, mode, *args, ctx=ctx)
            out = {mode: side.distances()}
            for i, seeds in enumerate(seed_sets):
                mm_out(out, f"seeds{i}", side.maxmin(20, seeds=seeds))
            _done(keep, side)
            return out

        def check(out):
            for i, seeds in enumerate(seed_sets):
                mm_check(out, f"seeds{i}", out[mode], seeds)

        def ref():  # (the check runs maxmin_ref over the device's own matrix; here, over the CPU reference's matrix)
            d = {"mash": lambda: sketch_ref("clean257", 12, 400, 4, False)[1], "jsd": lambda: jsd_ref(False),
                 "euclidean": lambda: euclid_ref(False)}[mode]()
            return [maxmin_ref(d, 20, seeds) for seeds in seed_sets]

        return Case(f"maxmin_{mode}", "maxmin", (f"DeviceSide.maxmin:{mode}",), "maxmin_ref over the mode's own matrix", run,
                    check, ref, env)

    for mode in distance.DeviceSide.MODE_NAMES:
        yield mode_case(mode)

    def run_matrix(ctx, keep=None):
        out = {}
        for i, seeds in enumerate(seed_sets):
            mm_out(out, f"seeds{i}", cluster.maxmin(random257(), 20, seeds=seeds, ctx=ctx))
        return out

    def check_matrix(out):
        for i, seeds in enumerate(seed_sets):
            mm_check(out, f"seeds{i}", random257(), seeds)

    yield Case("maxmin_matrix257", "maxmin", ("cluster.maxmin",), "maxmin_ref", run_matrix, check_matrix,
               lambda: [maxmin_ref(random257(), 20, s) for s in seed_sets], env)


SUMMARY_FIELDS = ("size", "lowest_index", "total_jsd", "mean_delta_jsd", "std_delta_jsd", "cov_delta_jsd", "summed_entropies")


def _selection_out(ctx, sel, shape: int, extras: bool) -> dict:
    """what is read back from a finished selection: members, the summary's results (no work counters), delta_jsd over
    six query rows, the gathered member rows and a matrix made of them, the two nearest members of every row"""
    import torch

    k = SELECT_SHAPES[shape][2]
    mem = sel.members()
    out = dict(positions=mem.positions, labels=mem.labels, delta_jsd=mem.delta_jsd, entropy=mem.entropy, kfreqs=mem.kfreqs)
    s = sel.summary()
    out["summary"] = np.array([float(getattr(s, f)) for f in SUMMARY_FIELDS])
    q = ctx.build_matrix(list(query_seqs(shape)), k, 4)
    out["query_delta_jsd"] = sel.delta_jsd(q)
    q.close()
    cap = mem.positions.size + 3
    rows_t = torch.full((cap, sel.matrix.nbins), -1.0, dtype=torch.float64, device="cuda:0")
    meta_t = torch.full((cap, 2), -1.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    sel.gather_members(rows_t.data_ptr(), meta_t.data_ptr(), cap)
    fm = ctx.matrix_from_device_freqs(rows_t.data_ptr(), cap, sel.matrix.nbins, meta_t.data_ptr())
    out["gathered_totals"], out["gathered_entropy"], out["gathered_source_rows"] = fm.totals(), fm.entropy(), fm.source_rows()
    fm.close()
    ctx.sync()
    out["gathered_rows"], out["gathered_meta"] = rows_t.cpu().numpy(), meta_t.cpu().numpy()
    if extras:
        # (labels no member carries: the scores of the unlabelled call, through the call's second block)
        q = ctx.build_matrix(list(query_seqs(shape)), k, 4)
        out["query_delta_jsd_labelled"] = sel.delta_jsd(q, np.full(q.nrows, 0xFFFFFFFF, dtype=np.uint32))
        q.close()
        out["assign_idx"], out["assign_val"] = sel.assign(2, "jsd")
        out["bench_scan_rows"] = np.array([sel.bench_scan(1)[1]])
    return out


def _check_selection_out(out, exp, shape, position_of=lambda p: p):
    """tests/test_gpu_parity.py _assert_selection, over the outputs"""
    elab, edelta, eent, efreq = exp.members(with_freqs=True)
    n = elab.size
    summary = dict(zip(SUMMARY_FIELDS, out["summary"]))
    assert summary["size"] == exp.size == n
    assert [int(position_of(p)) for p in out["positions"]] == elab.tolist(), "selected ids / member order differ"
    np.testing.assert_allclose(out["delta_jsd"], edelta, rtol=RTOL, atol=1e-13)
    np.testing.assert_allclose(out["entropy"], eent, rtol=RTOL)
    assert (out["kfreqs"] == efreq).all(), "member frequency rows must be bit-exact (count / total)"
    for name in ("total_jsd", "mean_delta_jsd", "std_delta_jsd", "cov_delta_jsd"):
        g, e = summary[name], getattr(exp, name)
        if np.isnan(e) or np.isinf(e):
            assert (np.isnan(g) and np.isnan(e)) or g == e, (name, g, e)
        else:
            assert abs(g - e) <= RTOL * max(abs(e), 1e-300) + 1e-13, (name, g, e)
    assert summary["lowest_index"] == exp.lowest_index
    k = SELECT_SHAPES[shape][2]
    for i, s in enumerate(query_seqs(shape)):  # (tests/test_gpu_parity.py test_delta_jsd_calculator)
        if oracle.count_kmers(s, 4, k).sum() == 0:
            assert np.isnan(out["query_delta_jsd"][i])
        else:
            f, h = oracle.to_kfreqs(s, 4, k)
            np.testing.assert_allclose(out["query_delta_jsd"][i], exp.delta_jsd(f, h), rtol=TIGHT)
    assert np.array_equal(out["gathered_rows"][:n], out["kfreqs"]) and (out["gathered_rows"][n:] == 0).all()
    assert np.array_equal(out["gathered_meta"][:n, 0], out["positions"].astype(np.float64))
    assert (out["gathered_meta"][:n, 1] == 1).all() and (out["gathered_meta"][n:] == 0).all()
    assert out["gathered_totals"].tolist() == [1] * n + [0] * 3 and out["gathered_source_rows"].tolist() == list(range(n + 3))
    np.testing.assert_allclose(out["gathered_entropy"][:n], eent, rtol=RTOL)
    if "assign_idx" in out:
        assert same_bits(out["query_delta_jsd_labelled"], out["query_delta_jsd"])
        members = out["positions"].astype(np.int64)
        assert (out["assign_idx"][members, 0] == np.arange(n)).all() and (out["assign_val"][members, 0] == 0).all()
        assert out["bench_scan_rows"][0] == SELECT_SHAPES[shape][0] - SELECT_SHAPES[shape][3]


@functools.lru_cache(maxsize=None)
def collision_seqs() -> tuple:
    return tuple(synth_seqs(8000, 200, 8003, ragged=True))


@functools.lru_cache(maxsize=None)
def collision_ref():
    return oracle.nmost(list(collision_seqs()), 10, 3, 4)


@functools.lru_cache(maxsize=None)
def head_phase_seqs() -> tuple:
    return tuple(synth_seqs(17_600, 120, 17_603, ragged=True, invalid_frac=0.001))


@functools.lru_cache(maxsize=None)
def head_phase_ref():
    return oracle.nmost(list(head_phase_seqs()), 10, 4, 4)


def selection_cases():
    def case(shape, what, env=None, ops=()):
        nseq, length, k, n = SELECT_SHAPES[shape]
        seqs = list(select_seqs(shape))

        def run(ctx, keep=None):
            import torch

            source = None
            if what == "resident":  # a device-resident build that is not waited for, the selection right behind it
                data, offs = oracle.concat(list(resident_seqs(shape)))
                source = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to("cuda:0")
                torch.cuda.synchronize()
                m = ctx.build_matrix_device(source.data_ptr(), offs, k, 4)
            else:
                m = ctx.build_matrix(seqs, k, 4)
            if what in ("nmost", "no_persist", "resident"):
                sel = m.nmost(n)
            elif what in ("stdev", "cov"):
                sel = m.max_divergent(n, 3 * n, what)
            elif what == "order":
                sel = m.nmost(n, order=select_order(shape), labels=select_order(shape))
            else:  # tests/test_gpu_configs.py test_stepwise_selection_without_an_order_array
                from diverseseq_amd.parallel import HipStepper, drive_exact

                sel = m.select(_lib.MODE_NMOST, n, window=4096, flags=_lib.SELECT_STEPWISE)
                stepper = HipStepper(ctx, sel, m.nbins, torch.device("cuda:0"))
                torch.cuda.synchronize()
                drive_exact(stepper, 1, torch.device("cuda:0"))
            out = _selection_out(ctx, sel, shape, extras=what == "nmost")
            if what == "nmost":
                grown = sel.diversify(n + 5, "jsd")
                out["diversify_picks"], out["diversify_radius"] = grown.picks, grown.radius
            _done(keep, sel, m)
            del source
            return out

        ref_key = {"no_persist": "nmost", "stepwise": "nmost"}.get(what, what)

        def check(out):
            order = select_order(shape)
            _check_selection_out(out, select_ref(shape, ref_key), shape, (lambda p: order[p]) if what == "order" else (lambda p: p))
            if what == "nmost":
                assert np.array_equal(out["diversify_picks"][:n], out["positions"].astype(np.int64))
                assert np.isnan(out["diversify_radius"][:n]).all() and (np.diff(out["diversify_radius"][n:]) <= 0).all()

        base = ("CountMatrix.select", "Selection.members", "Selection.delta_jsd", "Selection.gather_members",
                "Context.matrix_from_device_freqs")
        return Case(f"select{shape}_{what}", "selections", base + tuple(ops), "oracle selection", run, check,
                    lambda: select_ref(shape, ref_key), env or {})

    def run_collision(ctx, keep=None):
        """a device-resident build that is not waited for is closed at once, and a selection starts right behind a second
        unwaited build: the first one's 1 500 totals (6 000 bytes) and the second selection's 8 000 label flags fall into
        the same 8 KiB class of the cache, and the selection's set-up writes its blocks on a side stream"""
        import torch

        def resident(seqs):
            data, offs = oracle.concat(list(seqs))
            t = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to("cuda:0")
            torch.cuda.synchronize()
            return t, ctx.build_matrix_device(t.data_ptr(), offs, 3, 4)

        ta, a = resident(collision_seqs()[:1500])
        a.close()
        tb, b = resident(collision_seqs())
        sel = b.nmost(10)
        mem, s = sel.members(), sel.summary()
        out = dict(positions=mem.positions, delta_jsd=mem.delta_jsd, entropy=mem.entropy, kfreqs=mem.kfreqs,
                   summary=np.array([float(getattr(s, f)) for f in SUMMARY_FIELDS]))
        _done(keep, sel, b)
        ctx.sync()
        del ta, tb
        return out

    def check_collision(out, exp=None):
        exp = exp or collision_ref()
        elab, edelta, eent, efreq = exp.members(with_freqs=True)
        assert out["positions"].tolist() == elab.tolist() and (out["kfreqs"] == efreq).all()
        np.testing.assert_allclose(out["delta_jsd"], edelta, rtol=RTOL, atol=1e-13)
        np.testing.assert_allclose(out["entropy"], eent, rtol=RTOL)
        summary = dict(zip(SUMMARY_FIELDS, out["summary"]))
        assert summary["size"] == exp.size and summary["lowest_index"] == exp.lowest_index
        assert abs(summary["total_jsd"] - exp.total_jsd) <= RTOL * abs(exp.total_jsd) + 1e-13

    yield Case("select_behind_a_closed_unwaited_build", "selections", ("Context.build_matrix_device", "CountMatrix.select"),
               "oracle selection", run_collision, check_collision, collision_ref, {})

    def run_head_phase(ctx, keep=None):
        """a device-resident build of more than 17 408 rows is split -- the head rows first, the rest on the CU-masked
        stream -- and the selection behind it starts its persistent engine on the head CUs meanwhile: its set-up and
        the head phase's blocks go out on side streams (tests/test_gpu_configs.py test_head_phase_of_a_split_build_vs_oracle)"""
        import torch

        data, offs = oracle.concat(list(head_phase_seqs()))
        t = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to("cuda:0")
        torch.cuda.synchronize()
        m = ctx.build_matrix_device(t.data_ptr(), offs, 4, 4)
        sel = m.nmost(10)
        mem, s = sel.members(), sel.summary()
        out = dict(positions=mem.positions, delta_jsd=mem.delta_jsd, entropy=mem.entropy, kfreqs=mem.kfreqs,
                   summary=np.array([float(getattr(s, f)) for f in SUMMARY_FIELDS]), count_bytes=np.array([m.count_bytes]))
        _done(keep, sel, m)
        ctx.sync()
        del t
        return out

    def check_head_phase(out):
        assert out["count_bytes"][0] == 2 and len(head_phase_seqs()) - 1024 >= 16 * 1024  # (what makes the build split)
        check_collision(out, head_phase_ref())

    yield Case("select_head_phase", "selections", ("Context.build_matrix_device", "CountMatrix.select"), "oracle selection",
               run_head_phase, check_head_phase, head_phase_ref, {})

    for shape in range(len(SELECT_SHAPES)):
        yield case(shape, "nmost", ops=("Selection.assign", "Selection.member_rows", "Selection.bench_scan", "Selection.diversify"))
        yield case(shape, "no_persist", env={"DVS_NO_PERSIST": "1"})
        yield case(shape, "stdev")
        yield case(shape, "cov")
        yield case(shape, "order")
        yield case(shape, "stepwise")
        yield case(shape, "resident", ops=("Context.build_matrix_device",))


# ------------------------------------------------------------------ the operations added after the first table

def _put(out, name, got):
    """a NamedTuple result into the outputs, field by field (scalars as 0-d arrays)"""
    for field, value in zip(got._fields, got):
        out[f"{name}.{field}"] = np.asarray(value)


def _get(out, name, cls):
    """... and back: arrays as they are, scalars as Python's"""
    return cls(*(out[f"{name}.{f}"] if out[f"{name}.{f}"].ndim else out[f"{name}.{f}"].item() for f in cls._fields))


def _mode_side(ctx, mode, clean=True, mash=(12, 400)):
    """the side of one distance mode over the 257 sequences (mash: always the clean rows, two empty sketches would
    divide by zero)"""
    if mode == "mash":
        return distance.device_side(list(seqs257(True)), "mash", *mash, 4, False, ctx=ctx)
    return distance.device_side(list(seqs257(clean)), mode, 3, 4, ctx=ctx)


def _mode_ref(mode, clean=True, mash=(12, 400)) -> np.ndarray:
    """the CPU reference's matrix of that side"""
    if mode == "mash":
        return sketch_ref("clean257", *mash, 4, False)[1]
    return (euclid_ref if mode == "euclidean" else jsd_ref)(clean)


def _per_mode(name, family, ops, reference, run, check, ref, env) -> list:
    """one case per distance mode (a case over all three would make three times the requests, each run three times as
    long): run(ctx, mode) -> outputs, check(out, mode), ref(mode)"""
    return [Case(f"{name}_{mode}257", family, tuple(f"DeviceSide.{op}:{mode}" for op in ops[0]) + tuple(ops[1]), reference,
                 functools.partial(lambda ctx, keep=None, *, mode: run(ctx, mode, keep), mode=mode),
                 functools.partial(check, mode=mode), functools.partial(ref, mode), env)
            for mode in distance.DeviceSide.MODE_NAMES]


# radii between two cell values of the CPU references' matrices (about 2 % of the cells for the lists, about two edges a
# row for the components); the lists are checked against the device's own matrix, so the exact place does not matter
WITHIN_RADII = {"mash": (0.33, 0.30), "euclidean": (0.0428, 0.0407), "jsd": (0.0217, 0.0195), "matrix": (0.02, 0.008)}


def neighbour_cases():
    from test_within_host import expected_components, expected_within

    env = {"DVS_CROSS_STRIP_ROWS": "7"}  # 37 strips reuse one strip block and grow one pair buffer

    def check_lists(out, name, d, radii):
        nb, tc = _get(out, name + "_within", distance.Neighbours), _get(out, name + "_clusters", distance.ThresholdClusters)
        rs, idx, val = expected_within(d, radii[0], skip_self=True)
        assert np.array_equal(nb.row_start, rs) and np.array_equal(nb.index, idx) and same_bits(nb.distance, val), name
        assert N < idx.size < N * N // 4, (name, idx.size)
        labels = expected_components(d, radii[1])
        assert np.array_equal(tc.labels, labels) and tc.n_clusters == labels.max() + 1, name
        assert np.array_equal(tc.sizes, np.bincount(labels)) and 1 < tc.n_clusters < N, (name, tc.n_clusters)

    def run_matrix(ctx, keep=None):
        out = {}
        _put(out, "matrix_within", cluster.within(symmetric257(), WITHIN_RADII["matrix"][0], ctx=ctx))
        _put(out, "matrix_clusters", cluster.threshold_clusters(symmetric257(), WITHIN_RADII["matrix"][1], ctx=ctx))
        return out

    yield Case("within_matrix257", "neighbours", ("cluster.within", "cluster.threshold_clusters"),
               "expected_within, expected_components", run_matrix,
               lambda out: check_lists(out, "matrix", symmetric257(), WITHIN_RADII["matrix"]),
               lambda: (expected_within(symmetric257(), WITHIN_RADII["matrix"][0], True),
                        expected_components(symmetric257(), WITHIN_RADII["matrix"][1])), env)

    def run_mode(ctx, mode, keep=None):
        side = _mode_side(ctx, mode, clean=False, mash=(8, 50))  # (row 7 of the count modes: NaN cells, never listed)
        out = {"distances": side.distances()}
        _put(out, "mode_within", side.within(side, WITHIN_RADII[mode][0], skip_self=True))
        _put(out, "mode_clusters", side.threshold_clusters(WITHIN_RADII[mode][1]))
        _done(keep, side)
        return out

    def check_mode(out, mode):
        check_lists(out, "mode", out["distances"], WITHIN_RADII[mode])
        if mode != "mash":
            assert np.isnan(out["distances"][7, 8]) and 7 not in out["mode_within.index"]

    def ref_mode(mode):  # (the check: over the device's own matrix; here: over the oracle's)
        d = _mode_ref(mode, False, (8, 50))
        return expected_within(d, WITHIN_RADII[mode][0], True), expected_components(d, WITHIN_RADII[mode][1])

    yield from _per_mode("within", "neighbours", (("within", "threshold_clusters", "distances"), ()),
                         "expected_within, expected_components over the mode's own matrix", run_mode, check_mode, ref_mode, env)


def canonical_cases():
    from test_canonical_host import ENTROPY_TOL, folded, ragged
    from test_distance_truth_host import truth_euclid_rows, truth_jsd_rows

    seqs, k = list(ragged(65)), 3

    def run(ctx, keep=None):
        f = ctx.build_matrix(seqs, k, canonical=True)
        out = _matrix_out(f)
        for mode in ("jsd", "euclidean"):
            out[mode] = distance.DeviceSide(f, mode).distances()
        plain = ctx.build_matrix(seqs, k)
        again = plain.canonical()  # (the fold of a matrix that stays open)
        out["again_counts"] = again.counts()
        _done(keep, f, plain, again)
        return out

    def check(out):
        """tests/test_gpu_canonical.py test_fold_against_the_yardstick, test_distances_of_the_folded_matrix_against_the_truth"""
        counts, totals, ent = folded(seqs, k)
        assert out["count_bytes"][0] == 2
        assert np.array_equal(out["counts"], counts) and np.array_equal(out["again_counts"], counts)
        assert np.array_equal(out["totals"], totals)
        live = np.flatnonzero(totals > 0)
        assert (np.abs(out["entropy"][live] - ent[live]) <= ENTROPY_TOL * np.maximum(1.0, np.abs(ent[live]))).all()
        pairs = np.array([(i, j) for a, i in enumerate(live) for j in live[a + 1:]])
        err = np.abs(out["jsd"][pairs[:, 0], pairs[:, 1]].astype(np.longdouble) - truth_jsd_rows(counts, pairs))
        assert float(err.max()) <= tol_derived(counts.shape[1])
        truth = truth_euclid_rows(counts, pairs)
        rel = np.abs(out["euclidean"][pairs[:, 0], pairs[:, 1]].astype(np.longdouble) - truth) / truth
        assert (truth > 0).all() and float(rel.max()) <= EUCLID_RTOL
        dead = np.flatnonzero(totals == 0)
        assert dead.size == 3 and np.isnan(out["jsd"][dead][:, live]).all() and (np.diag(out["jsd"]) == 0).all()

    yield Case("canonical_k3", "histograms", ("Context.build_matrix", "CountMatrix.canonical", "DeviceSide.distances:jsd",
                                              "DeviceSide.distances:euclidean"),
               "test_canonical_host.folded; truth_jsd_rows (tol_derived), truth_euclid_rows (EUCLID_RTOL)", run, check,
               lambda: folded(seqs, k), {})


def _pcoa_holds(fit, d, label, n_axes):
    """tests/test_gpu_pcoa.py check_contract over a yardstick of the matrix d itself: the sign rule, honest residuals,
    orthonormal vectors orthogonal to 1, eigenvalues within Weyl's bound, the definitions"""
    from test_pcoa_host import EPS, Yardstick, sign_rule

    y, n, m = Yardstick(d), d.shape[0], n_axes
    unit = y.unit(n)
    assert fit.converged and fit.vectors.shape == fit.coordinates.shape == (n, m) and (np.diff(fit.values) <= 0).all(), label
    assert same_bits(sign_rule(fit.vectors), fit.vectors), label
    true_res = np.linalg.norm(y.B @ fit.vectors - fit.vectors * fit.values, axis=0)
    basis = max(fit.basis, 1)
    assert np.abs(true_res - fit.residuals).max() <= unit, label
    assert np.abs(fit.vectors.T @ fit.vectors - np.eye(m)).max() <= (n + 8) * EPS * basis, label
    assert np.abs(fit.vectors.sum(axis=0)).max() <= (n + 8) * EPS * basis * np.sqrt(n), label
    assert (np.abs(fit.values - y.values[:m]) <= fit.residuals + y.residuals[:m] + np.finfo(float).tiny).all(), label
    pos = fit.values > 0
    assert same_bits(fit.coordinates, np.where(pos, fit.vectors * np.sqrt(np.where(pos, fit.values, 0.0)), 0.0)), label
    assert same_bits(fit.proportion, fit.values / fit.trace) and abs(fit.trace - y.trace) <= 4 * n * EPS * y.trace, label
    assert np.abs(fit.row_means - y.mu).max() <= 4 * n * EPS * np.abs(y.mu).max(), label


def ordination_cases():
    import test_pcoa_host as ph

    shapes = (("cloud6", 9), ("jsd", 3))  # nine axes: one past a chunk of the Ritz kernel; a non-Euclidean matrix

    def run_matrix(ctx, keep=None):
        out = {}
        for kind, m in shapes:
            _put(out, kind, cluster.pcoa(ph.case(kind, N), m, ctx=ctx))
        return out

    def check_matrix(out):
        for kind, m in shapes:
            _pcoa_holds(_get(out, kind, distance.PCoA), ph.case(kind, N), kind, m)

    yield Case("pcoa_matrix257", "ordination", ("cluster.pcoa",), "test_pcoa_host.Yardstick, check_contract's bounds",
               run_matrix, check_matrix, lambda: [ph.yardstick(kind, N) for kind, _ in shapes], {})

    marks = np.arange(0, N, 2)  # the fitted rows of the projection: 129 of the 257

    def run_mode(ctx, mode, keep=None):
        side = _mode_side(ctx, mode)
        out = {"distances": side.distances()}
        _put(out, "fused", side.pcoa(3))
        _put(out, "route", cluster.pcoa(out["distances"], 3, ctx=ctx))
        fit = cluster.pcoa(side.cross_distances(side, marks, marks), 3, ctx=ctx)
        _put(out, "marks", fit)
        out["projected"] = side.pcoa_project(fit, side, None, marks)
        _done(keep, side)
        return out

    def check_mode(out, mode):
        """tests/test_gpu_pcoa.py: the fused route is the matrix route bit for bit; a projection against Gower's formula
        in numpy over the same cells (test_projection_row_lists_nan_rows_and_many_axes' bound)"""
        d, fused = out["distances"], _get(out, "fused", distance.PCoA)
        assert all(same_bits(a, b) for a, b in zip(fused, _get(out, "route", distance.PCoA))), mode
        _pcoa_holds(fused, d, mode, 3)
        fit = _get(out, "marks", distance.PCoA)
        _pcoa_holds(fit, d[np.ix_(marks, marks)], mode + " marks", 3)
        ref = ph.project(d[:, marks], fit.values, fit.vectors, fit.row_means)
        unit = marks.size * ph.EPS * np.abs(fit.coordinates).max() / np.sqrt(fit.values[fit.values > 0].min() / fit.values[0])
        assert np.abs(out["projected"] - ref).max() <= 8 * unit, mode
        assert np.abs(out["projected"][marks] - fit.coordinates).max() <= 1e-9 * np.abs(fit.coordinates).max(), mode

    yield from _per_mode("pcoa", "ordination", (("pcoa", "pcoa_project", "cross_distances", "distances"), ("cluster.pcoa",)),
                         "the yardstick over the mode's own matrix; test_pcoa_host.project", run_mode, check_mode,
                         lambda mode: ph.Yardstick(_mode_ref(mode)), {})


def medoid_cases():
    import kmedoids_cases as kc

    exact = tuple(kc.Case("clustered", N, k, init, 300, 2) for k in (7, 17) for init in ("build", "given"))
    assert all(c in kc.EXACT_CASES for c in exact)

    def run_matrix(ctx, keep=None):
        out = {}
        for c in exact:
            init = "build" if c.init == "build" else kc.given_medoids(c)
            _put(out, c.id, cluster.kmedoids(kc.case_matrix(c), c.k, init=init, max_swaps=c.max_swaps, ctx=ctx))
        return out

    def check_matrix(out):
        """tests/test_gpu_kmedoids.py assert_is_ref"""
        for c in exact:
            got, ref = _get(out, c.id, distance.KMedoids), kc.case_ref(c)
            for f in ("medoids", "swaps", "td", "labels", "dist", "second"):
                assert np.array_equal(getattr(got, f), getattr(ref, f)), (c.id, f)
            assert (got.stop, got.passes) == (ref.stop, ref.passes), c.id

    yield Case("kmedoids_matrix257", "medoids", ("cluster.kmedoids",), "kmedoids_cases.kmedoids_ref, as arrays", run_matrix,
               check_matrix, lambda: [kc.case_ref(c) for c in exact], {"DVS_KMEDOIDS_BATCH": "3"})

    def run_mode(ctx, mode, keep=None):
        side = _mode_side(ctx, mode)
        out = {"distances": side.distances()}
        _put(out, "fused", side.kmedoids(7))
        _put(out, "route", cluster.kmedoids(out["distances"], 7, ctx=ctx))
        _put(out, "maxmin", side.kmedoids(17, init="maxmin"))
        _done(keep, side)
        return out

    def check_mode(out, mode):
        """tests/test_gpu_kmedoids.py test_brca1_fused_equals_the_matrix_route"""
        fused = _get(out, "fused", distance.KMedoids)
        assert all(same_bits(a, b) for a, b in zip(fused, _get(out, "route", distance.KMedoids))), mode
        for got in (fused, _get(out, "maxmin", distance.KMedoids)):
            assert got.stop == 1 and (np.diff(got.td) < 0).all(), mode
            near, dn, ds = kc.state_of(kc.zero_diagonal(out["distances"]), got.medoids)
            assert np.array_equal(got.labels, near) and np.array_equal(got.dist, dn) and np.array_equal(got.second, ds), mode

    yield from _per_mode("kmedoids", "medoids", (("kmedoids", "maxmin", "distances"), ("cluster.kmedoids",)),
                         "kmedoids_cases.state_of over the mode's own matrix", run_mode, check_mode,
                         lambda mode: kc.kmedoids_ref(_mode_ref(mode), 7), {})


def spanning_cases():
    import mst_cases as mc

    env = {"DVS_CROSS_STRIP_ROWS": "64"}  # five strips of the 257 rows, the last of one row
    given = (("euclid", "none"), ("euclid", "given"), ("hamming", "none"), ("nan_blocks", "none"))

    def tree_out(out, name, got):
        out[name + "_edges"], out[name + "_weights"] = got.edges, got.weights
        out[name + "_rounds"] = np.array([got.n, got.n_rounds])

    def tree_check(out, name, want, n=N):
        """tests/test_gpu_mst.py assert_tree"""
        edges, weights, rounds = want
        assert np.array_equal(out[name + "_edges"], edges) and same_bits(out[name + "_weights"], weights), name
        assert out[name + "_rounds"].tolist() == [n, rounds], name

    def run_matrix(ctx, keep=None):
        out = {}
        for family, core in given:
            tree_out(out, f"{family}_{core}", cluster.minimum_spanning_tree(
                mc.FAMILIES[family](N), core=mc.core_of(N) if core == "given" else None, ctx=ctx))
        return out

    def check_matrix(out):
        for family, core in given:
            tree_check(out, f"{family}_{core}", mc.expected(family, N, core))

    yield Case("mst_matrix257", "spanning", ("cluster.minimum_spanning_tree",), "mst_cases.boruvka", run_matrix, check_matrix,
               lambda: [mc.expected(family, N, core) for family, core in given], env)

    def run_mode(ctx, mode, keep=None):
        side = _mode_side(ctx, mode)
        out = {"distances": side.distances()}
        tree_out(out, "plain", side.mst())
        tree_out(out, "m5", side.mst(min_samples=5))  # (the core distances: `nearest` over the same rows)
        tree_out(out, "rows", side.mst(Q_ROWS))
        _done(keep, side)
        return out

    def check_mode(out, mode):
        """tests/test_gpu_mst.py test_modes_against_their_own_distances"""
        d = out["distances"]
        tree_check(out, "plain", mc.boruvka(d))
        tree_check(out, "m5", mc.boruvka(d, mc.kth_smallest(d, 5)))
        tree_check(out, "rows", mc.boruvka(d[np.ix_(Q_ROWS, Q_ROWS)]), Q_ROWS.size)

    yield from _per_mode("mst", "spanning", (("mst", "nearest", "distances"), ()), "mst_cases.boruvka over the mode's own matrix",
                         run_mode, check_mode, lambda mode: mc.boruvka(_mode_ref(mode)), env)


PERMUTATIONS = 40  # with the observed labels 41 vectors: two batches of 16 and one of 9


def group_cases():
    import permanova_cases as pc

    exact = pc.Case("integer", N, 6, PERMUTATIONS, 4242)

    def run_matrix(ctx, keep=None):
        out = {}
        _put(out, "exact", cluster.permanova(pc.case_matrix(exact), pc.case_labels(exact).tolist(), permutations=exact.P,
                                             seed=exact.seed + 2, ctx=ctx))
        return out

    def check_matrix(out):
        """tests/test_gpu_permanova.py test_exact_families_as_arrays, through the Python layer"""
        got, ref = _get(out, "exact", distance.PERMANOVA), pc.case_ref(exact)
        assert got.ss_total == ref.ss_total and got.ss_within == ref.ss_within[0] and np.array_equal(got.group_ss, ref.group_ss)
        assert same_bits(np.float64(got.f), ref.f[0]) and same_bits(np.float64(got.r2), np.float64(ref.r2))
        assert same_bits(got.perm_f, ref.f[1:]) and got.p_value == ref.p_value and got.permutations == exact.P
        assert np.array_equal(got.group_sizes, np.bincount(pc.case_labels(exact)))

    yield Case("permanova_matrix257", "groups", ("cluster.permanova",), "permanova_cases.permanova_ref, as arrays", run_matrix,
               check_matrix, lambda: pc.case_ref(exact), {})

    def run_mode(ctx, mode, keep=None):
        side = _mode_side(ctx, mode)
        out = {"distances": side.distances()}
        _put(out, "fused", side.permanova(labels257(), permutations=PERMUTATIONS, seed=5))
        _put(out, "route", cluster.permanova(out["distances"], labels257(), permutations=PERMUTATIONS, seed=5, ctx=ctx))
        _done(keep, side)
        return out

    def labels_and_perms():
        lab = pc.encode(labels257().tolist())
        return lab, pc.documented_permutations(lab, PERMUTATIONS, 5)

    def check_mode(out, mode):
        """the fused route is the matrix route bit for bit; the sums within permanova_cases.band of the long-double
        truth over the mode's own matrix (tests/test_gpu_permanova.py test_real_valued_input_within_the_band)"""
        lab, perms = labels_and_perms()
        d, got = out["distances"], _get(out, "fused", distance.PERMANOVA)
        assert all(same_bits(np.asarray(a), np.asarray(b)) for a, b in zip(got, _get(out, "route", distance.PERMANOVA))), mode
        t_total, t_within, t_group = pc.sums(d, lab, 6, perms, np.longdouble)
        band = pc.band(N)
        assert abs(np.longdouble(got.ss_total) - t_total) <= band * t_total, mode
        assert abs(np.longdouble(got.ss_within) - t_within[0]) <= band * t_within[0], mode
        assert (np.abs(got.group_ss.astype(np.longdouble) - t_group) <= band * t_group).all(), mode
        assert got.p_value == pc.permanova_ref(d, lab, 6, perms).p_value and got.perm_f.size == PERMUTATIONS, mode

    yield from _per_mode("permanova", "groups", (("permanova", "distances"), ("cluster.permanova",)),
                         "permanova_cases.sums in long double over the mode's own matrix", run_mode, check_mode,
                         lambda mode: pc.permanova_ref(_mode_ref(mode), *(lambda lp: (lp[0], 6, lp[1]))(labels_and_perms())), {})


def all_cases() -> dict:
    cases = {}
    for gen in (distance_cases, tree_cases, cophenet_cluster_cases, maxmin_cases, sketch_cases, histogram_cases, ingest_cases,
                selection_cases, neighbour_cases, canonical_cases, ordination_cases, medoid_cases, spanning_cases, group_cases):
        for c in gen():
            assert c.name not in cases and c.family in FAMILIES
            cases[c.name] = c
    return cases


CASES = all_cases()


def cases_of(family: str) -> list:
    return [name for name, c in CASES.items() if c.family == family]


# ------------------------------------------------------------------ the error cases

def error_cases() -> dict:
    bad = random257().copy()
    bad[3, 100] = np.nan
    negative = symmetric257() - 0.5
    empties = list(two_empty_sketches())

    def mash_side(ctx):
        return distance.device_side(empties, "mash", 12, 400, 4, False, ctx=ctx)

    def with_side(ctx, f):
        with mash_side(ctx) as side:
            return f(side)

    def bad_seeds(ctx):
        import torch

        seqs = list(select_seqs(0))
        for r in range(SELECT_SHAPES[0][3]):
            seqs[r] = np.full(40, 4, dtype=np.uint8)  # no seed row has a valid k-mer
        data, offs = oracle.concat(seqs)
        t = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to("cuda:0")
        torch.cuda.synchronize()
        m = ctx.build_matrix_device(t.data_ptr(), offs, SELECT_SHAPES[0][2], 4)
        try:
            m.nmost(SELECT_SHAPES[0][3])
        finally:
            m.close()
            ctx.sync()

    def setup_side(ctx):
        mash_side(ctx).close()

    def setup_bad_seeds(ctx):
        import torch

        seqs = list(select_seqs(0))
        for r in range(SELECT_SHAPES[0][3]):
            seqs[r] = np.full(40, 4, dtype=np.uint8)
        data, offs = oracle.concat(seqs)
        t = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to("cuda:0")
        torch.cuda.synchronize()
        ctx.build_matrix_device(t.data_ptr(), offs, SELECT_SHAPES[0][2], 4).close()
        ctx.sync()

    def setup_delta_jsd(ctx):
        m = ctx.build_matrix(list(select_seqs(0)), 3, 4)
        q = ctx.build_matrix(list(query_seqs(0)), 4, 4)
        sel = m.nmost(10)
        for h in (sel, q, m):
            h.close()

    def host_bad_seeds():
        seqs = list(select_seqs(0))
        for r in range(SELECT_SHAPES[0][3]):
            seqs[r] = np.full(40, 4, dtype=np.uint8)
        oracle.nmost(seqs, SELECT_SHAPES[0][3], SELECT_SHAPES[0][2], 4)

    def refused_delta_jsd(ctx):
        m = ctx.build_matrix(list(select_seqs(0)), 3, 4)
        q = ctx.build_matrix(list(query_seqs(0)), 4, 4)  # 256 bins against the set's 64
        sel = m.nmost(10)
        try:
            sel.delta_jsd(q)
        finally:
            for h in (sel, q, m):
                h.close()

    def host_mash():
        """the oracle states the reference's ZeroDivisionError (diverse_seq/distance.py:283) as NaN: its value is returned"""
        sk = [expected_sketch(q, 12, 400, 4, False) for q in (empties[3], empties[40])]
        assert sk[0].size == sk[1].size == 0
        return oracle.mash_distance(sk[0], sk[1], 12, 400)

    def host_scipy(d, method):
        def run():
            from scipy.cluster.hierarchy import linkage as scipy_linkage

            scipy_linkage(np.asarray(d)[np.triu_indices(N, 1)], method)
        return run

    cases = [
        ErrorCase("linkage_non_finite", "trees", lambda ctx: cluster.linkage(bad, "average", ctx=ctx), ValueError,
                  "linkage_random257", host_scipy(bad, "average")),
        ErrorCase("nj_non_finite", "trees", lambda ctx: cluster.neighbor_joining(bad, ctx=ctx), ValueError, "nj_matrices257", None),
        ErrorCase("ward_negative", "trees", lambda ctx: cluster.linkage(negative, "ward", ctx=ctx), ValueError,
                  "linkage_random257", None),
        ErrorCase("mash_distances_two_empty", "distances", lambda ctx: with_side(ctx, lambda s: s.distances()), ZeroDivisionError,
                  "distances_mash", host_mash, setup_side),
        ErrorCase("mash_cluster_scores_two_empty", "cophenet_clusters",
                  lambda ctx: with_side(ctx, lambda s: s.cluster_scores(labels257())), ZeroDivisionError, "scores_modes257", host_mash,
                  setup_side),
        ErrorCase("mash_maxmin_two_empty", "maxmin", lambda ctx: with_side(ctx, lambda s: s.maxmin(N, seeds=(3,))), ZeroDivisionError,
                  "maxmin_mash", host_mash, setup_side),
        ErrorCase("bad_seeds_behind_resident_build", "selections", bad_seeds, ValueError, "select0_resident", host_bad_seeds,
                  setup_bad_seeds),
        ErrorCase("delta_jsd_bins_mismatch", "selections", refused_delta_jsd, ValueError, "select0_nmost", None, setup_delta_jsd),
    ]
    return {e.name: e for e in cases}


ERROR_CASES = error_cases()


# ------------------------------------------------------------------ the schedules of tests/test_gpu_mixed_workload.py

def schedule_orders() -> dict:
    """(a) three orders of all cases"""
    names = list(CASES)
    shuffled = [names[i] for i in np.random.default_rng(20_260).permutation(len(names))]
    return {"ascending": names, "reversed": names[::-1], "shuffled": shuffled}


def schedule_kept_handles():
    """(b) the shuffle with every handle kept: [("run", case) | ("close", how many of the oldest-but-shuffled handles) |
    ("drop_context",)]: handles are closed in a seeded order, in three batches, the last one after the owner of the
    context has dropped it"""
    steps = [("run", name) for name in schedule_orders()["shuffled"]]
    third = len(steps) // 3
    steps.insert(2 * third, ("close", 0.5))     # half of what is open, picked by the seed
    steps.insert(third, ("close", 0.5))
    return steps + [("drop_context",), ("close", 1.0)]


def schedule_with_errors() -> list:
    """(c) the shuffle with every error case directly in front of its follower"""
    steps = []
    for name in schedule_orders()["shuffled"]:
        steps += [("error", e.name) for e in ERROR_CASES.values() if e.follower == name]
        steps.append(("run", name))
    return steps


def largest_block() -> int:
    """the largest single block any case asks the cache for: the 97 x 65 536 x 4-byte count rows of k = 8"""
    return (97 * 65536 * 4 + 4095) & ~4095


# ------------------------------------------------------------------ what must be named by a case

# every public method of the two classes, sorted by whether it enqueues GPU work
ENQUEUES = {
    "Context": ("build_matrix", "build_matrix_concat", "build_matrix_device", "pack_device", "pack_host", "build_matrix_packed",
                "encode_fasta", "encode_genbank", "matrix_from_freqs", "matrix_from_device_freqs", "kmer_counts"),
    "Selection": ("members", "gather_members", "bench_scan", "delta_jsd", "member_rows", "assign", "diversify"),
}
HOST_ONLY = {
    "Context": ("close", "check", "sync", "refresh_knobs", "set_timing", "device_info", "block_stats"),
    "Selection": ("close", "summary", "global_ids"),
}


# the operations of a DeviceSide (the written list), which defines every one of them itself; every one serves every mode
DEVICE_SIDE_OPS = ("distances", "linkage", "nj", "cross_distances", "nearest", "cluster_scores", "cophenet", "maxmin", "within",
                   "threshold_clusters", "pcoa", "pcoa_project", "kmedoids", "mst", "permanova")


def device_side_operations() -> set:
    """the public methods of DeviceSide, and of any class it might come to inherit from"""
    return {n for klass in distance.DeviceSide.__mro__ if klass is not object
            for n, v in vars(klass).items() if callable(v) and not n.startswith("_")} - {"close"}


def required_ops() -> set:
    ops = {f"DeviceSide.{op}:{mode}" for op in DEVICE_SIDE_OPS for mode in distance.DeviceSide.MODE_NAMES}
    ops |= {f"{cls}.{m}" for cls, methods in ENQUEUES.items() for m in methods}
    return ops


# ------------------------------------------------------------------ the CPU assertions

def test_the_knob_is_a_word_of_the_test_knobs_variable():
    """one more word of DVS_TEST_KNOBS, beside the others, listed with the tests that use it"""
    import pathlib

    root = pathlib.Path(__file__).resolve().parent.parent
    assert POISON in (root / "diverseseq_amd" / "csrc" / "api.cpp").read_text()
    table = [line for line in (root / "INTEGRATION.md").read_text().splitlines() if "DVS_TEST_KNOBS" in line]
    assert any(POISON in line and "test_gpu_poisoned_blocks.py" in line for line in table)


def test_the_refusing_knob_is_a_word_of_the_test_knobs_variable():
    """... and one more: parsed in api.cpp, described where the others are, listed with the test that walks it; the
    runtime's allocation calls stand in api.cpp alone, behind the counted gates"""
    import pathlib
    import re

    root = pathlib.Path(__file__).resolve().parent.parent
    csrc = root / "diverseseq_amd" / "csrc"
    assert f'"{REFUSE}"' in (csrc / "api.cpp").read_text() and REFUSE + "<i>" in (csrc / "dvs_internal.h").read_text()
    table = [line for line in (root / "INTEGRATION.md").read_text().splitlines() if "DVS_TEST_KNOBS" in line]
    assert any(REFUSE in line and "test_gpu_refused_blocks.py" in line for line in table)
    assert REFUSE in (root / "DESIGN.md").read_text()
    assert "int dvs_ctx_block_stats(const dvs_ctx *ctx, uint64_t out[4]);" in (root / "include" / "dvs_hip.h").read_text()
    assert "dvs_ctx_block_stats" in _lib.EXPORTS
    calls = re.compile(r"\bhip(Malloc|HostMalloc|MallocAsync|HostAlloc|MallocManaged|ExtMallocWithFlags|MallocPitch)\s*\(")
    found = sorted(f.name for f in csrc.iterdir() if f.suffix in (".hip", ".cpp", ".h") and calls.search(f.read_text()))
    assert found == ["api.cpp"], found


def test_every_public_method_is_sorted_and_every_operation_named():
    for cls in (engine.Context, engine.Selection):
        public = {n for n in vars(cls) if not n.startswith("_")}
        listed = set(ENQUEUES[cls.__name__]) | set(HOST_ONLY[cls.__name__])
        assert public == listed, (cls.__name__, public ^ listed)  # a method added later is sorted here, and gets a case
    named = {op for c in CASES.values() for op in c.ops}
    assert required_ops() <= named, sorted(required_ops() - named)
    own = {n for n, v in vars(distance.DeviceSide).items() if callable(v) and not n.startswith("_")} - {"close"}
    assert len(set(DEVICE_SIDE_OPS)) == len(DEVICE_SIDE_OPS) == 15
    assert own == set(DEVICE_SIDE_OPS), own ^ set(DEVICE_SIDE_OPS)  # (an operation added later is listed here)
    # ... and nowhere but in the class itself, each with a case in every mode
    assert distance.DeviceSide.__bases__ == (object,)
    assert device_side_operations() == own
    assert {f"DeviceSide.{op}:{mode}" for op in device_side_operations() for mode in distance.DeviceSide.MODE_NAMES} <= named


def test_the_table_has_every_family_and_its_shapes():
    assert [f for f in FAMILIES if not cases_of(f)] == []
    assert len(ragged97()) == 97 and ragged97()[0].size == 0 and ragged97()[1].size < 2 and (ragged97()[2] == 4).all()
    assert np.array_equal(ragged97()[3], ragged97()[4]) and (ragged97()[5][[0, -1]] == 4).all()
    assert all(300 <= s.size <= 900 for s in ragged97()[6:]) and ragged97_long()[-1].size == 70_001
    assert len(seqs65()) == 65 and seqs65()[1].size > 2 * MASH_TILE + 12 and seqs65()[0].size < 3
    assert Q_ROWS.size == 65 and R_ROWS.size == 31 and not set(Q_ROWS) & set(R_ROWS)
    raw = ingest_fasta()
    assert 2 * 128 * 1024 < len(raw) < 400_000 and b"\r\n" in raw and not raw.endswith(b"\n")
    labels, seqs = oracle.load_fasta(raw)
    assert len(labels) == 782 and sum(s.size == 0 for s in seqs) >= 2
    assert all(CASES[e.follower].family == e.family for e in ERROR_CASES.values())
    assert {e.family for e in ERROR_CASES.values()} == {"trees", "distances", "cophenet_clusters", "maxmin", "selections"}


@pytest.mark.parametrize("name", list(CASES))
def test_reference_can_be_computed_here(name):
    CASES[name].ref()


@pytest.mark.parametrize("name", [n for n, e in ERROR_CASES.items() if e.host])
def test_error_cases_raise_from_the_references_side(name):
    """... or, for 0 / 0 between two empty sketches, give the NaN by which the oracle states the reference's
    ZeroDivisionError (oracle.mash_distance)"""
    err = ERROR_CASES[name]
    if err.raises is ZeroDivisionError:
        assert np.isnan(err.host())
        return
    with pytest.raises(err.raises):
        err.host()


def test_schedules_are_valid():
    orders = schedule_orders()
    assert all(sorted(o) == sorted(CASES) for o in orders.values())
    assert orders["shuffled"] not in (orders["ascending"], orders["reversed"])
    runs = [name for o in orders.values() for name in o]
    kept = schedule_kept_handles()
    runs += [s[1] for s in kept if s[0] == "run"]
    assert [s[0] for s in kept].count("close") == 3 and kept[-2:] == [("drop_context",), ("close", 1.0)]
    mixed = schedule_with_errors()
    runs += [s[1] for s in mixed if s[0] == "run"]
    for i, step in enumerate(mixed):  # every failing call is followed directly by a case that asks for the same sizes
        if step[0] == "error":
            behind = next(s for s in mixed[i + 1:] if s[0] == "run")
            assert behind[1] == ERROR_CASES[step[1]].follower
    assert all(runs.count(name) >= 2 for name in CASES)
    assert sorted(s[1] for s in mixed if s[0] == "error") == sorted(ERROR_CASES)
    assert largest_block() >= N * N * 8
