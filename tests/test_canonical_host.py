"""Canonical (strand-folded) k-mer count rows without a GPU: the yardstick, the cases that
tests/test_gpu_canonical.py runs, and the argument errors of the Python layer.

The yardstick is a numpy fold, by the definition of include/dvs_hip.h "canonical k-mer count rows", of
`oracle.count_kmers`; the reverse complement of a k-mer comes from `oracle.reverse_complement` ((base + 2) % 4,
src/distance.rs:18).  Nothing of the code under test is used by it:
  * `yardstick_bins(k)`: the representatives min(idx, rc(idx)) in ascending order, and rc of each;
  * `fold_counts(counts, k)`: out[c] = in[rep_c] + in[rc(rep_c)], a palindrome counted once;
  * `folded(seqs, k)`: (counts uint32 [n, C(k)], totals uint32 [n], `oracle.entropy` of counts / total, 0.0 for a row
    of total 0);
  * `revcomp(seq)`: a sequence's reverse complement, an invalid byte staying where the reversal puts it."""
import functools

import numpy as np
import pytest

import oracle
from diverseseq_amd import _dvs, apps, cluster, distance, engine

C_OF_K = (2, 10, 32, 136, 512, 2080, 8192, 32896)  # C(k), k = 1 .. 8 (include/dvs_hip.h "canonical k-mer count rows")
N_ROWS = (1, 63, 64, 65, 257)
ENTROPY_TOL = 1e-11   # the build's own bound against oracle.entropy (tests/test_gpu_parity.py TIGHT)
SELECT_RTOL = 1e-6    # selections against the oracle: the existing parity rule
LONG_BASES = 40_000   # more than 32 768 windows: 32-bit count rows whatever the switches say


# --------------------------------------------------------------------------------------------- the yardstick
def canonical_count(k: int) -> int:
    return 4 ** k // 2 if k % 2 else (4 ** k + 4 ** (k // 2)) // 2


@functools.lru_cache(maxsize=None)
def yardstick_bins(k: int):
    """(reps uint32 [C(k)] ascending, partner uint32 [C(k)] = rc(rep)): every k-mer index as k digits, first base most
    significant (src/record.rs:18-29), reverse-complemented by the oracle in one call (the reverse complement of the
    concatenation lists the k-mers' reverse complements in reverse order)"""
    idx = np.arange(4 ** k, dtype=np.int64)
    weights = 4 ** np.arange(k - 1, -1, -1, dtype=np.int64)
    digits = ((idx[:, None] // weights) % 4).astype(np.uint8)
    rc_digits = oracle.reverse_complement(digits.reshape(-1)).reshape(-1, k)[::-1]
    rc = (rc_digits.astype(np.int64) * weights).sum(axis=1)
    keep = idx <= rc
    reps, partner = idx[keep].astype(np.uint32), rc[keep].astype(np.uint32)
    reps.setflags(write=False)
    partner.setflags(write=False)
    return reps, partner


def fold_counts(counts, k: int) -> np.ndarray:
    """the last axis of `counts` (4^k plain bins) folded onto the canonical bins"""
    reps, partner = yardstick_bins(k)
    counts = np.asarray(counts)
    return counts[..., reps] + np.where(partner != reps, counts[..., partner], 0)


def revcomp(seq) -> np.ndarray:
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    out = oracle.reverse_complement(seq) if seq.size else seq.copy()
    back = seq[::-1]
    out[back >= 4] = back[back >= 4]
    return out


def plain_counts(seqs, k: int) -> np.ndarray:
    return np.stack([oracle.count_kmers(s, 4, k) for s in seqs]).astype(np.uint32).reshape(len(seqs), 4 ** k)


def folded_of_counts(counts, k: int):
    f = fold_counts(counts, k).astype(np.uint32)
    totals = f.sum(axis=1, dtype=np.uint64).astype(np.uint32)
    ent = np.array([oracle.entropy(row / np.float64(t)) if t else 0.0 for row, t in zip(f.astype(np.float64), totals)])
    return f, totals, ent


def folded(seqs, k: int):
    return folded_of_counts(plain_counts(seqs, k), k)


def folded_freqs(seqs, k: int) -> np.ndarray:
    """the yardstick's frequency rows (every row must have a valid k-mer): what the oracle's selections take"""
    f, totals, _ = folded(seqs, k)
    assert (totals > 0).all()
    return f.astype(np.float64) / totals.astype(np.float64)[:, None]


# --------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def ragged(n: int, seed: int = 0) -> tuple:
    """n sequences of 40-400 bases with invalid bytes inside; from 5 rows on, rows without a valid k-mer (k >= 2) first,
    inside and last: a single base, all gaps, empty"""
    rng = np.random.default_rng(1000 * n + seed)
    seqs = []
    for _ in range(n):
        s = rng.integers(0, 4, size=int(rng.integers(40, 401)), dtype=np.uint8)
        s[rng.random(s.size) < 0.01] = 4
        seqs.append(s)
    if n >= 5:
        seqs[0] = seqs[0][:1].copy()
        seqs[n // 2] = np.full(50, 4, dtype=np.uint8)
        seqs[-1] = np.zeros(0, dtype=np.uint8)
    return tuple(seqs)


@functools.lru_cache(maxsize=None)
def with_a_long_row() -> tuple:
    """five short sequences around one of 40 000 bases, which takes more than one histogram tile"""
    rng = np.random.default_rng(LONG_BASES)
    long_row = rng.integers(0, 4, size=LONG_BASES, dtype=np.uint8)
    long_row[rng.integers(0, LONG_BASES, size=30)] = 4
    return ragged(6, 1)[:3] + (long_row,) + ragged(6, 1)[3:]


@functools.lru_cache(maxsize=None)
def many_rows(n: int, length: int) -> tuple:
    """more rows than the fold's grid has row groups (eight workgroups a CU, four rows a group for rows of 1 KiB and
    less): workgroups then take a second group"""
    rng = np.random.default_rng(n + length)
    return tuple(rng.integers(0, 4, size=length, dtype=np.uint8) for _ in range(n))


MANY_ROWS = ((8300, 24, 2), (2200, 60, 5))  # (rows, bases, k): a wave per row; a workgroup per row


def strand_subset(n: int, seed: int = 5) -> np.ndarray:
    """which of n sequences are reverse-complemented in the strand-invariance case: about half, seeded"""
    return np.random.default_rng(seed).random(n) < 0.5


@functools.lru_cache(maxsize=None)
def family200() -> tuple:
    """200 sequences of 400 bases from 8 mutated families (1-8 % substitutions, a few gaps), every second one
    reverse-complemented, in a seeded shuffle: what a strand-dependent selection mistakes for diversity"""
    rng = np.random.default_rng(200)
    seqs = []
    for _ in range(8):
        root = rng.integers(0, 4, 400, dtype=np.uint8)
        for _ in range(25):
            s = root.copy()
            hit = rng.random(400) < rng.uniform(0.01, 0.08)
            s[hit] = rng.integers(0, 4, int(hit.sum()), dtype=np.uint8)
            s[rng.random(400) < 0.002] = 4
            seqs.append(s)
    seqs = [seqs[i] for i in rng.permutation(200)]
    return tuple(revcomp(s) if i % 2 else s for i, s in enumerate(seqs))


@functools.lru_cache(maxsize=None)
def family_queries() -> tuple:
    """six queries for delta_jsd: members of the set's families in either strand, and two unrelated sequences"""
    rng = np.random.default_rng(6)
    fam = family200()
    return (fam[3], revcomp(fam[3]), revcomp(fam[10]), fam[77][:300].copy(),
            rng.integers(0, 4, 350, dtype=np.uint8), rng.integers(0, 4, 90, dtype=np.uint8))


SELECT_KS = (4, 6)


@functools.lru_cache(maxsize=None)
def family_reference(k: int, what: str):
    rows = folded_freqs(list(family200()), k)
    if what == "nmost":
        return oracle.final_nmost(rows, 10)
    return oracle.final_max(rows, 5, 30, what)


# --------------------------------------------------------------------------------------------- the CPU assertions
@pytest.mark.parametrize("k", range(1, 9))
def test_canonical_bins(k):
    reps, partner = yardstick_bins(k)
    assert reps.size == canonical_count(k) == C_OF_K[k - 1]
    assert (np.diff(reps.astype(np.int64)) > 0).all() and (reps <= partner).all()
    assert int((reps == partner).sum()) == (0 if k % 2 else 4 ** (k // 2))  # palindromes: even k only
    # every plain bin lies in exactly one canonical bin
    assert np.array_equal(np.sort(np.concatenate([reps, partner[partner != reps]])), np.arange(4 ** k))
    got = engine.canonical_bins(k)
    assert got.dtype == np.uint32 and np.array_equal(got, reps)


def test_canonical_bins_refuses_other_k():
    for k in (0, 17, 40):
        with pytest.raises(ValueError, match="canonical bins are defined for k in 1..16"):
            engine.canonical_bins(k)


def test_rc_is_the_digit_rule():
    """T0 C1 A2 G3: the complement is d ^ 2; index 0b00_01_10 = TCA -> TGA = 0b00_11_10"""
    reps, partner = yardstick_bins(3)
    at = {int(r): int(p) for r, p in zip(reps, partner)}
    assert at[0b000110] == 0b001110 and at[0] == 0b101010  # TTT -> AAA
    assert np.array_equal(revcomp(np.array([0, 1, 4, 2, 3], np.uint8)), [1, 0, 4, 3, 2])


@pytest.mark.parametrize("k", range(1, 8))
def test_yardstick_fold_is_strand_invariant(k):
    rng = np.random.default_rng(k)
    differ = 0
    for _ in range(20):
        s = rng.integers(0, 4, size=int(rng.integers(k, 300)), dtype=np.uint8)
        s[rng.random(s.size) < 0.03] = 4
        a, b = oracle.count_kmers(s, 4, k), oracle.count_kmers(revcomp(s), 4, k)
        assert np.array_equal(fold_counts(a, k), fold_counts(b, k))
        assert a.sum() == b.sum() == fold_counts(a, k).sum()
        differ += int(not np.array_equal(a, b))
    assert differ >= 15  # (the plain counts do tell the strands apart)


def test_cases_are_what_the_gpu_file_needs():
    for n in N_ROWS:
        seqs = ragged(n)
        assert len(seqs) == n and max(s.size for s in seqs) <= 400
        if n >= 5:
            _, totals, ent = folded(list(seqs), 2)
            empty = np.flatnonzero(totals == 0).tolist()
            assert empty == [0, n // 2, n - 1] and (ent[empty] == 0).all()
        assert any((s >= 4).any() for s in seqs)
    long_case = with_a_long_row()
    assert len(long_case) == 7 and long_case[3].size == LONG_BASES and LONG_BASES - 6 + 1 > 32768
    for n, length, k in MANY_ROWS:
        assert n > 256 * 8 * (4 if 4 ** k * 4 <= 1024 else 1) and len(many_rows(n, length)) == n
    fam = family200()
    assert len(fam) == 200 and all(s.size == 400 for s in fam)
    assert 60 <= int(strand_subset(257).sum()) <= 200


@pytest.mark.parametrize("k", SELECT_KS)
def test_oracle_selects_over_the_yardsticks_rows(k):
    """the oracle's merges take the folded frequency rows (their sum-to-one check holds) and the fold matters: about
    half of what the plain selection finds on this input is strand"""
    sr = family_reference(k, "nmost")
    assert sr.size == 10 and 0 < sr.total_jsd < np.log2(10)
    plain = oracle.nmost(list(family200()), 10, k, 4)
    # (k = 4: 0.308 folded against 0.551 plain; at k = 6 rows of 400 bases are sparse and differ in most bins anyway)
    assert sr.total_jsd < (0.75 if k == 4 else 1.0) * plain.total_jsd
    for stat in ("stdev", "cov"):
        assert 5 <= family_reference(k, stat).size <= 30
    rows = folded_freqs(list(family_queries()), k)
    assert all(np.isfinite(sr.delta_jsd(r)) for r in rows)


# --------------------------------------------------------------------------------------------- argument errors
MASH = "Canonical count rows should only be specified for the jsd and euclidean distances"
PROTEIN = "Canonical kmers only supported for"
_SEQS = [np.array([0, 1, 2, 3, 0, 1], np.uint8), np.array([3, 3, 2, 1, 0, 0], np.uint8), np.array([1, 1, 2, 0, 3, 2], np.uint8)]
_NAMED = {f"s{i}": s for i, s in enumerate(_SEQS)}


@pytest.mark.parametrize("call", [
    lambda: distance.check_mode_args("mash", 100, False, True),
    lambda: distance.device_side(_SEQS, "mash", 3, 100, 4, False, canonical=True),
    lambda: distance.cross_distances(_SEQS, _SEQS, "mash", k=3, sketch_size=100, canonical=True),
    lambda: distance.nearest(_SEQS, _SEQS, 1, "mash", k=3, sketch_size=100, canonical=True),
    lambda: distance.cluster_scores(_SEQS, [0, 0, 1], "mash", k=3, sketch_size=100, canonical=True),
    lambda: distance.cophenet(_SEQS, np.array([[0, 1, .1, 2], [2, 3, .2, 3]]), "mash", k=3, sketch_size=100, canonical=True),
    lambda: distance.maxmin(_SEQS, 2, "mash", k=3, sketch_size=100, canonical=True),
    lambda: cluster.ctree(_NAMED, k=3, sketch_size=100, canonical=True),
    lambda: cluster.nj_tree(_NAMED, k=3, sketch_size=100, canonical=True),
    lambda: cluster.ctree_clusters(_NAMED, n_clusters=2, k=3, sketch_size=100, canonical=True),
    lambda: cluster.ctree_cophenet(_NAMED, k=3, sketch_size=100, canonical=True),
    lambda: cluster.compare_linkages(_NAMED, k=3, sketch_size=100, canonical=True),
    lambda: apps.dvs_ctree(canonical=True),
    lambda: apps.dvs_dist("mash", canonical=True),
    lambda: apps.dvs_maxmin(n=2, canonical=True),
])
def test_mash_refuses_canonical_count_rows(call):
    with pytest.raises(ValueError, match=MASH):
        call()


@pytest.mark.parametrize("call", [
    lambda: apps.dvs_nmost(moltype="protein", canonical=True),
    lambda: apps.dvs_max(moltype="protein", canonical=True),
    lambda: apps.dvs_delta_jsd({"a": "ACDE"}, moltype="protein", canonical=True),
    lambda: apps.dvs_ctree(distance_mode="jsd", sketch_size=None, moltype="protein", canonical=True),
    lambda: apps.dvs_dist("euclidean", sketch_size=None, moltype="protein", canonical=True),
])
def test_other_moltypes_refuse_canonical(call):
    with pytest.raises(ValueError, match=PROTEIN):
        call()


def test_other_alphabets_refuse_canonical_before_any_device_work():
    store = _dvs.make_zarr_store()
    for name, s in _NAMED.items():
        store.write(name, s.tobytes())
    with pytest.raises(ValueError, match="four-state"):
        _dvs.nmost_divergent(store, n=2, k=2, num_states=20, canonical=True)
    with pytest.raises(ValueError, match="four-state"):
        _dvs.max_divergent(store, min_size=2, max_size=3, k=2, num_states=20, canonical=True)
    with pytest.raises(ValueError, match="four-state"):
        _dvs.get_delta_jsd_calculator(list(_NAMED.items()), 2, 20, canonical=True)


def _result(canonical: bool):
    r = _dvs.SummedRecordsResult()
    bins = 10 if canonical else 16
    r.records = [(f"{'c' if canonical else 'p'}{i}", [1.0 / bins] * bins, 0.1) for i in range(3)]
    r.size, r.k, r.num_states, r.canonical = 3, 2, 4, canonical
    return r


def test_results_of_mixed_flag_do_not_merge():
    with pytest.raises(ValueError, match="canonical k-mers with results over plain k-mers"):
        _dvs.final_nmost([_result(True), _result(False)], n=2)
    with pytest.raises(ValueError, match="canonical k-mers with results over plain k-mers"):
        _dvs.final_max([_result(False), _result(True)], min_size=2, max_size=4)


def test_result_remembers_the_flag():
    import pickle

    assert _dvs.SummedRecordsResult().canonical is False
    assert pickle.loads(pickle.dumps(_result(True))).canonical is True
    plain = _result(False)
    assert "canonical" not in plain.__getstate__() and pickle.loads(pickle.dumps(plain)).canonical is False


def test_defaults_and_positions_are_kept():
    """`canonical` comes last and defaults to False everywhere it was added"""
    import inspect

    fns = [engine.Context.build_matrix, engine.Context.build_matrix_concat, engine.Context.build_matrix_device,
           engine.Context.build_matrix_packed, engine.SeqBatch.build_matrix, _dvs.nmost_divergent, _dvs.max_divergent,
           _dvs.get_delta_jsd_calculator, distance.device_side, distance.jsd_distances, distance.euclidean_distances,
           distance.jsd_linkage, distance.euclidean_linkage, distance.jsd_nj, distance.euclidean_nj,
           distance.cross_distances, distance.nearest, distance.cluster_scores, distance.cophenet, distance.maxmin,
           cluster.ctree, cluster.nj_tree, cluster.ctree_clusters, cluster.ctree_cophenet, cluster.compare_linkages,
           apps.dvs_nmost.__init__, apps.dvs_max.__init__, apps.dvs_delta_jsd.__init__, apps.dvs_ctree.__init__,
           apps.dvs_dist.__init__]
    for fn in fns:
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "canonical" and params[-1].default is False, fn
    assert list(inspect.signature(_dvs.nmost_divergent).parameters)[:5] == ["store", "n", "k", "num_states", "seqids"]
