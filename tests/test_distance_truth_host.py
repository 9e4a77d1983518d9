"""The yardstick of tests/test_gpu_distance_truth.py, pinned on the CPU before it is used on the device.

The distance stage over count rows (csrc/rowdist.hip) is compared cell by cell with the definitions evaluated in
80-bit long double, not with the oracle: the oracle is itself an f64 evaluation and "within X of the oracle" cannot be
sharper than the oracle is.  This module holds

  * `truth_jsd` / `truth_jsd_rows`: H((f_i + f_j) / 2) - (H(f_i) + H(f_j)) / 2 in np.longdouble (f = c / t in long
    double, np.sum over the non-zero bins), pinned against mpmath at 50 digits;
  * `truth_euclid` / `truth_euclid_rows`: ||f_i - f_j||_2 in long double from the f64 quotients RN(c / t), which both
    the reference (diverse_seq/distance.py:294-336) and the kernel start from;
  * `tol_derived(B)`, the bound a correct f64 evaluation over B bins keeps against the truth (below);
  * `distance_cases()`: the cases the GPU module runs, and `oracle_errors(case)`: the oracle's own worst error against
    the truth on a seeded sample of each case's pairs, which the GPU module's second gate is measured against.

tol_derived(B) = (B + 8) 2^-52 max(1, log2 B).  Each of the three entropies is B accumulations into a partial sum of at
most log2 B (bits), every accumulation rounds once, by at most 2^-53 of the partial sum; the per-term logarithm adds
about one ulp of the result (csrc/select_dev.h); the three entropies combine as 1 - 1/2 - 1/2, and a handful of
roundings finish the cell."""
import functools
import math
import zlib
from typing import NamedTuple

import numpy as np
import pytest

import oracle
from test_gpu_linkage import family_seqs
from test_jsd_host import pair_jsd

LD = np.longdouble
if not np.finfo(LD).eps < 1e-18:
    pytest.skip(f"np.longdouble is no 80-bit long double here (eps = {np.finfo(LD).eps}): no yardstick sharper than "
                "the f64 evaluations under test", allow_module_level=True)

SAMPLE = 2000          # pairs of a case the oracle is compared on
CROSS_FAMILY = 20_000  # family1000: seeded pairs from different families, beside all 9 500 within a family
EUCLID_RTOL = 1e-12    # the project's bound for a euclidean cell (tests/test_gpu_sketch.py test_euclidean_all_pairs)


def tol_derived(nbins: int) -> float:
    """the bound of a correct f64 evaluation of a JSD cell over `nbins` bins against the truth (module docstring)"""
    return (nbins + 8) * 2.0 ** -52 * max(1.0, math.log2(nbins))


def gate2_floor(nbins: int) -> float:
    """a few ulps of an entropy: what the second gate never asks less than"""
    return 8 * 2.0 ** -52 * max(1.0, math.log2(nbins))


# --------------------------------------------------------------------------------------------- the truth
def _freqs_ld(rows) -> np.ndarray:
    """count rows (an integer dtype) -> c / t in long double, a row of total 0 -> zeros; frequency rows as they are"""
    rows = np.asarray(rows)
    if rows.dtype.kind in "ui":
        c = rows.astype(LD)
        t = c.sum(axis=-1, keepdims=True)
        return np.divide(c, t, out=np.zeros_like(c), where=t > 0)
    return rows.astype(LD)


def _entropy_ld(f: np.ndarray) -> np.ndarray:
    """-sum f log2 f over the non-zero bins of the last axis, in long double"""
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(f > 0, f * np.log2(f), LD(0))
    return -np.sum(terms, axis=-1)


def truth_jsd_rows(F, pairs) -> np.ndarray:
    """the long-double JSD of the rows F[i], F[j] (counts of an integer dtype, or f64 frequencies) for every (i, j) of
    `pairs` [m, 2] -> np.longdouble [m]"""
    f = _freqs_ld(F)
    h = _entropy_ld(f)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(len(pairs), dtype=LD)
    step = max(1, (1 << 20) // f.shape[1])
    for a in range(0, len(pairs), step):
        i, j = pairs[a:a + step, 0], pairs[a:a + step, 1]
        out[a:a + step] = _entropy_ld((f[i] + f[j]) / 2) - (h[i] + h[j]) / 2
    return out


def truth_jsd(row_i, row_j):
    """H((f_i + f_j) / 2) - (H(f_i) + H(f_j)) / 2 of two count rows or two frequency rows, in long double"""
    return truth_jsd_rows(np.stack([np.asarray(row_i), np.asarray(row_j)]), [(0, 1)])[0]


def f64_quotients(rows) -> np.ndarray:
    """RN(c / t) of count rows (src/record.rs:139; NaN for a row of total 0); frequency rows as they are"""
    rows = np.asarray(rows)
    if rows.dtype.kind in "ui":
        c = rows.astype(np.float64)  # (exact: a count is below 2^32)
        with np.errstate(invalid="ignore"):
            return c / c.sum(axis=-1, keepdims=True)
    return rows.astype(np.float64)


def truth_euclid_rows(F, pairs) -> np.ndarray:
    """||f_i - f_j||_2 in long double over the f64 quotients of the rows"""
    q = f64_quotients(F).astype(LD)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(len(pairs), dtype=LD)
    step = max(1, (1 << 20) // q.shape[1])
    for a in range(0, len(pairs), step):
        d = q[pairs[a:a + step, 0]] - q[pairs[a:a + step, 1]]
        out[a:a + step] = np.sqrt(np.sum(d * d, axis=-1))
    return out


def truth_euclid(row_i, row_j):
    return truth_euclid_rows(np.stack([np.asarray(row_i), np.asarray(row_j)]), [(0, 1)])[0]


# --------------------------------------------------------------------------------------------- the cases
class Case(NamedTuple):
    name: str
    seqs: object     # list of uint8 sequences, or None for a case of frequency rows
    freqs: object    # float64 [n, bins] for matrix_from_freqs, or None
    num_states: int  # (0 for frequency rows)
    k: int
    empty: tuple     # indices of the rows without a valid k-mer

    @property
    def nbins(self):
        return self.freqs.shape[1] if self.seqs is None else self.num_states ** self.k

    @property
    def nrows(self):
        return len(self.freqs) if self.seqs is None else len(self.seqs)


def _seed(name: str) -> int:
    return zlib.crc32(name.encode())


def _random_seq(rng, n, num_states=4):
    return rng.integers(0, num_states, size=n, dtype=np.uint8)


def _composed_seq(rng, n):
    """a sequence with its own base composition, as tests/gpu_synth.py draws them"""
    cuts = np.minimum(255, np.cumsum(rng.dirichlet([4.0] * 4))[:3] * 256).astype(np.uint8)
    x = rng.integers(0, 256, size=n, dtype=np.uint8)
    return ((x >= cuts[0]).astype(np.uint8) + (x >= cuts[1]) + (x >= cuts[2])).astype(np.uint8)


def _bins_seq_case(num_states, k):
    """12 ragged rows, row 0 with 5 % invalid symbols; at k = 1 row 11 is row 3 twice over: counts in proportion"""
    name = f"bins_s{num_states}_k{k}"
    rng = np.random.default_rng(_seed(name))
    seqs = [_random_seq(rng, int(rng.integers(200, 3000)), num_states) for _ in range(12)]
    seqs[0][rng.random(seqs[0].size) < 0.05] = num_states
    if k == 1:
        seqs[11] = np.concatenate([seqs[3], seqs[3]])
    return Case(name, seqs, None, num_states, k, ())


def _normalised(v):
    """v / sum(v), again where the sequential sum over the non-zero bins is not yet within bins * eps of 1 (the check
    of matrix_from_freqs, src/record.rs:90-104)"""
    f = v / v.sum()
    for _ in range(3):
        s = np.add.accumulate(f[f != 0])[-1]
        if abs(s - 1.0) <= 0.5 * f.size * np.finfo(np.float64).eps:
            break
        f = f / s
    return f


def _bins_freq_case(nbins):
    """12 normalised random vectors, the odd ones 90 % zeros"""
    name = f"bins_freqs_b{nbins}"
    rng = np.random.default_rng(_seed(name))
    rows = []
    for r in range(12):
        v = rng.random(nbins)
        if r % 2:
            v[rng.permutation(nbins)[:int(0.9 * nbins)]] = 0.0
        rows.append(_normalised(v))
    return Case(name, None, np.stack(rows), 0, 0, ())


def _tiles_case():
    """100 random 1 kb rows at k = 4: four tile rows, the last one partial; rows without a valid k-mer on both sides
    of the first tile edge and at the end; copies of row 5 in the third and the fourth tile row"""
    rng = np.random.default_rng(_seed("tiles"))
    seqs = [_random_seq(rng, 1000) for _ in range(100)]
    seqs[31], seqs[32], seqs[99] = np.full(40, 4, np.uint8), _random_seq(rng, 3), np.full(1000, 4, np.uint8)
    seqs[70], seqs[98] = seqs[5].copy(), seqs[5].copy()
    return Case("tiles", seqs, None, 4, 4, (31, 32, 99))


@functools.lru_cache(maxsize=None)
def _totals_seqs(k):
    rng = np.random.default_rng(_seed("totals"))
    seqs = [_composed_seq(rng, 3_000_000) for _ in range(6)]          # totals of 3e6, counts beyond 2^16
    seqs += [_random_seq(rng, 300) for _ in range(2)]                 # beside rows of 300 bp
    seqs += [_random_seq(rng, k), _random_seq(rng, k + 1)]            # totals 1 and 2
    seqs.append(np.full(70_000, 2, np.uint8))                         # a single count of about 70 000
    seqs.append(np.full(500, 4, np.uint8))                            # no valid k-mer
    return seqs


def _substituted(rng, root, nsub):
    s = root.copy()
    at = rng.choice(root.size, size=nsub, replace=False)
    s[at] = (s[at] + rng.integers(1, 4, size=nsub, dtype=np.uint8)) % 4  # (another base, always)
    return s


@functools.lru_cache(maxsize=None)
def _near_seqs(length):
    """a root; its copies with 1, 3, 30 substitutions (the same total); its copy with one base deleted (total - 1)"""
    rng = np.random.default_rng(_seed(f"near{length}"))
    root = _random_seq(rng, length)
    out = [root] + [_substituted(rng, root, n) for n in (1, 3, 30)]
    out.append(np.delete(root, int(rng.integers(length))))
    return out


@functools.lru_cache(maxsize=None)
def _family(nfam):
    return list(family_seqs(nfam, 20, 20_000, seed=11).values())


def _freq_rows_case(k):
    """the 35 rows of test_jsd_of_frequency_rows, and three rows at the edges of the kernel's arithmetic"""
    name = f"freq_rows_k{k}"
    rng = np.random.default_rng(8)
    seqs = [_random_seq(rng, int(rng.integers(300, 2500))) for _ in range(35)]
    f = np.stack([oracle.to_kfreqs(s, 4, k)[0] for s in seqs])
    extra = np.zeros((3, f.shape[1]))
    extra[0, 5] = 1.0                                  # 1.0 in one bin
    extra[1, 2], extra[1, 9] = 1.0, 5e-324             # a subnormal entry
    extra[2, 7], extra[2, 11] = 1.0, 2.0 ** -1001      # below the kernel's clamp of the logarithm's argument
    return Case(name, None, np.vstack([f, extra]), 0, 0, ())


BINS_STATES_K = ((2, 1), (3, 1), (4, 1), (5, 2), (20, 1), (4, 3), (3, 4), (5, 3), (2, 7), (20, 2), (20, 3), (4, 6), (4, 7),
                 (4, 8), (5, 7))  # (the last two: rows beyond 16 384 bins, tests/test_wide_rows_host.py)
BINS_FREQS = (1, 63, 64, 65, 127, 129, 4097)


@functools.lru_cache(maxsize=None)
def distance_cases():
    cases = [_bins_seq_case(s, k) for s, k in BINS_STATES_K]
    cases += [_bins_freq_case(b) for b in BINS_FREQS]
    cases.append(_tiles_case())
    cases += [Case(f"totals_k{k}", _totals_seqs(k), None, 4, k, (11,)) for k in (3, 6, 7)]
    cases += [Case(f"near_{length // 1000}kb_k{k}", _near_seqs(length), None, 4, k, ())
              for length, ks in ((5_000, (5, 6)), (20_000, (5, 6)), (3_000_000, (3, 5, 6))) for k in ks]
    cases.append(Case("family320", _family(16), None, 4, 5, ()))
    cases.append(Case("family1000", _family(50), None, 4, 5, ()))
    cases += [_freq_rows_case(k) for k in (2, 6)]
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


_rows, _cells, _errors = {}, {}, {}


def case_rows(case) -> np.ndarray:
    """the rows of a case as the truth takes them: uint64 counts by the oracle, or the f64 frequency rows"""
    if case.name not in _rows:
        _rows[case.name] = case.freqs if case.seqs is None else \
            np.stack([oracle.count_kmers(s, case.num_states, case.k) for s in case.seqs])
    return _rows[case.name]


def case_pairs(case) -> np.ndarray:
    """the pairs (i > j) of valid rows a case is compared on: all of them, but for family1000 every pair within a
    family and CROSS_FAMILY seeded pairs between families"""
    n = case.nrows
    if case.name == "family1000":
        i, j = np.tril_indices(20, -1)
        within = np.concatenate([np.stack([i, j], axis=1) + 20 * f for f in range(n // 20)])
        rng = np.random.default_rng(_seed(case.name))
        cross = set()
        while len(cross) < CROSS_FAMILY:
            a, b = (int(x) for x in rng.integers(0, n, size=2))
            if a // 20 != b // 20:
                cross.add((max(a, b), min(a, b)))
        return np.concatenate([within, np.array(sorted(cross))])
    i, j = np.tril_indices(n, -1)
    keep = ~np.isin(i, case.empty) & ~np.isin(j, case.empty)
    return np.stack([i[keep], j[keep]], axis=1)


def case_truth(case):
    """(pairs [m, 2], long-double JSD [m], long-double euclidean distance [m]) of a case, computed once per session"""
    if case.name not in _cells:
        pairs, rows = case_pairs(case), case_rows(case)
        _cells[case.name] = (pairs, truth_jsd_rows(rows, pairs), truth_euclid_rows(rows, pairs))
    return _cells[case.name]


def sample_of(case) -> np.ndarray:
    """indices into case_pairs(case) of the seeded sample the oracle is compared on"""
    m = len(case_pairs(case))
    if m <= SAMPLE:
        return np.arange(m)
    return np.sort(np.random.default_rng(_seed(case.name) + 1).choice(m, size=SAMPLE, replace=False))


def oracle_cell(row_i, row_j) -> float:
    """the oracle's JSD of two rows of any alphabet: test_jsd_host.pair_jsd over RN(c / t) and the oracle's entropies"""
    fi, fj = f64_quotients(row_i), f64_quotients(row_j)
    return pair_jsd(fi, oracle.entropy(fi), fj, oracle.entropy(fj))


def oracle_errors(case):
    """(E_oracle, worst relative euclidean error) of a case: the oracle against the truth on the case's sample"""
    if case.name not in _errors:
        pairs, tj, te = case_truth(case)
        q = f64_quotients(case_rows(case))
        ents = {}
        ej = er = 0.0
        for s in sample_of(case):
            i, j = (int(x) for x in pairs[s])
            for r in (i, j):
                if r not in ents:
                    ents[r] = oracle.entropy(q[r])
            ej = max(ej, abs(float(LD(pair_jsd(q[i], ents[i], q[j], ents[j])) - tj[s])))
            d = LD(oracle.euclidean_distance(q[i], q[j]))
            er = max(er, float(abs(d - te[s]) / te[s]) if te[s] > 0 else (0.0 if d == 0 else np.inf))
        _errors[case.name] = (ej, er)
    return _errors[case.name]


# --------------------------------------------------------------------------------------------- the tests
_CASES = distance_cases()


def _mp_jsd(ci, cj):
    """the definition at 50 digits from exact rationals (counts) or exact f64 values (frequencies)"""
    import mpmath as mp

    mp.mp.dps = 50
    ci, cj = np.asarray(ci), np.asarray(cj)
    if ci.dtype.kind in "ui":
        ti, tj = mp.mpf(int(ci.sum())), mp.mpf(int(cj.sum()))
        fi, fj = [mp.mpf(int(c)) / ti for c in ci], [mp.mpf(int(c)) / tj for c in cj]
    else:
        fi, fj = [mp.mpf(float(c)) for c in ci], [mp.mpf(float(c)) for c in cj]

    def h(f):
        return -mp.fsum(x * mp.log(x, 2) for x in f if x > 0)

    return h([(a + b) / 2 for a, b in zip(fi, fj)]) - (h(fi) + h(fj)) / 2


def _mp_pairs():
    by = {c.name: c for c in _CASES}
    return [("bins_s4_k1", 1, 0), ("bins_s4_k1", 11, 3), ("bins_s4_k1", 7, 0), ("bins_s5_k2", 4, 2),
            ("bins_s4_k6", 3, 1), ("bins_s4_k7", 5, 0), ("bins_s4_k7", 9, 8), ("near_5kb_k6", 1, 0),
            ("near_5kb_k6", 4, 0), ("near_20kb_k5", 2, 0), ("near_3000kb_k3", 1, 0), ("near_3000kb_k3", 4, 0),
            ("totals_k3", 8, 0), ("totals_k6", 9, 6), ("bins_freqs_b65", 3, 2), ("freq_rows_k2", 37, 36)], by


def test_truth_is_the_definition_at_50_digits():
    """random, near-duplicate and one-deletion pairs, 4 and 16 384 bins, totals 1 and 2 against 3 Mb, frequency rows
    with a subnormal and a 2^-1001 entry: the long-double value is within 1e-17 max(1, log2 B) of mpmath's"""
    mp = pytest.importorskip("mpmath")
    names, by = _mp_pairs()
    for name, i, j in names:
        rows = case_rows(by[name])
        got = truth_jsd(rows[i], rows[j])
        exp = _mp_jsd(rows[i], rows[j])
        diff = abs(mp.mpf(int(np.floor(got * LD(2) ** 80))) / mp.mpf(2) ** 80 - exp)  # (exact: 64 bits below 2^1)
        bound = 1e-17 * max(1.0, math.log2(rows.shape[1]))
        print(f"{name} ({i}, {j}): truth {float(got):.6g}, |long double - mpmath| = {float(diff):.3g} (bound {bound:.3g})")
        assert diff <= bound, (name, i, j)
        assert got == truth_jsd(rows[j], rows[i])


def test_truth_of_simple_rows():
    a, b = np.array([40, 0, 0, 0], np.uint64), np.array([0, 17, 0, 0], np.uint64)
    assert truth_jsd(a, b) == 1 and truth_jsd(a, a) == 0 and truth_jsd(a, 3 * a) == 0
    assert truth_euclid(a, b) == np.sqrt(LD(2)) and truth_euclid(b, 2 * b) == 0
    f = np.array([0.25, 0.75, 0.0]), np.array([0.75, 0.25, 0.0])
    assert abs(float(truth_jsd(*f)) - (1.0 - (-0.25 * math.log2(0.25) - 0.75 * math.log2(0.75)))) < 1e-15
    assert truth_euclid(*f) == np.sqrt(LD(0.5))


def test_tol_derived_is_below_the_old_constant():
    assert all(tol_derived(c.nbins) < 1e-9 for c in _CASES)
    assert abs(tol_derived(16384) - 5.1e-11) < 1e-12 and abs(tol_derived(4096) - 1.1e-11) < 1e-12
    assert abs(tol_derived(4) - 5.3e-15) < 1e-16


def test_case_table_is_complete():
    by = {c.name: c for c in _CASES}
    nb = len(BINS_STATES_K)
    assert [c.nbins for c in _CASES[:nb]] == [2, 3, 4, 25, 20, 64, 81, 125, 128, 400, 8000, 4096, 16384, 65536, 78125]
    assert [c.nbins for c in _CASES[nb:nb + 7]] == list(BINS_FREQS)
    for c in _CASES:
        rows = case_rows(c)
        assert rows.shape == (c.nrows, c.nbins)
        if c.seqs is not None:  # the rows without a valid k-mer are the ones the case names
            assert tuple(np.flatnonzero(rows.sum(axis=1) == 0)) == c.empty, c.name
        else:                   # matrix_from_freqs takes every row (src/record.rs:90-104)
            for f in rows:
                assert abs(np.add.accumulate(f[f != 0])[-1] - 1.0) <= f.size * np.finfo(np.float64).eps, c.name
    for c in _CASES[:nb]:
        assert c.nrows == 12 and len({s.size for s in c.seqs}) > 6 and (c.seqs[0] == c.num_states).any()
        if c.k == 1:  # counts in proportion, quotients that round alike
            rows = case_rows(c)
            assert (rows[11] == 2 * rows[3]).all() and (f64_quotients(rows[11]) == f64_quotients(rows[3])).all()
    for c in _CASES[nb:nb + 7]:
        assert ((c.freqs == 0).sum(axis=1) == int(0.9 * c.nbins))[1::2].all() and (c.freqs[0::2] > 0).all()
    assert by["tiles"].nrows == 100
    for k in (3, 6, 7):
        t = case_rows(by[f"totals_k{k}"]).sum(axis=1)
        assert (t[:6] > 2_999_000).all() and (t[6:8] < 300).all() and tuple(t[8:]) == (1, 2, 70_001 - k, 0)
        assert case_rows(by[f"totals_k{k}"]).max() > 2 ** 16
    for name, length in (("near_5kb_k5", 5_000), ("near_20kb_k6", 20_000), ("near_3000kb_k3", 3_000_000)):
        t = case_rows(by[name]).sum(axis=1)
        assert tuple(t) == (length - by[name].k + 1,) * 4 + (length - by[name].k,)
        assert [int((a != by[name].seqs[0]).sum()) for a in by[name].seqs[1:4]] == [1, 3, 30]
    assert float(case_truth(by["near_3000kb_k3"])[1].min()) < 1e-10  # (cells of 1e-11 are among them)
    assert by["family320"].nrows == 320 and by["family1000"].nrows == 1000
    pairs = case_pairs(by["family1000"])
    assert len(pairs) == 9_500 + CROSS_FAMILY == len({(int(a), int(b)) for a, b in pairs})
    assert (pairs[:, 0] > pairs[:, 1]).all()
    assert (pairs[:9_500, 0] // 20 == pairs[:9_500, 1] // 20).all()
    q = f64_quotients(case_rows(by["family320"]))
    assert (q[23] == q[37]).all() and 23 // 32 != 37 // 32  # (exact duplicates in different tile rows)
    f = by["freq_rows_k6"].freqs
    assert f.shape == (38, 4096) and f[35].max() == 1.0 and 0 < f[36, 9] < 2.3e-308 and f[37, 11] == 2.0 ** -1001


@pytest.mark.parametrize("case", _CASES, ids=lambda c: c.name)
def test_oracle_is_within_the_derived_bound_of_the_truth(case):
    """every sampled oracle cell is within tol_derived(B) of the long-double JSD, and the oracle's euclidean distance
    within 1e-12 relative of the long-double one; the worst difference is E_oracle[case] of the GPU module"""
    e_jsd, e_euclid = oracle_errors(case)
    tol = tol_derived(case.nbins)
    print(f"{case.name}: B = {case.nbins}, {len(sample_of(case))} pairs, E_oracle = {e_jsd:.3g}, "
          f"oracle / tol_derived = {e_jsd / tol:.3g}, euclidean worst relative error = {e_euclid:.3g}")
    assert e_jsd <= tol
    assert e_euclid <= EUCLID_RTOL
