"""The yardstick and the cases of the PERMANOVA tests (test_permanova_host.py pins them on the CPU, test_gpu_permanova.py
holds the device to them).

`sums` restates include/dvs_hip.h "PERMANOVA" in numpy: q_ij = D[i][j]^2 for i < j only, C_j = the q_ij of column j's
own group above the diagonal added in ascending i, SS_W = sum_j w[g_j] C_j with w[g] = 1.0 / n_g rounded once, SS_T =
(sum_{i<j} q_ij) / n, a group's own term w[g] * (its R_i in ascending i) -- in float64, or in np.longdouble (`dtype`), the
truth the device is held to.  The device adds the same terms in the tile order the header states; the float64 yardstick
adds them column by column.  Both are two levels of sums of at most n terms, so both lie within BAND(n) = (n + 8) 2^-52 of
the truth, relatively, and for the EXACT families they are the same doubles.  `statistics` derives SS_A, F, R^2 and p.

Two kinds of families.  EXACT: every entry a small integer and every group size a power of two (mixed, ones among
them), so that every q, every w, every product and every partial sum is exact: any order of summation gives the same
doubles and the device must agree as arrays.  REAL: real-valued entries, seeded so that no permutation's SS_W lies within
twice the band of the observed one unless it makes the same partition, which makes n_le and p unique."""
import functools
from typing import NamedTuple

import numpy as np

# the bounds of csrc/permanova.hip: a tile's rows and columns, a wave, the rows in flight, the entry kernel's chunk of a
# row, and the tiles the final kernel's 256 threads take one each (ceil(n / 256) * ceil(n / 128) tiles: 242 at 2816,
# 276 at 2817)
TILE_ROWS, TILE_COLS, WAVE, UNROLL, ENTRY_CHUNK, FINAL_THREADS = 128, 256, 64, 8, 512, 256
DEFAULT_BATCH, MAX_BATCH = 16, 32
MAX_GROUPS = 65535
BATCHES = (1, 3, 16, None)  # DVS_PERMANOVA_BATCH; None: the default

SIZES = (3, 4, 63, 64, 65, 257, 1025, 2049)
BOUND_SIZES = (8, 9, 127, 128, 129, 255, 256, 511, 512, 513, 2816, 2817)  # (64 | 65 and 256 | 257 are in SIZES)
GROUPS = (2, 3, 16, 255, 256, 257, "n-1")
PERMS = (0, 1, DEFAULT_BATCH - 1, DEFAULT_BATCH, DEFAULT_BATCH + 1, 3 * DEFAULT_BATCH + 5)
LARGE = 2049          # from this size on a case has LARGE_PERMS permutations: the yardstick costs n^2 a label vector
LARGE_PERMS = 3


def band(n: int) -> float:
    """what a float64 sum of the header's order may be off by, relative to the sum of its (non-negative) terms"""
    return (n + 8) * 2.0 ** -52


# ------------------------------------------------------------------ the rule of the permutations, restated

def encode(grouping) -> np.ndarray:
    """hashables -> codes 0 .. a - 1 in the order of first appearance"""
    codes = {}
    return np.array([codes.setdefault(g, len(codes)) for g in grouping], dtype=np.uint32)


def documented_permutations(labels, permutations: int, seed, strata=None) -> np.ndarray:
    """distance.permuted_labels's rule, restated: one rng.permutation(n) per row, drawn in order; labels[perm], or with
    strata the labels of every block's positions re-dealt inside the block in ascending order of perm"""
    labels = np.asarray(labels, dtype=np.uint32)
    n = labels.size
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(permutations):
        perm = rng.permutation(n)
        if strata is None:
            rows.append(labels[perm])
            continue
        row = np.zeros(n, dtype=np.uint32)
        for s in np.unique(strata):
            idx = np.flatnonzero(np.asarray(strata) == s)
            row[idx] = labels[idx[np.argsort(perm[idx], kind="stable")]]
        rows.append(row)
    return np.array(rows, dtype=np.uint32).reshape(permutations, n)


# ------------------------------------------------------------------ the yardstick

class Ref(NamedTuple):
    ss_total: float
    ss_within: np.ndarray  # [P + 1], [0] the observed labels'
    group_ss: np.ndarray   # [a]
    n_le: int
    f: np.ndarray          # [P + 1]
    r2: float
    p_value: float


def upper_squares(D, dtype=np.float64) -> np.ndarray:
    """q_ij for i < j, zero on and below the diagonal (whatever stands there)"""
    D = np.asarray(D)
    q = np.zeros(D.shape, dtype=dtype)
    iu = np.triu_indices(D.shape[0], 1)
    d = D[iu].astype(dtype)
    q[iu] = d * d
    return q


def group_sums(q: np.ndarray, labels: np.ndarray, a: int):
    """(C, R): C_j = sum_{i<j, g_i = g_j} q_ij in ascending i, R_i = sum_{j>i, g_j = g_i} q_ij in ascending j (q:
    upper_squares), group by group"""
    C, R = np.zeros(q.shape[0], dtype=q.dtype), np.zeros(q.shape[0], dtype=q.dtype)
    order = np.argsort(labels, kind="stable")
    bounds = np.searchsorted(labels[order], np.arange(a + 1))
    for g in range(a):
        idx = order[bounds[g]:bounds[g + 1]]  # ascending
        sub = q[np.ix_(idx, idx)]
        down, along = np.zeros(idx.size, dtype=q.dtype), np.zeros(idx.size, dtype=q.dtype)
        for r in range(idx.size):  # (one row, one column at a time: ascending, whatever numpy's own reduction would do)
            down += sub[r]
            along += sub[:, r]
        C[idx], R[idx] = down, along
    return C, R


def chain(terms, dt):
    acc = dt(0.0)
    for t in terms:
        acc += t
    return acc


def sums(D, labels, a: int, perm_labels, dtype=np.float64):
    """(SS_T, SS_W [P + 1], group_ss [a]) in `dtype`"""
    labels = np.asarray(labels, dtype=np.int64)
    q = upper_squares(D, dtype)
    n = q.shape[0]
    dt = q.dtype.type
    w = dt(1.0) / np.bincount(labels, minlength=a).astype(dtype)  # (the same under every permutation)
    ss_total = chain(q.sum(axis=1), dt) / dt(n)  # (T_i in numpy's own order: within the band, exact for the exact families)
    ss_within = np.zeros(np.asarray(perm_labels).reshape(-1, n).shape[0] + 1, dtype=dtype)
    for p, v in enumerate([labels, *np.asarray(perm_labels).reshape(-1, n)]):
        v = np.asarray(v, dtype=np.int64)
        ss_within[p] = chain(w[v] * group_sums(q, v, a)[0], dt)
    R = group_sums(q, labels, a)[1]
    group_ss = np.zeros(a, dtype=dtype)
    for i in range(n):
        group_ss[labels[i]] += R[i]
    return ss_total, ss_within, group_ss * w


def statistics(n: int, a: int, ss_total, ss_within):
    """(SS_A, F, R^2) per label vector, float64: x / 0 = inf, 0 / 0 = nan, nan wherever SS_T == 0"""
    ssw = np.asarray(ss_within, dtype=np.float64)
    sst = np.float64(ss_total)
    with np.errstate(divide="ignore", invalid="ignore"):
        ssa = sst - ssw
        f = (ssa / np.float64(a - 1)) / (ssw / np.float64(n - a))
        if sst == 0:
            f = np.full(ssw.shape, np.nan)
        r2 = ssa / sst
    return ssa, f, r2


def permanova_ref(D, labels, a: int, perm_labels) -> Ref:
    n = np.asarray(D).shape[0]
    ss_total, ss_within, group_ss = sums(D, labels, a, perm_labels)
    P = ss_within.size - 1
    n_le = int((ss_within[1:] <= ss_within[0]).sum())
    _, f, r2 = statistics(n, a, ss_total, ss_within)
    return Ref(float(ss_total), ss_within, group_ss, n_le, f, float(r2[0]), (1 + n_le) / (1 + P) if P else float("nan"))


# ------------------------------------------------------------------ the cases

class Case(NamedTuple):
    family: str
    n: int
    a: int
    P: int
    seed: int

    @property
    def id(self) -> str:
        return f"{self.family}-n{self.n}-a{self.a}-P{self.P}"


def groups_of(n: int, a) -> int:
    return n - 1 if a == "n-1" else int(a)


def power_of_two_sizes(n: int, a: int):
    """a powers of two that add up to n (None when n has more than a ones in binary, or a > n): the binary digits of n,
    the largest part halved until there are a of them"""
    parts = [1 << b for b in range(n.bit_length()) if n >> b & 1]
    if len(parts) > a or a > n:
        return None
    while len(parts) < a:
        parts.sort()
        big = parts.pop()
        parts += [big // 2, big // 2]
    return sorted(parts, reverse=True)


def exact_labels(n: int, a: int, seed: int) -> np.ndarray:
    """a labelling with power-of-two group sizes, dealt at random, the groups numbered in the order of first appearance"""
    sizes = power_of_two_sizes(n, a)
    lab = np.repeat(np.arange(a), sizes)
    return encode(np.random.default_rng(seed).permutation(lab).tolist())


def exact_cases() -> list:
    """every size with group counts and permutation counts dealt round-robin from those that fit it (a power-of-two
    labelling exists, 2 <= a < n), then every group count at n = 1025 and every permutation count at n = 65 and 257"""
    cases, seen = [], set()

    def add(n, a, P):
        a = groups_of(n, a)
        if not 2 <= a < n or power_of_two_sizes(n, a) is None or (n, a, P) in seen:
            return
        seen.add((n, a, P))
        cases.append(Case("integer", n, a, P if n < LARGE else min(P, LARGE_PERMS), 1000 + len(cases)))

    for k, n in enumerate(SIZES + BOUND_SIZES):
        fits = [a for a in GROUPS if 2 <= groups_of(n, a) < n and power_of_two_sizes(n, groups_of(n, a))]
        for r in range(2):
            add(n, fits[(k + r * 3) % len(fits)], PERMS[(k + r * 2 + 2) % len(PERMS)])
    for a in GROUPS:
        add(1025, a, DEFAULT_BATCH + 1)
        add(300, a, 3)
    for P in PERMS:
        add(65, 3, P)
        add(257, 16, P)
    return cases


EXACT_CASES = exact_cases()
REAL_FAMILIES = ("uniform", "grouped", "crowded")
REAL_CASES = [Case(f, n, a, P, 7000 + 10 * i + j)
              for i, f in enumerate(REAL_FAMILIES) for j, (n, a, P) in enumerate(((40, 3, 99), (300, 7, 3 * DEFAULT_BATCH + 5),
                                                                                 (1025, 300, DEFAULT_BATCH + 1)))]


@functools.lru_cache(maxsize=4)
def case_matrix(case: Case) -> np.ndarray:
    rng = np.random.default_rng(case.seed)
    n = case.n
    if case.family == "integer":  # small integers; the lower triangle other integers: it is never read
        d = rng.integers(0, 8, (n, n)).astype(np.float64)
    elif case.family == "uniform":
        u = np.triu(rng.random((n, n)), 1)
        d = u + u.T
    else:  # points whose groups sit apart ("grouped": clearly; "crowded": barely), euclidean distances
        lab = case_labels(case).astype(np.int64)
        centres = rng.normal(size=(case.a, 5)) * (3.0 if case.family == "grouped" else 0.3)
        x = centres[lab] + rng.normal(size=(n, 5))
        d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    d.setflags(write=False)
    return d


def case_labels(case: Case) -> np.ndarray:
    if case.family == "integer":
        return exact_labels(case.n, case.a, case.seed + 1)
    rng = np.random.default_rng(case.seed + 1)
    lab = np.concatenate([np.arange(case.a), rng.integers(0, case.a, case.n - case.a)])
    return encode(rng.permutation(lab).tolist())


def case_perms(case: Case) -> np.ndarray:
    return documented_permutations(case_labels(case), case.P, case.seed + 2)


@functools.lru_cache(maxsize=None)
def case_ref(case: Case) -> Ref:
    return permanova_ref(case_matrix(case), case_labels(case), case.a, case_perms(case))


@functools.lru_cache(maxsize=None)
def case_truth(case: Case):
    """(SS_T, SS_W [P + 1], group_ss [a]) in np.longdouble"""
    return sums(case_matrix(case), case_labels(case), case.a, case_perms(case), np.longdouble)
