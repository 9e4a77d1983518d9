"""The yardstick and the cases of the Mantel tests (test_mantel_host.py pins them on the CPU, test_gpu_mantel.py holds the
device to them).

`sums` restates include/dvs_hip.h "Mantel" in numpy: only the cells above the diagonal of either matrix, y(a, b) =
Y[min(a, b)][max(a, b)]; the shifts s = fl(S / m); u = fl(x - s_x), v = fl(y - s_y) in float64; A, B, S_uu, S_vv and, per
permutation, Z(pi) = sum_{i<j} u_ij v(pi[i], pi[j]) -- summed in float64, or in np.longdouble (`dtype`), the truth the
device is held to.  The shifts may be handed in (`shifts`): the header's band is stated over the u and v, so the truth of
a device run is formed over the device's own shifts.  The device adds the same terms in the order the header states, the
float64 yardstick in numpy's; both are at most two levels of sums of at most n terms, so both lie within BAND(n) = (n +
8) 2^-52 of the truth, relative to the sum of the terms' magnitudes, and for the EXACT families they are the same doubles.
`statistics` derives r, the three counts and p.

Two kinds of families.  EXACT: the counted cells of each matrix are c + e_k with c an integer and the e small integers (|e|
<= 2^8) in balanced +- pairs (one 0 when m is odd), shuffled by a seed -- so S = m c, the shift is c, and every u, v,
product and partial sum is exact: any order gives the same doubles and the device must agree as arrays.  The diagonal and
the lower triangle hold NaN: they are never read.  REAL: real-valued cells in three spreads, seeded so that no permuted Z
lies within 2 BAND(n) sqrt(S_uu S_vv) of Z(id) or of its mirror about c0 unless it is the same arrangement, which makes
the counts and p unique."""
import functools
from typing import NamedTuple

import numpy as np

# the bounds of csrc/mantel.hip: a wave; the chunk of a row the entry and centre kernels take at a time (64 lanes x 4 in
# flight); the scoring kernel's threads, which is also the alignment of its first column, and its chunk (256 threads x 4
# in flight); the final kernel's threads, one strided chain of rows each
WAVE, ROW_CHUNK, SCORE_THREADS, SCORE_CHUNK, FINAL_THREADS = 64, 256, 256, 1024, 256
DEFAULT_BATCH, MAX_BATCH = 32, 32
BATCHES = (1, 3, 16, 32, None)  # DVS_MANTEL_BATCH; None: the default
ALTERNATIVES = ("two-sided", "greater", "less")

SIZES = (3, 4, 63, 64, 65, 257, 513, 1025, 2049)
BOUND_SIZES = (255, 256, 1023, 1024)  # (64 | 65, 256 | 257 and 1024 | 1025 straddle with SIZES)
PERMS = (0, 1, DEFAULT_BATCH - 1, DEFAULT_BATCH, DEFAULT_BATCH + 1, 3 * DEFAULT_BATCH + 5)
LARGE = 2049          # from this size on a case has LARGE_PERMS permutations: the yardstick costs n^2 a permutation
LARGE_PERMS = 3
SUB_FAMILIES = ("plain", "ties", "same", "negated", "constant", "identity", "automorph", "stratified")


def band(n: int) -> float:
    """what a float64 sum of the header's order may be off by, relative to the sum of its terms' magnitudes"""
    return (n + 8) * 2.0 ** -52


def pairs_of(n: int) -> int:
    return n * (n - 1) // 2


# ------------------------------------------------------------------ the rule of the permutations, restated

def documented_permutations(n: int, permutations: int, seed, strata=None) -> np.ndarray:
    """mantel.permutations's rule, restated: one rng.permutation(n) per row, drawn in order; the row is perm, or with
    strata the positions of every block receive the block's items in ascending order of perm"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(permutations):
        perm = rng.permutation(n)
        if strata is None:
            rows.append(perm)
            continue
        row = np.zeros(n, dtype=np.int64)
        for s in np.unique(strata):
            idx = np.flatnonzero(np.asarray(strata) == s)
            row[idx] = idx[np.argsort(perm[idx], kind="stable")]
        rows.append(row)
    return np.array(rows, dtype=np.uint32).reshape(permutations, n)


# ------------------------------------------------------------------ the yardstick

class Sums(NamedTuple):
    s_x: float
    s_y: float
    A: object
    B: object
    S_uu: object
    S_vv: object
    z: np.ndarray  # [P + 1], [0] the observed

    @property
    def moments(self) -> np.ndarray:
        return np.array([self.s_x, self.s_y, self.A, self.B, self.S_uu, self.S_vv], dtype=np.float64)


def upper_cells(M) -> np.ndarray:
    """the counted cells, row by row, float64"""
    M = np.asarray(M, dtype=np.float64)
    return M[np.triu_indices(M.shape[0], 1)]


def symmetric_from_upper(M) -> np.ndarray:
    """y(a, b) for a != b as a full matrix, 0 on the diagonal, from the cells above the diagonal alone"""
    M = np.asarray(M, dtype=np.float64)
    up = np.zeros(M.shape)
    iu = np.triu_indices(M.shape[0], 1)
    up[iu] = M[iu]
    return up + up.T


def sums(X, Y, perms, dtype=np.float64, shifts=None) -> Sums:
    """the header's sums in `dtype`; u, v and the shifts are float64 whatever the dtype"""
    n = np.asarray(X).shape[0]
    m = pairs_of(n)
    iu = np.triu_indices(n, 1)
    x, ysym = upper_cells(X), symmetric_from_upper(Y)
    if shifts is None:
        s_x = np.float64(x.astype(dtype).sum() / dtype(m))
        s_y = np.float64(ysym[iu].astype(dtype).sum() / dtype(m))
    else:
        s_x, s_y = (np.float64(s) for s in shifts)
    u = (x - s_x).astype(dtype)       # fl(x - s_x), then widened
    V = ysym - s_y                    # fl(y - s_y); the diagonal is never taken
    v = V[iu].astype(dtype)
    rows = [np.arange(n), *np.asarray(perms, dtype=np.int64).reshape(-1, n)]
    z = np.zeros(len(rows), dtype=dtype)
    for p, pi in enumerate(rows):
        z[p] = (u * V[np.ix_(pi, pi)][iu].astype(dtype)).sum()
    return Sums(float(s_x), float(s_y), u.sum(), v.sum(), (u * u).sum(), (v * v).sum(), z)


def magnitudes(X, Y, perms, shifts) -> Sums:
    """the sum of the magnitudes of every sum's terms (np.longdouble): what the band is relative to"""
    n = np.asarray(X).shape[0]
    iu = np.triu_indices(n, 1)
    ld = np.longdouble
    s_x, s_y = (np.float64(s) for s in shifts)
    u = np.abs(upper_cells(X) - s_x).astype(ld)
    V = np.abs(symmetric_from_upper(Y) - s_y)
    v = V[iu].astype(ld)
    rows = [np.arange(n), *np.asarray(perms, dtype=np.int64).reshape(-1, n)]
    z = np.array([(u * V[np.ix_(pi, pi)][iu].astype(ld)).sum() for pi in rows], dtype=ld)
    return Sums(float(s_x), float(s_y), u.sum(), v.sum(), (u * u).sum(), (v * v).sum(), z)


class Stats(NamedTuple):
    r: np.ndarray  # float64 [P + 1]
    n_ge: int
    n_le: int
    n_abs_ge: int
    p_value: dict  # alternative -> p; nan for P = 0 or r nan


def correlation(n: int, s: Sums) -> np.ndarray:
    """r of every z from the sums, in np.longdouble, rounded once; nan where either variance factor is <= 0"""
    ld = np.longdouble
    m = ld(pairs_of(n))
    a, b, suu, svv = ld(s.A), ld(s.B), ld(s.S_uu), ld(s.S_vv)
    vx, vy = suu - a * a / m, svv - b * b / m
    if not (vx > 0 and vy > 0):
        return np.full(np.asarray(s.z).shape, np.nan)
    return ((np.asarray(s.z).astype(ld) - a * b / m) / np.sqrt(vx * vy)).astype(np.float64)


def statistics(n: int, s: Sums) -> Stats:
    """r, the counts on z in float64 and p for each alternative, from float64 sums"""
    z = np.asarray(s.z, dtype=np.float64)
    P = z.size - 1
    c0 = np.float64(np.float64(s.A) * np.float64(s.B)) / np.float64(pairs_of(n))
    n_ge, n_le = int((z[1:] >= z[0]).sum()), int((z[1:] <= z[0]).sum())
    n_abs = int((np.abs(z[1:] - c0) >= np.abs(z[0] - c0)).sum())
    r = correlation(n, s)
    counts = dict(zip(ALTERNATIVES, (n_abs, n_ge, n_le)))
    ok = P > 0 and not np.isnan(r[0])
    return Stats(r, n_ge, n_le, n_abs, {alt: (1 + c) / (1 + P) if ok else float("nan") for alt, c in counts.items()})


def pearson_truth(X, Y) -> np.longdouble:
    """Pearson's r of the original counted cells, two-pass, in np.longdouble"""
    ld = np.longdouble
    x, y = upper_cells(X).astype(ld), upper_cells(Y).astype(ld)
    dx, dy = x - x.mean(), y - y.mean()
    return (dx * dy).sum() / np.sqrt((dx * dx).sum() * (dy * dy).sum())


# ------------------------------------------------------------------ the cases

class Case(NamedTuple):
    family: str  # a sub-family of EXACT, or a spread of REAL
    n: int
    P: int
    seed: int

    @property
    def id(self) -> str:
        return f"{self.family}-n{self.n}-P{self.P}"


def balanced(count: int, rng, amp: int) -> np.ndarray:
    """count integers in [-amp, amp] in +- pairs, one 0 when count is odd, shuffled"""
    a = rng.integers(0, amp + 1, count // 2)
    e = np.concatenate([a, -a, np.zeros(count % 2, dtype=a.dtype)])
    rng.shuffle(e)
    return e.astype(np.float64)


def matrix_of(n: int, cells: np.ndarray) -> np.ndarray:
    """the counted cells row by row above the diagonal, NaN on and below it"""
    M = np.full((n, n), np.nan)
    M[np.triu_indices(n, 1)] = cells
    return M


def exact_cases() -> list:
    cases = []

    def add(family, n, P):
        P = P if n < LARGE else LARGE_PERMS
        if not any((c.family, c.n, c.P) == (family, n, P) for c in cases):
            cases.append(Case(family, n, P, 3000 + len(cases)))

    for k, n in enumerate(SIZES + BOUND_SIZES):
        add("plain", n, PERMS[(k + 2) % len(PERMS)])
    for P in PERMS:
        add("plain", 65, P)
        add("plain", 257, P)
    for family in SUB_FAMILIES[1:]:
        add(family, 65, DEFAULT_BATCH + 1)
        add(family, 257, 3 * DEFAULT_BATCH + 5)
    return cases


EXACT_CASES = exact_cases()
REAL_FAMILIES = ("uniform", "points", "crowded")
REAL_CASES = [Case(f, n, P, 9000 + 10 * i + j)
              for i, f in enumerate(REAL_FAMILIES) for j, (n, P) in enumerate(((40, 99), (300, 3 * DEFAULT_BATCH + 5),
                                                                              (1025, DEFAULT_BATCH + 1)))]
CX, CY = 1000.0, 777.0  # the integer the EXACT cells of X and of Y sit around


def is_exact(case: Case) -> bool:
    return case.family in SUB_FAMILIES


@functools.lru_cache(maxsize=8)
def case_matrices(case: Case) -> tuple:
    """(X, Y), read-only"""
    rng = np.random.default_rng(case.seed)
    n, m = case.n, pairs_of(case.n)
    if is_exact(case):
        amp = 1 if case.family == "ties" else 256
        ex = balanced(m, rng, amp)
        ey = balanced(m, rng, amp)
        if case.family == "same":
            ey = ex
        elif case.family == "negated":
            ey = -ex
        elif case.family == "constant":
            ey = np.zeros(m)
        elif case.family == "automorph":  # items 0 and 1 are twins in Y: y(0, k) == y(1, k) for k >= 2
            E = np.zeros((n, n))
            twin = balanced(n - 2, rng, amp)
            E[0, 2:], E[1, 2:] = twin, twin
            E[0, 1] = 0.0
            rest = np.triu_indices(n - 2, 1)
            E[rest[0] + 2, rest[1] + 2] = balanced(pairs_of(n - 2), rng, amp)
            ey = E[np.triu_indices(n, 1)]
        X, Y = matrix_of(n, CX + ex), matrix_of(n, (CX if case.family in ("same", "negated") else CY) + ey)
    elif case.family == "uniform":
        a = rng.random(m)
        X, Y = matrix_of(n, a), matrix_of(n, 0.6 * a + 0.4 * rng.random(m))
    elif case.family == "points":  # euclidean distances of points, and of the same points moved a little
        pts = rng.normal(size=(n, 4))
        moved = pts + 0.7 * rng.normal(size=(n, 4))
        iu = np.triu_indices(n, 1)
        X = matrix_of(n, np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))[iu])
        Y = matrix_of(n, np.sqrt(((moved[:, None] - moved[None]) ** 2).sum(-1))[iu])
    else:  # crowded: every cell within 1e-3 of 1, relatively
        a = rng.random(m)
        X, Y = matrix_of(n, 1.0 + 1e-3 * a), matrix_of(n, 1.0 + 1e-3 * (0.5 * a + 0.5 * rng.random(m)))
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


def case_strata(case: Case):
    return np.arange(case.n) % 4 if case.family == "stratified" else None


def case_perms(case: Case) -> np.ndarray:
    """uint32 [P, n]"""
    perms = documented_permutations(case.n, case.P, case.seed + 2, case_strata(case))
    if case.family == "identity" and case.P:  # the identity at several places of the batches
        for at in (0, DEFAULT_BATCH - 2, DEFAULT_BATCH - 1, DEFAULT_BATCH, case.P - 1):
            if at < case.P:
                perms[at] = np.arange(case.n)
    if case.family == "automorph" and case.P > 2:  # the twins exchanged: Y is mapped onto itself
        swap = np.arange(case.n, dtype=np.uint32)
        swap[[0, 1]] = [1, 0]
        perms[2] = swap
    return perms


@functools.lru_cache(maxsize=None)
def case_sums(case: Case) -> Sums:
    """the float64 yardstick"""
    return sums(*case_matrices(case), case_perms(case))


@functools.lru_cache(maxsize=None)
def case_stats(case: Case) -> Stats:
    return statistics(case.n, case_sums(case))
