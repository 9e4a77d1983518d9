"""The yardstick and the cases of the k-medoids tests (test_kmedoids_host.py pins them on the CPU, test_gpu_kmedoids.py
holds the device to them).

`kmedoids_ref` restates include/dvs_hip.h "k-medoids" in numpy float64: the state, BUILD, the swap rounds with the
R / C / shared split, the tie rules, the stop rules (the noise level included) and the count of passes.  `delta_truth`
gives every Delta_x[l] in np.longdouble straight from "new nearest distance minus old", without that split.

Two kinds of families.  EXACT: every entry a multiple of 2^-10 below 4, so that every sum of <= 4096 of them (and of
their differences) is exact in any order and the device must agree bit for bit.  GENERAL: real-valued entries, seeded so
that at every round of the yardstick's run the best and the second-best Delta (and, in BUILD, gain) by the long-double
truth differ by more than twice the band a float64 evaluation may be off by, and the best Delta lies further than that
from 0, which makes the exchange sequence and its end unique."""
import functools
from typing import NamedTuple

import numpy as np

SIZES = (2, 3, 5, 63, 64, 65, 257, 1025, 2049)
KS = (1, 2, 3, 7, 64, 65, 1024)
EXACT_FAMILIES = ("random", "clustered", "small_integer", "constant", "zero", "duplicated", "asymmetric")
GENERAL_FAMILIES = ("uniform", "clustered", "crowded")
GENERAL_SIZES = (40, 300)
GENERAL_KS = (2, 5, 33)
BATCHES = (1, 3, None)  # DVS_KMEDOIDS_BATCH; None: the default
MAX_K, MAX_SWAPS_LIMIT = 1024, 65535
# the most exchanges a case of the large sizes is run for: the yardstick's rounds cost n^2 each
LARGE_SWAPS = 4


class Ref(NamedTuple):
    medoids: np.ndarray  # int64 [k]
    labels: np.ndarray   # int64 [n]
    dist: np.ndarray     # float64 [n]
    second: np.ndarray   # float64 [n]
    swaps: np.ndarray    # int64 [m, 2]
    td: np.ndarray       # float64 [m + 1]
    stop: int
    passes: int
    build: np.ndarray    # int64 [k]: the initial medoids


def zero_diagonal(D) -> np.ndarray:
    D0 = np.array(D, dtype=np.float64)
    np.fill_diagonal(D0, 0.0)
    return D0


def state_of(D0: np.ndarray, med: np.ndarray):
    """(near, dn, ds) of the medoids `med` over D0 (the diagonal zeroed): the k cells D0[med[l]][o] per item in slot order"""
    n, k = D0.shape[0], med.size
    cols = np.arange(n)
    cells = D0[med, :].copy()
    near = np.argmin(cells, axis=0)  # (the first of equal values: the lowest slot)
    near[med] = np.arange(k)
    dn = cells[near, cols]
    dn[med] = 0.0
    cells[near, cols] = np.inf
    ds = cells.min(axis=0)  # (+inf when k = 1)
    return near.astype(np.int64), dn, ds


def build_ref(D0: np.ndarray, k: int) -> np.ndarray:
    """PAM's BUILD -> the k initial medoids.  Terms that are exactly zero (an item at distance 0 from a medoid) are left
    out of the sums, which changes no sum."""
    n = D0.shape[0]
    med = [int(np.argmin(D0.sum(axis=1)))]
    dn = D0[med[0]].copy()
    dn[med[0]] = 0.0
    is_med = np.zeros(n, dtype=bool)
    is_med[med[0]] = True
    while len(med) < k:
        live = np.flatnonzero(dn > 0.0)
        cand = np.flatnonzero(~is_med)
        gain = np.maximum(dn[live][None, :] - D0[np.ix_(cand, live)], 0.0).sum(axis=1)
        x = int(cand[np.argmax(gain)])  # (the first of equal gains: the lowest x)
        med.append(x)
        is_med[x] = True
        dn = np.minimum(dn, D0[x])
        dn[x] = 0.0
    return np.array(med, dtype=np.int64)


def build_direct(D, k: int) -> list:
    """the same by the definition's own loops, O(n^2 k) scalar operations"""
    n = len(D)
    sums = [sum(D[x][o] for o in range(n) if o != x) for x in range(n)]
    med = [min(range(n), key=lambda x: (sums[x], x))]
    while len(med) < k:
        dn = [0.0 if o in med else min(D[m][o] for m in med) for o in range(n)]
        best, best_gain = None, None
        for x in range(n):
            if x in med:
                continue
            gain = sum(max(dn[o] - (0.0 if o == x else D[x][o]), 0.0) for o in range(n))
            if best is None or gain > best_gain:
                best, best_gain = x, gain
        med.append(best)
    return med


def round_deltas(D0: np.ndarray, med: np.ndarray, near, dn, ds) -> np.ndarray:
    """Delta_x[l] of one round by the definition's split, float64 [n, k]; +inf in the rows of the medoids"""
    n, k = D0.shape[0], med.size
    if k == 1:
        delta = (D0 - dn[None, :]).sum(axis=1)[:, None]
    else:
        R = np.bincount(near, weights=ds - dn, minlength=k)
        shared = np.minimum(D0 - dn[None, :], 0.0).sum(axis=1)
        c = np.where(D0 < dn[None, :], (dn - ds)[None, :], np.where(D0 < ds[None, :], D0 - ds[None, :], 0.0))
        order = np.argsort(near, kind="stable")
        starts = np.searchsorted(near[order], np.arange(k))  # (every slot holds its medoid: no group is empty)
        C = np.add.reduceat(c[:, order], starts, axis=1)
        delta = (R[None, :] + C) + shared[:, None]
    delta[med, :] = np.inf
    return delta


def kmedoids_ref(D, k: int, init="build", max_swaps: int = 300) -> Ref:
    """include/dvs_hip.h "k-medoids" over the matrix D; init "build" or the initial medoids"""
    D0 = zero_diagonal(D)
    n = D0.shape[0]
    given = not isinstance(init, str)
    med = np.array(init, dtype=np.int64) if given else build_ref(D0, k)
    build = med.copy()
    near, dn, ds = state_of(D0, med)
    td, swaps = [dn.sum()], []
    passes = 1 + (0 if given else k - 1)
    stop = 1 if k == n else 0
    noise = 4.0 * (n + 8.0) * n * 2.0 ** -52 * D0.max()
    while not stop and len(swaps) < max_swaps:
        delta = round_deltas(D0, med, near, dn, ds)
        passes += 1
        x, l = divmod(int(np.argmin(delta)), k)  # (the first of equal values: the lowest x, then the lowest l)
        if not delta[x, l] < -noise:
            stop = 1
            break
        med[l] = x
        near, dn, ds = state_of(D0, med)
        td.append(dn.sum())
        swaps.append((x, l))
    return Ref(med, near, dn, ds, np.array(swaps, dtype=np.int64).reshape(-1, 2), np.array(td), stop, passes, build)


def delta_truth(D, med) -> np.ndarray:
    """every Delta_x[l] in np.longdouble straight from the definition of td: the total distance with slot l given to x
    minus the total distance as it is; [n, k], +inf in the rows of the medoids"""
    D0 = zero_diagonal(D).astype(np.longdouble)
    med = np.asarray(med, dtype=np.int64)
    n, k = D0.shape[0], med.size
    near, dn, ds = state_of(zero_diagonal(D), med)
    dn, ds = dn.astype(np.longdouble), ds.astype(np.longdouble)
    td = dn.sum()
    out = np.full((n, k), np.inf, dtype=np.longdouble)
    rows = np.setdiff1d(np.arange(n), med)
    for l in range(k):
        rest = np.where(near == l, ds, dn)  # the nearest medoid of every item once slot l is empty
        out[rows, l] = np.minimum(D0[rows], rest[None, :]).sum(axis=1) - td
    return out


def gain_truth(D, med) -> np.ndarray:
    """BUILD's gain of every non-medoid x beside the medoids `med`, np.longdouble [n]; -inf for the medoids"""
    D0 = zero_diagonal(D).astype(np.longdouble)
    med = np.asarray(med, dtype=np.int64)
    dn = D0[med].min(axis=0)
    dn[med] = 0
    gain = np.maximum(dn[None, :] - D0, 0).sum(axis=1)
    gain[med] = -np.inf
    return gain


def band(n: int, d_max: float) -> float:
    """what a float64 Delta may be off by: three sums of <= n terms each <= d_max, plus two additions"""
    return 4.0 * (n + 8) * 2.0 ** -52 * n * d_max


def td_bound(n: int) -> float:
    return (n + 8) * 2.0 ** -52


# ---- the families

def _grid(values) -> np.ndarray:
    """onto the multiples of 2^-10 in [2^-10, 4)"""
    return np.clip(np.round(np.asarray(values, dtype=np.float64) * 1024.0), 1.0, 4095.0) / 1024.0


def _points(rng, n: int, clusters: int) -> np.ndarray:
    centres = rng.uniform(-1.0, 1.0, size=(clusters, 3))
    return centres[rng.integers(0, clusters, size=n)] + rng.normal(0.0, 0.08, size=(n, 3))


def exact_matrix(family: str, n: int, seed: int) -> np.ndarray:
    """an n x n matrix of an EXACT family: multiples of 2^-10 below 4 off the diagonal; the diagonal is NaN, which the
    entry must never read"""
    rng = np.random.default_rng([seed, n, EXACT_FAMILIES.index(family)])
    if family == "random":
        D = _grid(rng.uniform(0.0, 4.0, size=(n, n)))
        D = np.triu(D, 1) + np.triu(D, 1).T
    elif family == "clustered":
        p = _points(rng, n, max(2, min(12, n // 8)))
        D = _grid(np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)))
    elif family == "small_integer":
        D = rng.integers(0, 4, size=(n, n)).astype(np.float64)
        D = np.triu(D, 1) + np.triu(D, 1).T
    elif family == "constant":
        D = np.full((n, n), 1.5)
    elif family == "zero":
        D = np.zeros((n, n))
    elif family == "duplicated":
        m = max(1, (n + 2) // 3)
        base = _grid(rng.uniform(0.0, 4.0, size=(m, m)))
        base = np.triu(base, 1) + np.triu(base, 1).T
        np.fill_diagonal(base, 0.0)
        of = rng.integers(0, m, size=n)
        D = base[np.ix_(of, of)]  # copies of one original are at distance 0 from each other
    elif family == "asymmetric":
        D = _grid(rng.uniform(0.0, 4.0, size=(n, n)))
    else:
        raise ValueError(family)
    D = np.ascontiguousarray(D, dtype=np.float64)
    np.fill_diagonal(D, np.nan)
    return D


def general_matrix(family: str, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng([seed, n, 100 + GENERAL_FAMILIES.index(family)])
    if family == "uniform":
        D = rng.uniform(0.0, 1.0, size=(n, n))
        D = np.triu(D, 1) + np.triu(D, 1).T
    elif family == "clustered":
        p = _points(rng, n, 6)
        D = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2))
    elif family == "crowded":  # jsd-like: the values crowded near one value
        D = 0.69 + 0.004 * rng.standard_normal(size=(n, n))
        D = np.abs(np.triu(D, 1) + np.triu(D, 1).T)
    else:
        raise ValueError(family)
    # A symmetric matrix has exact ties by its structure -- the two members of a cluster of two exchange at Delta = 0,
    # two candidates nearer to each other than to any medoid have the same gain -- and a tie has no gap: every cell
    # gets a relative jitter of its own, up to 10^-3, which the entry takes as it takes any asymmetric matrix
    D = D * (1.0 + 1e-3 * rng.uniform(-1.0, 1.0, size=(n, n)))
    D = np.ascontiguousarray(D, dtype=np.float64)
    np.fill_diagonal(D, np.nan)
    return D


class Case(NamedTuple):
    family: str
    n: int
    k: int
    init: str        # "build" or "given"
    max_swaps: int
    seed: int

    @property
    def id(self) -> str:
        return f"{self.family}-n{self.n}-k{self.k}-{self.init}-s{self.max_swaps}"


def given_medoids(case: Case) -> np.ndarray:
    rng = np.random.default_rng([case.seed, case.n, case.k, 7])
    return rng.permutation(case.n)[:case.k].astype(np.int64)


def _exact_cases():
    """every (n, k) of SIZES x KS with k <= n (k = 1024 stands for min(n, 1024), so k = n is there for every n) with
    both kinds of init, the families dealt round over the pairs; then every family at two sizes beside a tile edge"""
    cases, i = [], 0
    for n in SIZES:
        for k in sorted({min(k, n) if k == 1024 else k for k in KS if k <= n or k == 1024}):
            large = n * n * k > 3 * 10 ** 8
            for init in ("build", "given"):
                family = EXACT_FAMILIES[i % len(EXACT_FAMILIES)]
                if large and init == "build":
                    family = "small_integer"  # (BUILD's yardstick costs n^2 a slot: the family whose sums empty fastest)
                i += 1
                cases.append(Case(family, n, k, init, LARGE_SWAPS if n > 300 else 300, 1))
    for family in EXACT_FAMILIES:
        for n, k in ((65, 3), (257, 7)):
            for init in ("build", "given"):
                cases.append(Case(family, n, k, init, 300, 2))
    # k = 16 and 17: either side of the number of medoids up to which a lane keeps buckets of its own
    for n, family in ((65, "random"), (257, "clustered"), (257, "small_integer"), (1025, "asymmetric")):
        for k in (16, 17):
            for init in ("build", "given"):
                cases.append(Case(family, n, k, init, LARGE_SWAPS if n > 300 else 300, 2))
    # max_swaps = 0 (a set scored as it is) and a limit below the yardstick's count of exchanges (stop = 0)
    for family in ("random", "clustered", "asymmetric", "small_integer"):
        for max_swaps in (0, 1, 2):
            cases.append(Case(family, 257, 7, "given", max_swaps, 2))
        cases.append(Case(family, 65, 3, "build", 0, 2))
    return tuple(dict.fromkeys(cases))


EXACT_CASES = _exact_cases()
GENERAL_CASES = tuple(Case(family, n, k, init, 300, 3) for family in GENERAL_FAMILIES for n in GENERAL_SIZES
                      for k in GENERAL_KS for init in ("build", "given"))


@functools.lru_cache(maxsize=None)
def case_matrix(case: Case) -> np.ndarray:
    D = (general_matrix if case in GENERAL_CASES else exact_matrix)(case.family, case.n, case.seed)
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def case_ref(case: Case) -> Ref:
    init = "build" if case.init == "build" else given_medoids(case)
    return kmedoids_ref(case_matrix(case), case.k, init, case.max_swaps)


def gaps_of_run(D, ref: Ref, init_build: bool):
    """the least (second-best - best) over the rounds of the yardstick's run, by the long-double truth: (of the swap
    rounds' Deltas, of BUILD's gains, and the least |best Delta|: its distance from the stop rule's threshold); inf
    where there was nothing to decide"""
    med = ref.build.copy()
    k = med.size
    build_gap = np.inf
    if init_build:
        sums = np.sort(zero_diagonal(D).astype(np.longdouble).sum(axis=1))
        if sums.size > 1:
            build_gap = float(sums[1] - sums[0])
        for m in range(1, k):
            g = np.sort(gain_truth(D, med[:m]))[::-1]
            if g.size > m + 1:
                build_gap = min(build_gap, float(g[0] - g[1]))
    swap_gap = stop_gap = np.inf
    rounds = list(ref.swaps) + ([None] if ref.stop and k < len(D) else [])
    for step in rounds:
        d = np.sort(delta_truth(D, med).ravel())
        if d.size > 1 and np.isfinite(d[1]):
            swap_gap = min(swap_gap, float(d[1] - d[0]))
        stop_gap = min(stop_gap, float(abs(d[0])))
        if step is not None:
            med[step[1]] = step[0]
    return swap_gap, build_gap, stop_gap
