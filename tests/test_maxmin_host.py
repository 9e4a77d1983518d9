"""Farthest-first (max-min) selection without a GPU: `maxmin_ref`, a numpy restatement of the algorithm pinned in
include/dvs_hip.h ("farthest-first selection") that tests/test_gpu_maxmin.py holds the device to bit for bit; the public
names; the argument checks that come before any device work; and the cases of the GPU test as data, with the
preconditions that make them meaningful pinned on the CPU with the oracle's distances."""
from typing import NamedTuple

import numpy as np
import pytest

from diverseseq_amd import _lib, apps, cluster, distance, engine
from test_gpu_linkage import family_seqs
from test_jsd_host import oracle_jsd_matrix


class Ref(NamedTuple):
    picks: np.ndarray
    radius: np.ndarray
    owner: np.ndarray
    dist: np.ndarray
    cover: float


def maxmin_ref(d, n_select=None, seeds=(0,), min_distance=None) -> Ref:
    """the pinned algorithm over the matrix d (rows read as they stand, the diagonal never): two loops -- the seeds,
    the picks -- over one rule, take(p, r)"""
    d = np.asarray(d, dtype=np.float64)
    n = d.shape[0]
    n_select = n if n_select is None else n_select
    mind, owner = np.full(n, np.inf), np.full(n, -1, dtype=np.int64)
    taken, out = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    picks, radius = [], []

    def take(p, r):
        pos = len(picks)
        picks.append(p)
        radius.append(r)
        taken[p], mind[p], owner[p] = True, 0.0, pos
        live = ~taken & ~out
        c = d[p]
        gone = live & np.isnan(c)
        out[gone], mind[gone], owner[gone] = True, np.nan, -1
        with np.errstate(invalid="ignore"):
            nearer = live & ~gone & (c < mind)  # strict: a tie stays with the earlier pick
        mind[nearer], owner[nearer] = c[nearer], pos

    for s in seeds:
        take(int(s), np.nan)
    while len(picks) < n_select:
        live = np.flatnonzero(~taken & ~out)
        if live.size == 0:
            break
        j = int(live[np.argmax(mind[live])])  # the first of equal values: the lowest j
        if min_distance is not None and not mind[j] > min_distance:
            break
        take(j, mind[j])
    live = ~taken & ~out
    return Ref(np.array(picks, dtype=np.int64), np.array(radius, dtype=np.float64), owner, mind,
               float(mind[live].max()) if live.any() else 0.0)


def same_bits(a, b) -> bool:
    """equal shapes, NaN in the same cells, the same bits everywhere else"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return bool((np.ascontiguousarray(a[ok]).view(np.uint64) == np.ascontiguousarray(b[ok]).view(np.uint64)).all())


# ------------------------------------------------------------------ the cases of tests/test_gpu_maxmin.py, as data
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000)  # both sides of a wave and of a workgroup of either width; several workgroups
BINS = ((1, 4), (3, 4), (6, 4), (2, 20))  # (k, states): 4, 64 and 4 096 bins (under a chunk of 64, one, many), 400 (a partial last chunk)
MATRIX_SIZES = (1, 2, 5, 64, 65, 257, 300)
MASH_CASES = tuple((n, s, canonical) for n in (2, 65, 300) for s in (16, 1000) for canonical in (False, True))
BATCHES = (1, 2, 3, 64)
LARGE = dict(n=5000, k=6, n_select=50)
# (nfam, per, length, seed, k): members 3 and 10 of a family are exact copies of its root
FAMILY_CASE = (6, 12, 2000, 9, 4)


def threshold_plan(radius: np.ndarray) -> dict:
    """min_distance values for the family case from the radii of its unbounded run (seed 0), and the number of picks
    each must end at.  A threshold equal to radius[i] ends the run at i picks -- the candidate at that radius is not
    farther than min_distance: the strict > -- provided radius[i - 1] > radius[i].  The stop is decided behind step
    i - 1, the last step of a batch when the batch length divides i: 6 picks end at a batch boundary for batches of 1,
    2 and 3 steps, 4 picks in the middle of a batch of 3 or 64, 5 picks (a threshold between two radii) in the middle
    of a batch of 2, 3 or 64."""
    assert radius[3] > radius[4] > radius[5] > radius[6] > 0.0
    return {"equals_a_radius_mid_batch": (float(radius[4]), 4), "equals_a_radius_at_a_batch_boundary": (float(radius[6]), 6),
            "between_two_radii": (float((radius[4] + radius[5]) / 2), 5)}


# ------------------------------------------------------------------ the restatement, pinned
def test_ref_hand_example():
    x = np.array([0.0, 1.0, 2.0, 4.0, 8.0, 8.0])
    r = maxmin_ref(np.abs(x[:, None] - x[None, :]), 3)
    assert r.picks.tolist() == [0, 4, 3]
    assert np.isnan(r.radius[0]) and r.radius[1:].tolist() == [8.0, 4.0]
    assert r.owner.tolist() == [0, 0, 0, 2, 1, 1]
    assert r.dist.tolist() == [0.0, 1.0, 2.0, 0.0, 0.0, 0.0]
    assert r.cover == 2.0


def test_ref_all_ones_and_nan_row():
    r = maxmin_ref(np.ones((7, 7)), 5)
    assert r.picks.tolist() == [0, 1, 2, 3, 4] and r.radius[1:].tolist() == [1.0] * 4
    assert r.owner.tolist() == [0, 1, 2, 3, 4, 0, 0] and r.cover == 1.0
    d = np.random.default_rng(0).random((9, 9))
    d[4, :] = d[:, 4] = np.nan
    r = maxmin_ref(d)
    assert 4 not in r.picks.tolist() and sorted(r.picks.tolist()) == [0, 1, 2, 3, 5, 6, 7, 8]
    assert r.owner[4] == -1 and np.isnan(r.dist[4]) and r.cover == 0.0
    r = maxmin_ref(d, seeds=(4,))  # a seed that is NaN against everything: the rest goes out
    assert r.picks.tolist() == [4] and (np.delete(r.owner, 4) == -1).all() and r.owner[4] == 0 and r.cover == 0.0
    r = maxmin_ref(d, 3, seeds=(1, 4))  # ... taken all the same when it is a later seed, and the rest goes out then
    assert r.picks.tolist() == [1, 4] and r.owner[4] == 1 and r.dist[4] == 0.0 and r.owner[1] == 0
    assert (np.delete(r.owner, [1, 4]) == -1).all() and np.isnan(np.delete(r.dist, [1, 4])).all()


@pytest.mark.parametrize("n", [1, 2, 5, 64, 65, 200])
def test_ref_properties(n):
    rng = np.random.default_rng(n)
    d = rng.random((n, n))
    d = np.triu(d, 1) + np.triu(d, 1).T
    full = maxmin_ref(d)
    assert sorted(full.picks.tolist()) == list(range(n)) and full.cover == 0.0
    rad = full.radius[1:]
    assert (np.diff(rad) <= 0).all()
    for m in sorted(m for m in {1, 2, n // 2, n} if 1 <= m <= n):
        part = maxmin_ref(d, m)
        assert part.picks.tolist() == full.picks[:m].tolist()
        if m > 1:
            sub = d[np.ix_(part.picks, part.picks)] + np.diag(np.full(m, np.inf))
            assert sub.min() >= part.radius[-1]
        assert np.array_equal(part.dist, d[:, part.picks].min(axis=1) * (1 - np.eye(n)[part.picks].sum(axis=0)))
    for t in (0.0, 0.1, 0.5, float(rad[len(rad) // 2]) if n > 2 else 0.3, 2.0):
        cut = maxmin_ref(d, min_distance=t)
        m = len(cut.picks)
        assert cut.picks.tolist() == full.picks[:m].tolist() and cut.cover <= t
        assert m == n or full.radius[m] <= t
        assert m == 1 or full.radius[m - 1] > t


# ------------------------------------------------------------------ the names
def test_public_names_exist():
    for name in ("MaxMin", "maxmin", "matrix_maxmin", "mash_maxmin", "jsd_maxmin", "euclidean_maxmin", "check_maxmin_args"):
        assert hasattr(distance, name), name
    assert distance.MaxMin._fields == ("picks", "radius", "owner", "dist", "cover")
    assert callable(distance.Sketches.maxmin) and callable(cluster.maxmin) and callable(engine.Selection.diversify)
    assert callable(apps.dvs_maxmin) and "dvs_maxmin" in apps.__all__
    new = {"dvs_maxmin"}  # one entry: the mode, or the caller's matrix, travels in the dvs_source
    assert new <= set(_lib.EXPORTS)
    lib = _lib.load()
    for name in new:
        assert getattr(lib, name).argtypes is not None, name
    assert lib.dvs_abi_version() == 5


# ------------------------------------------------------------------ argument errors come before any device work
class _NoContext:
    """stands in for a context: any use is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the context was used ({name}) before the arguments were checked")


BAD_ARGS = (  # (keyword arguments over 5 items, what the message names)
    (dict(), "n_select, min_distance or both"),
    (dict(n_select=3, seeds=()), "seeds"),
    (dict(n_select=3, seeds=(5,)), "seed outside"),
    (dict(n_select=3, seeds=(-1,)), "seed outside"),
    (dict(n_select=3, seeds=(1, 2, 1)), "more than once"),
    (dict(n_select=3, seeds=(0.5,)), "seeds"),
    (dict(n_select=1, seeds=(0, 1)), "n_select = 1"),
    (dict(n_select=6), "n_select = 6"),
    (dict(n_select=0), "n_select = 0"),
    (dict(n_select=2.0), "n_select must be an integer"),
    (dict(n_select=True), "n_select must be an integer"),
    (dict(n_select=3, min_distance=float("nan")), "NaN"),
    (dict(min_distance=float("nan")), "NaN"),
)


@pytest.mark.parametrize("kw,match", BAD_ARGS)
def test_argument_errors_need_no_context(kw, match):
    ctx = _NoContext()
    a = [np.arange(30, dtype=np.uint8) % 4 for _ in range(5)]
    kw = dict(kw)
    n_select = kw.pop("n_select", None)
    with pytest.raises(ValueError, match=match):
        cluster.maxmin(np.zeros((5, 5)), n_select, ctx=ctx, **kw)
    for mode, extra in (("jsd", {}), ("euclidean", {}), ("mash", dict(sketch_size=20))):
        with pytest.raises(ValueError, match=match):
            distance.maxmin(a, n_select, mode, k=3, ctx=ctx, **extra, **kw)

    class _Matrix:  # (checked before the handle is touched)
        nrows, ctx = 5, _NoContext()

    with pytest.raises(ValueError, match=match):
        distance.matrix_maxmin(_Matrix(), n_select, **kw)


def test_mode_and_shape_errors_need_no_context():
    ctx = _NoContext()
    a = [np.arange(30, dtype=np.uint8) % 4 for _ in range(5)]
    with pytest.raises(ValueError, match="Unexpected distance 'manhattan'"):
        distance.maxmin(a, 2, "manhattan", k=3, ctx=ctx)
    with pytest.raises(ValueError, match="Expected sketch size"):
        distance.maxmin(a, 2, "mash", k=3, ctx=ctx)
    with pytest.raises(ValueError, match="Sketch size"):
        distance.maxmin(a, 2, "jsd", k=3, sketch_size=10, ctx=ctx)
    with pytest.raises(ValueError, match="Canonical kmers"):
        distance.maxmin(a, 2, "euclidean", k=3, mash_canonical=True, ctx=ctx)
    with pytest.raises(ValueError, match="seed outside"):
        distance.maxmin([], 1, "jsd", k=3, ctx=ctx)
    with pytest.raises(ValueError, match="square distance matrix"):
        cluster.maxmin(np.zeros((3, 4)), 2, ctx=ctx)

    class _Matrix:
        nrows, ctx = 5, _NoContext()

    with pytest.raises(ValueError, match="Unexpected distance 'mash'"):
        distance.matrix_maxmin(_Matrix(), 2, mode="mash")


def test_dvs_maxmin_constructor_checks():
    with pytest.raises(ValueError, match="Unexpected distance 'manhattan'"):
        apps.dvs_maxmin(3, distance_mode="manhattan")
    with pytest.raises(ValueError, match="Expected sketch size for mash distance measure"):
        apps.dvs_maxmin(3, sketch_size=None)
    with pytest.raises(ValueError, match="Canonical kmers only supported for dna sequences"):
        apps.dvs_maxmin(3, moltype="protein", mash_canonical_kmers=True)
    with pytest.raises(ValueError, match="n, min_distance or both"):
        apps.dvs_maxmin()
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="n must be an integer"):
            apps.dvs_maxmin(bad)
    with pytest.raises(ValueError, match="NaN"):
        apps.dvs_maxmin(min_distance=float("nan"))
    with pytest.raises(ValueError, match="one seed at least"):
        apps.dvs_maxmin(3, seeds=[])
    with pytest.raises(ValueError, match="seed names not among"):
        apps.dvs_maxmin(1, distance_mode="jsd", k=2, seeds="zebra")({"a": "ACGTACGT", "b": "AACCGGTT"})


# ------------------------------------------------------------------ the family case of the GPU test
def test_family_case_preconditions():
    nfam, per, length, seed, k = FAMILY_CASE
    seqs = family_seqs(nfam, per, length, seed)
    names = list(seqs)
    assert len(names) == nfam * per
    d = oracle_jsd_matrix([seqs[n] for n in names], k)
    assert not np.isnan(d).any()
    zero = {(names[i], names[j]) for i, j in zip(*np.nonzero(np.triu(d == 0.0, 1)))}
    assert zero == {(f"fam{f}_m3", f"fam{f}_m10") for f in range(nfam)}  # exact duplicates: ties at 0
    full = maxmin_ref(d)
    plan = threshold_plan(full.radius)  # (asserts that the radii around the thresholds differ)
    for t, m in plan.values():
        r = maxmin_ref(d, min_distance=t)
        assert len(r.picks) == m and r.picks.tolist() == full.picks[:m].tolist()
    t, m = plan["equals_a_radius_at_a_batch_boundary"]
    assert t == full.radius[m] and all(m % b == 0 for b in (1, 2, 3))
    t, m = plan["equals_a_radius_mid_batch"]
    assert t == full.radius[m] and m % 3 != 0 and m % 64 != 0
    dedup = maxmin_ref(d, min_distance=0.0)  # one of every group of duplicates
    assert len(dedup.picks) == len(names) - nfam and dedup.cover == 0.0
    assert (full.radius[len(dedup.picks):] == 0.0).all()
