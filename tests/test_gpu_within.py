"""Neighbours within a radius and threshold clusters on the GPU (the within_* kernels and their drivers in
csrc/within.hip).  The expected pairs always come from something other than the code under test: `expected_within`
(tests/test_within_host.py: numpy's nonzero of d <= radius) over the matrix that the existing cross_distances / distances
entries return for the same handles, or over a caller's own seeded matrix; the expected labels from `expected_components`
(pinned there against scipy twice) and from the project's own single linkage and cut.  tests/test_within_host.py pins
the family cases' radii on the CPU."""
import ctypes as C

import numpy as np
import pytest

import oracle
from diverseseq_amd import _lib, apps, cluster, distance, engine
from test_blocks_host import POISON, assert_same_outputs
from test_cross_host import FAMILY_CASES
from test_gpu_cross import _seqs, same_bits
from test_within_host import expected_components, expected_within, family_within_case, tie_matrix

pytestmark = pytest.mark.gpu

# pairs of (queries, references) from the sizes on both sides of a 32-row tile and a 64-column wave step: every size on
# either side, the ends against each other
SIZES = (1, 31, 32, 33, 63, 64, 65, 129, 200)
SIZE_PAIRS = ((1, 1), (1, 200), (200, 1), (31, 65), (32, 64), (33, 63), (63, 33), (64, 32), (65, 31), (129, 129),
              (200, 129), (64, 200))
MODES = ("jsd", "euclidean")


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def radii_of(d: np.ndarray):
    """the radii every case is run at: negative, 0, a cell of the matrix exactly (its median), one ulp below it, +inf"""
    cells = np.sort(d[~np.isnan(d)])
    median = float(cells[cells.size // 2]) if cells.size else 0.5
    return (-0.25, 0.0, median, float(np.nextafter(median, -np.inf)), float("inf")), median


def assert_within(nb, d, radius, skip_self=False, what=""):
    """a Neighbours against expected_within over the matrix d: the same cells in the same order, the same bits"""
    rs, idx, val = expected_within(d, radius, skip_self)
    assert isinstance(nb, distance.Neighbours), what
    assert nb.row_start.dtype == np.int64 and nb.index.dtype == np.int64 and nb.distance.dtype == np.float64, what
    assert np.array_equal(nb.row_start, rs), (what, radius)
    assert np.array_equal(nb.index, idx), (what, radius)
    assert same_bits(nb.distance, val) and not np.isnan(nb.distance).any(), (what, radius)
    # stated on their own, though the equalities imply them: ascending within a row, the bits of the matrix cell
    row_of = np.repeat(np.arange(d.shape[0]), np.diff(nb.row_start))
    assert (np.diff(nb.index)[np.diff(row_of) == 0] > 0).all(), (what, radius)
    assert same_bits(nb.distance, np.asarray(d, dtype=np.float64)[row_of, nb.index]), (what, radius)
    for i in (0, d.shape[0] - 1):
        mine, dist = nb.of(i)
        assert np.array_equal(mine, idx[rs[i]:rs[i + 1]]) and same_bits(dist, d[i, mine]), (what, radius, i)


def assert_all_radii(run, d, skip_self=False, what=""):
    """run(radius) -> Neighbours at every radius of radii_of(d); -> the median"""
    radii, median = radii_of(d)
    counts = []
    for radius in radii:
        nb = run(radius)
        assert_within(nb, d, radius, skip_self, what)
        counts.append(int(nb.row_start[-1]))
    keep = ~np.isnan(d)
    if skip_self:
        keep[np.arange(min(d.shape)), np.arange(min(d.shape))] = False
    assert counts[0] == 0 and counts[4] == int(keep.sum()), what  # nothing; every cell that is not NaN
    if keep.any() and median in d[keep]:
        assert counts[2] > counts[3], what                        # the radius is inclusive: one ulp less loses that cell
    return median


def same_neighbours(a, b) -> bool:
    return (np.array_equal(a.row_start, b.row_start) and np.array_equal(a.index, b.index)
            and same_bits(a.distance, b.distance))


# ------------------------------------------------------------------ 1. same cells, same order, every mode and element type
def _row_lists(rng, m, n):
    """(query rows, reference rows) into the m + n stacked rows: shuffled, and with repeats on BOTH sides -- where a
    position in the list and the matrix row behind it part ways"""
    head = rng.permutation(m + n)[: max(1, m)]
    qr = np.concatenate([head, rng.integers(0, m + n, size=3), head[:2], head[:1]])
    rr = np.concatenate([rng.integers(0, m + n, size=n), qr[:1], qr[:1]])
    assert np.unique(qr).size < qr.size and np.unique(rr).size < rr.size
    return qr, rr


def assert_twins_are_listed(nb, rows, totals):
    """nb: a list against itself at radius 0 with skip_self.  Position a never lists a; it does list every other
    position b of the same matrix row (distance exactly 0), unless that row has no valid k-mer (NaN)"""
    for a, row in enumerate(rows):
        mine = nb.of(a)[0]
        assert a not in mine, a
        twins = [b for b in np.flatnonzero(rows == row) if b != a]
        assert all((b in mine) == bool(totals[row]) for b in twins), (a, twins, mine)
    assert any(np.flatnonzero(rows == row).size > 1 and totals[row] for row in rows)


def _two_sides(rng, m, n, states=4, empties=True):
    """the rows of test_gpu_cross._count_case: an empty sequence on each side, an identical pair across the sides"""
    q = _seqs(rng, m, states, empty=(3,) if empties else ())
    r = _seqs(rng, n, states, empty=(5,) if empties else ())
    if n > 2 and m > 1:
        r[1] = q[0].copy()
    return q, r


def _matrices(ctx, monkeypatch, kind, q, r, k, states=4):
    """(the queries' matrix, the references', their stack's) of element type `kind`"""
    if kind == "freq":
        f = [np.stack([oracle.to_kfreqs(s, states, k)[0] for s in x]) for x in (q, r, q + r)]
        return tuple(ctx.matrix_from_freqs(x) for x in f)
    if kind == "u32":
        monkeypatch.setenv("DVS_COUNTS_U32", "1")
    mq = ctx.build_matrix(q, k, states)
    if kind == "mixed":
        monkeypatch.setenv("DVS_COUNTS_U32", "1")
    mr, ms = ctx.build_matrix(r, k, states), ctx.build_matrix(q + r, k, states)
    want = {"u16": (2, 2), "u32": (4, 4), "mixed": (2, 4)}[kind]
    assert (mq.count_bytes, mr.count_bytes) == want
    return mq, mr, ms


def _count_within_case(ctx, monkeypatch, mode, kind, m, n, k, seed):
    rng = np.random.default_rng(seed)
    q, r = _two_sides(rng, m, n, empties=kind != "freq")
    mq, mr, ms = _matrices(ctx, monkeypatch, kind, q, r, k)
    try:
        d = distance.matrix_cross_distances(mq, mr, mode)
        assert d.shape == (m, n)
        assert_all_radii(lambda radius: distance.matrix_within(mq, mr, radius, mode), d, what=(mode, kind, m, n))
        if n > 2 and m > 1:  # at 0: the identical pair and nothing else
            nb = distance.matrix_within(mq, mr, 0.0, mode)
            assert nb.index.tolist() == [1] and nb.of(0)[0].tolist() == [1] and nb.distance.tolist() == [0.0]
        if kind != "freq" and m > 3 and n > 5:  # none of the NaN cells, at any radius
            nb = distance.matrix_within(mq, mr, float("inf"), mode)
            assert nb.of(3)[0].size == 0 and 5 not in nb.index and np.isnan(d[3]).all() and np.isnan(d[:, 5]).all()
        # shuffled and repeated row lists on both sides, into the stacked matrix
        qr, rr = _row_lists(rng, m, n)
        via = distance.matrix_cross_distances(ms, ms, mode, q_rows=qr, r_rows=rr)
        assert_all_radii(lambda radius: distance.matrix_within(ms, ms, radius, mode, q_rows=qr, r_rows=rr), via,
                         what=(mode, kind, m, n, "row lists"))
        # the repeated list against itself: skip_self drops position a against position a, not row against row
        own = distance.matrix_cross_distances(ms, ms, mode, q_rows=qr, r_rows=qr)
        assert_all_radii(lambda radius: distance.matrix_within(ms, ms, radius, mode, q_rows=qr, r_rows=qr, skip_self=True),
                         own, skip_self=True, what=(mode, kind, m, n, "a repeated list against itself"))
        assert_twins_are_listed(distance.matrix_within(ms, ms, 0.0, mode, q_rows=qr, r_rows=qr, skip_self=True), qr, ms.totals())
    finally:
        for x in (mq, mr, ms):
            x.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m,n", SIZE_PAIRS)
def test_count_modes_same_cells_same_order_sizes(ctx, monkeypatch, mode, m, n):
    assert {a for pair in SIZE_PAIRS for a in pair} == set(SIZES)
    _count_within_case(ctx, monkeypatch, mode, "u16", m, n, 3, 1000 * m + n)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["u32", "freq", "mixed"])
def test_count_modes_same_cells_same_order_element_types(ctx, monkeypatch, mode, kind):
    _count_within_case(ctx, monkeypatch, mode, kind, 33, 65, 4, 77)


@pytest.mark.parametrize("m,n", [(1, 1), (33, 65), (64, 200), (200, 63)])
def test_mash_same_cells_same_order(ctx, m, n):
    rng = np.random.default_rng(31 * m + n)
    q, r = _two_sides(rng, m, n, empties=False)  # (two empty sketches would divide by zero)
    skq, skr, sks = (distance.Sketches(x, 8, 50, ctx=ctx) for x in (q, r, q + r))
    try:
        d = skq.cross_distances(skr)
        run = lambda radius: distance.DeviceSide(skq, "mash").within(distance.DeviceSide(skr, "mash"), radius)  # noqa: E731
        assert_all_radii(run, d, what=("mash", m, n))
        if n > 2 and m > 1:
            assert run(0.0).index.tolist() == [1]
        median = radii_of(d)[1]
        assert same_neighbours(skq.within(skr, median), run(median))  # (the Sketches methods are the same calls)
        assert np.array_equal(sks.threshold_clusters(median).labels, distance.DeviceSide(sks, "mash").threshold_clusters(median).labels)
        qr, rr = _row_lists(rng, m, n)
        side = distance.DeviceSide(sks, "mash")
        assert_all_radii(lambda radius: side.within(side, radius, qr, qr, skip_self=True), sks.cross_distances(sks, qr, qr),
                         skip_self=True, what=("mash", m, n, "a repeated list against itself"))
        assert_twins_are_listed(side.within(side, 0.0, qr, qr, skip_self=True), qr, np.ones(m + n))
        assert_all_radii(lambda radius: side.within(side, radius, qr, rr), sks.cross_distances(sks, qr, rr),
                         what=("mash", m, n, "row lists"))
    finally:
        for x in (skq, skr, sks):
            x.close()


def test_module_functions_over_sequences(ctx):
    rng = np.random.default_rng(9)
    q, r = _two_sides(rng, 40, 70)
    for mode, kw in (("jsd", {}), ("euclidean", {}), ("mash", dict(sketch_size=40))):
        qq, rr = (q, r) if mode != "mash" else _two_sides(np.random.default_rng(9), 40, 70, empties=False)
        d = distance.cross_distances(qq, rr, mode, k=4, ctx=ctx, **kw)
        median = radii_of(d)[1]
        assert_within(distance.within(qq, rr, median, mode, k=4, ctx=ctx, **kw), d, median, what=mode)
        dd = distance.cross_distances(qq, qq, mode, k=4, ctx=ctx, **kw)
        assert_within(distance.neighbours(qq, median, mode, k=4, ctx=ctx, **kw), dd, median, skip_self=True, what=mode)


# ------------------------------------------------------------------ 2. wide and tall
def _planted(n: int, seed: int):
    """tie_matrix with NaN and +inf cells, a row of NaN, and many cells exactly at the radius 2/64"""
    d = tie_matrix(n, seed)
    rng = np.random.default_rng(seed + 1)
    hit = rng.integers(0, n, size=(400, 2))
    d[hit[:200, 0], hit[:200, 1]] = np.nan
    d[hit[200:, 0], hit[200:, 1]] = np.inf
    d[n // 2, :] = np.nan
    d[5, n - 1] = d[n - 1, 2047] = d[n - 1, 2048] = 2 / 64  # (the last column, and both sides of a 2 048-cell staging)
    return d, 2 / 64


def test_wide_rows_of_a_callers_matrix_host_and_device(ctx):
    """(where this is the first test of a process to put a tensor on the device, its time is torch's initialisation)"""
    torch = pytest.importorskip("torch")
    n = 2049
    d, radius = _planted(n, 12)
    assert (d == radius).sum() > 1000 and np.isnan(d[n // 2]).all()
    on_device = torch.from_numpy(d).cuda()
    for skip_self in (True, False):
        host = cluster.within(d, radius, skip_self=skip_self, ctx=ctx)
        assert_within(host, d, radius, skip_self, what="host matrix")
        assert host.of(n // 2)[0].size == 0
        assert same_neighbours(cluster.within(on_device, radius, skip_self=skip_self, ctx=ctx), host)
    assert_within(cluster.within(d, float("inf"), ctx=ctx), d, float("inf"), True, what="every cell")  # +inf cells too
    assert np.array_equal(on_device.cpu().numpy(), d, equal_nan=True)  # only read


def test_one_very_tall_strip(ctx):
    rng = np.random.default_rng(50)
    q = [rng.integers(0, 4, size=int(rng.integers(20, 60)), dtype=np.uint8) for _ in range(5000)]
    q[4999] = q[0].copy()
    mq, mr = ctx.build_matrix(q, 2, 4), ctx.build_matrix([q[0], q[1], np.full(30, 4, np.uint8)], 2, 4)
    try:
        d = distance.matrix_cross_distances(mq, mr, "euclidean")
        assert d.shape == (5000, 3) and np.isnan(d[:, 2]).all()
        median = assert_all_radii(lambda radius: distance.matrix_within(mq, mr, radius, "euclidean"), d, what="tall")
        nb = distance.matrix_within(mq, mr, median, "euclidean")
        assert 2000 < nb.row_start[-1] < 8000 and nb.of(4999)[0][0] == 0 and nb.of(4999)[1][0] == 0.0
    finally:
        mq.close()
        mr.close()


# ------------------------------------------------------------------ 3. strip heights
@pytest.mark.parametrize("strip", [1, 32, 33])
def test_strip_height_does_not_change_a_bit(ctx, monkeypatch, strip):
    rng = np.random.default_rng(5)
    q, r = _seqs(rng, 200, empty=(3, 150)), _seqs(rng, 65, empty=(5,))
    r[64] = r[2].copy()
    sq_, sr_ = _seqs(rng, 200), _seqs(rng, 65)
    D = tie_matrix(130, 8)
    mq, mr = ctx.build_matrix(q, 4, 4), ctx.build_matrix(r, 4, 4)
    skq, skr = distance.Sketches(sq_, 8, 50, ctx=ctx), distance.Sketches(sr_, 8, 50, ctx=ctx)
    try:
        radius = {mode: radii_of(distance.matrix_cross_distances(mq, mr, mode))[1] for mode in MODES}
        radius["mash"] = radii_of(skq.cross_distances(skr))[1]
        # (about two edges a row: components of many sizes)
        self_radius = {mode: float(np.nanquantile(distance.DeviceSide(mq, mode).distances()[np.triu_indices(200, 1)], 0.01))
                       for mode in MODES}

        def run():
            out = {"host": cluster.within(D, 6 / 64, ctx=ctx), "host labels": cluster.threshold_clusters(D, 6 / 64, ctx=ctx),
                   "mash": distance.DeviceSide(skq, "mash").within(distance.DeviceSide(skr, "mash"), radius["mash"]),
                   "mash labels": distance.DeviceSide(skq, "mash").threshold_clusters(radius["mash"])}
            for mode in MODES:
                out[mode] = distance.matrix_within(mq, mr, radius[mode], mode)
                out[mode + " self"] = distance.matrix_within(mq, mq, radius[mode], mode, skip_self=True)
                out[mode + " labels"] = distance.matrix_threshold_clusters(mq, self_radius[mode], mode)
            return out

        whole = run()
        assert 1 < whole["host labels"].n_clusters < 130 and whole["jsd"].row_start[-1] > 1000
        monkeypatch.setenv("DVS_CROSS_STRIP_ROWS", str(strip))
        for what, got in run().items():
            if isinstance(got, distance.Neighbours):
                assert same_neighbours(got, whole[what]), (what, strip)
            else:
                assert np.array_equal(got.labels, whole[what].labels) and got.n_clusters == whole[what].n_clusters, (what, strip)
    finally:
        for x in (mq, mr, skq, skr):
            x.close()


# ------------------------------------------------------------------ 4. skip_self
@pytest.mark.parametrize("mode", ["jsd", "euclidean", "mash"])
def test_skip_self_of_a_collection_against_itself(ctx, mode):
    rng = np.random.default_rng(44)
    seqs = _seqs(rng, 129, empty=() if mode == "mash" else (7,))
    seqs[100], seqs[64] = seqs[2].copy(), seqs[63].copy()  # pairs at exactly 0
    handle = distance.Sketches(seqs, 8, 50, ctx=ctx) if mode == "mash" else ctx.build_matrix(seqs, 4, 4)
    try:
        side = distance.DeviceSide(handle, mode)
        d = side.cross_distances(side)
        median = assert_all_radii(lambda radius: side.within(side, radius, skip_self=True), d, skip_self=True, what=mode)
        nb = side.within(side, median, skip_self=True)
        pairs = {(i, int(j)): v for i in range(129) for j, v in zip(*nb.of(i))}
        assert pairs and all(i != j for i, j in pairs)
        assert all((j, i) in pairs and np.float64(pairs[(j, i)]).tobytes() == np.float64(v).tobytes() for (i, j), v in pairs.items())
        assert side.within(side, 0.0, skip_self=True).of(2)[0].tolist() == [100]
    finally:
        handle.close()


def test_skip_self_never_reads_the_diagonal_of_a_callers_matrix(ctx):
    d = tie_matrix(200, 21)
    clean = cluster.within(d, 8 / 64, ctx=ctx)
    assert_within(clean, d, 8 / 64, True)
    labels = cluster.threshold_clusters(d, 3 / 64, ctx=ctx)
    for poison in (np.nan, -1.0):
        p = d.copy()
        np.fill_diagonal(p, poison)
        assert same_neighbours(cluster.within(p, 8 / 64, ctx=ctx), clean), poison
        assert np.array_equal(cluster.threshold_clusters(p, 3 / 64, ctx=ctx).labels, labels.labels), poison
    # without skip_self the diagonal is a cell like any other
    assert_within(cluster.within(d, 8 / 64, skip_self=False, ctx=ctx), d, 8 / 64, False)


# ------------------------------------------------------------------ 5. max_pairs
@pytest.mark.parametrize("strip", [None, 32])
def test_max_pairs(ctx, monkeypatch, strip):
    if strip:
        monkeypatch.setenv("DVS_CROSS_STRIP_ROWS", str(strip))
    d = tie_matrix(200, 33)
    radius = 8 / 64
    total = int(expected_within(d, radius, True)[0][-1])
    assert total > 300
    with pytest.raises(NotImplementedError, match=f"max_pairs = {total - 1}") as err:
        cluster.within(d, radius, max_pairs=total - 1, ctx=ctx)
    assert any(tok.isdigit() and int(tok) > total - 1 for tok in str(err.value).split())  # both numbers are named
    for limit in (total, total + 1, None):  # the context gives the right answer on the next call
        assert_within(cluster.within(d, radius, max_pairs=limit, ctx=ctx), d, radius, True, what=limit)
    with pytest.raises(NotImplementedError):
        cluster.within(d, radius, max_pairs=1, ctx=ctx)
    assert cluster.threshold_clusters(d, 3 / 64, ctx=ctx).n_clusters == expected_components(d, 3 / 64).max() + 1


# ------------------------------------------------------------------ 6. threshold clusters
def assert_labels(got, D, t, what="", tree=True, Z=None):
    want = expected_components(D, t)
    assert isinstance(got, distance.ThresholdClusters) and got.labels.dtype == np.int64, what
    assert np.array_equal(got.labels, want), (what, t)
    assert got.n_clusters == (int(want.max()) + 1 if want.size else 0), (what, t)
    assert np.array_equal(got.sizes, np.bincount(want, minlength=got.n_clusters)), (what, t)
    if tree and D.shape[0] >= 2:  # equal as arrays, not only as partitions, to the project's own single linkage and cut
        Z = cluster.linkage(D, "single") if Z is None else Z
        assert np.array_equal(got.labels, cluster.cut_tree(Z, height=t)), (what, t)


def thresholds_of(D):
    """below every cell, above every cell, and cells of the matrix (ties) that pass about 0.5, 1.5 and 4 edges a row"""
    n = D.shape[0]
    v = np.sort(D[np.triu_indices(n, 1)])
    if not v.size:
        return [0.5]
    cells = [float(v[min(v.size - 1, int(f * n))]) for f in (0.25, 0.75, 2.0)]
    return [float(np.nextafter(v[0], -np.inf)), *cells, float(v[-1])]


@pytest.mark.parametrize("mode", ["jsd", "euclidean", "mash"])
@pytest.mark.parametrize("n", [1, 2, 33, 200])
def test_threshold_clusters_are_the_single_linkage_cut(ctx, mode, n):
    rng = np.random.default_rng(600 + n)
    seqs = _seqs(rng, n)
    if n > 20:
        seqs[17] = seqs[4].copy()
    with distance.device_side(seqs, mode, *((8, 50) if mode == "mash" else (4, 4)), ctx=ctx) as side:
        D = side.distances()
        counts = set()
        for t in thresholds_of(D):
            got = side.threshold_clusters(t)
            assert_labels(got, D, t, what=(mode, n))
            counts.add(got.n_clusters)
        assert {1, n} <= counts  # n singletons below every cell, one cluster above every cell
        rows = np.concatenate([rng.permutation(n)[: max(1, n // 2)], rng.integers(0, n, size=min(n, 3))])  # shuffled, repeated
        t = thresholds_of(D)[len(thresholds_of(D)) // 2]
        assert_labels(side.threshold_clusters(t, rows), D[np.ix_(rows, rows)], t, what=(mode, n, "rows"))


@pytest.mark.parametrize("n", [1, 2, 33, 200, 2049])
def test_threshold_clusters_of_a_callers_matrix_with_ties(ctx, n):
    D = tie_matrix(n, 70 + n)
    # (n = 2 049: no edge; half an edge a row; two; thirty-six, which joins everything)
    ts = thresholds_of(D) if n < 2049 else (0.0, 1 / 64, 2 / 64, 6 / 64)
    Z = cluster.linkage(D, "single", ctx=ctx) if n >= 2 else None
    counts = set()
    for t in ts:
        got = cluster.threshold_clusters(D, t, ctx=ctx)
        assert_labels(got, D, t, what=n, Z=Z)
        counts.add(got.n_clusters)
    assert {1, n} <= counts
    if n == 2049:
        assert (D == 1 / 64).sum() > 500 and len(counts) == 4
    torch = pytest.importorskip("torch")
    dev = torch.from_numpy(D).cuda()
    t = ts[len(ts) // 2]
    assert np.array_equal(cluster.threshold_clusters(dev, t, ctx=ctx).labels, expected_components(D, t))
    assert np.array_equal(dev.cpu().numpy(), D)


def test_a_row_of_nan_is_a_singleton(ctx):
    D = tie_matrix(65, 3)
    D[40, :] = D[:, 40] = np.nan
    got = cluster.threshold_clusters(D, 1.0, ctx=ctx)
    assert_labels(got, D, 1.0, tree=False)
    assert got.n_clusters == 2 and got.sizes.tolist() == [64, 1]
    rng = np.random.default_rng(8)
    seqs = _seqs(rng, 65, empty=(40,))
    for mode in MODES:  # a sequence without a valid k-mer: NaN against every other
        with distance.device_side(seqs, mode, 4, 4, ctx=ctx) as side:
            got = side.threshold_clusters(float("inf"))
            assert got.n_clusters == 2 and got.labels[40] == 1 and got.sizes.tolist() == [64, 1]
            assert_labels(got, side.distances(), float("inf"), tree=False)
        assert np.array_equal(distance.threshold_clusters(seqs, float("inf"), mode, k=4, ctx=ctx).labels, got.labels)


# ------------------------------------------------------------------ 7. the oracle's families
@pytest.mark.parametrize("case", FAMILY_CASES, ids=["k4", "k6"])
def test_families_neighbours_dereplicate_and_the_app(ctx, case):
    nfam, per, length, seed, k = case
    names, seqs, d, radius, _ = family_within_case(case)
    rs, idx, _ = expected_within(d, radius, skip_self=True)
    nb = distance.neighbours(seqs, radius, "jsd", k=k, ctx=ctx)
    assert np.array_equal(nb.row_start, rs) and np.array_equal(nb.index, idx)  # exactly the oracle's pair set
    assert (nb.distance <= radius).all()
    family = np.arange(nfam * per) // per
    tree, Z, sc = cluster.dereplicate(dict(zip(names, seqs)), radius, k=k, sketch_size=None, distance_mode="jsd")
    assert tree is None and Z is None and isinstance(sc, distance.ClusterScores)
    assert np.array_equal(sc.labels, family) and sc.sizes.tolist() == [per] * nfam
    assert all(family[m] == c for c, m in enumerate(sc.medoids.tolist()))  # a representative inside each family
    out = apps.dvs_dereplicate(radius, "jsd", k=k)(dict(zip(names, seqs)))
    assert out["tree"] is None and set(out) == {"tree", "clusters", "medoids", "silhouette", "mean_silhouette"}
    assert out["clusters"] == {c: [n for n in names if n.startswith(f"fam{c}_")] for c in range(nfam)}
    assert out["medoids"] == {c: names[m] for c, m in enumerate(sc.medoids.tolist())}
    assert out["mean_silhouette"] == sc.mean_silhouette


# ------------------------------------------------------------------ 8. poisoned and reused blocks
def _within_and_clusters(c, radii=None):
    """every new entry once on the context c -> its outputs by name; radii None: -> the radii instead, a quarter of
    the cells for the lists and about two edges a row for the labels, from the matrices the existing entries give"""
    rng = np.random.default_rng(88)
    q, r = _seqs(rng, 129, empty=(3,)), _seqs(rng, 65, empty=(5,))
    r[1] = q[0].copy()
    D = tie_matrix(257, 5)
    mq, mr = c.build_matrix(q, 4, 4), c.build_matrix(r, 4, 4)
    skq = distance.Sketches(_seqs(rng, 129), 8, 50, ctx=c)
    out = {}
    try:
        side = distance.DeviceSide(skq, "mash")
        if radii is None:
            sides = {"jsd": distance.DeviceSide(mq, "jsd"), "euclidean": distance.DeviceSide(mq, "euclidean"), "mash": side}
            return {mode: (float(np.nanquantile(s.distances(), 0.25)), float(np.nanquantile(s.distances(), 2 / 129)))
                    for mode, s in sides.items()}

        def put(name, got):
            for field, value in zip(got._fields, got):
                out[f"{name}.{field}"] = np.asarray(value)

        for mode in MODES:
            put(mode, distance.matrix_within(mq, mr, radii[mode][0], mode))
            put(mode + " self", distance.matrix_within(mq, mq, radii[mode][0], mode, skip_self=True))
            put(mode + " labels", distance.matrix_threshold_clusters(mq, radii[mode][1], mode))
        put("mash", side.within(side, radii["mash"][0], skip_self=True))
        put("mash labels", side.threshold_clusters(radii["mash"][1]))
        put("host", cluster.within(D, 6 / 64, ctx=c))
        put("host labels", cluster.threshold_clusters(D, 5 / 64, ctx=c))
    finally:
        for x in (mq, mr, skq):
            x.close()
    return out


def _fresh(runs, radii):
    c = engine.Context(0)
    try:
        return [_within_and_clusters(c, radii) for _ in range(runs)]
    finally:
        c.close()


def test_within_and_threshold_clusters_on_poisoned_blocks(ctx, monkeypatch):
    """every block the calls take (the strip, the counts and offsets, the pair buffers) full of 0xFF, on a fresh context
    and again on the blocks that run hands back: the bits of the run without the knob"""
    radii = _within_and_clusters(ctx)
    clean, = _fresh(1, radii)
    assert clean["host.row_start"][-1] > 500 and 1 < clean["host labels.n_clusters"] < 257
    assert all(clean[f"{mode}.row_start"][-1] > 100 for mode in ("jsd", "euclidean", "mash"))
    monkeypatch.setenv("DVS_TEST_KNOBS", POISON)
    first, again = _fresh(2, radii)
    assert_same_outputs(first, clean, "poisoned, fresh context")
    assert_same_outputs(again, clean, "poisoned, the first run's blocks again")


# ------------------------------------------------------------------ 9. errors on the device side
def test_sketch_errors_where_the_existing_entries_raise_them(ctx):
    rng = np.random.default_rng(4)
    short = [np.zeros(3, np.uint8), rng.integers(0, 4, 80, dtype=np.uint8), rng.integers(0, 4, 90, dtype=np.uint8)]
    a, b = distance.Sketches(short, 8, 10, ctx=ctx), distance.Sketches(short[::-1], 8, 10, ctx=ctx)
    try:
        sa, sb = distance.DeviceSide(a, "mash"), distance.DeviceSide(b, "mash")
        for rows, other_rows in ((None, None), ([0], [2]), ([1], [0, 0]), ([0], [0]), ([1, 2], [0, 1])):
            try:
                d = a.cross_distances(b, rows, other_rows)
            except ZeroDivisionError:
                with pytest.raises(ZeroDivisionError):
                    sa.within(sb, 0.5, rows, other_rows)
            else:
                assert_within(sa.within(sb, 0.5, rows, other_rows), d, 0.5, what=(rows, other_rows))
        for rows in (None, [0, 1], [1, 2], [2, 1, 1]):
            n = 3 if rows is None else len(rows)
            try:
                a.cluster_scores([0] * n, rows)
            except ZeroDivisionError:
                with pytest.raises(ZeroDivisionError):
                    sa.threshold_clusters(0.5, rows)
            else:
                got = sa.threshold_clusters(2.0, rows)
                assert got.n_clusters == 1 and got.labels.tolist() == [0] * n
        a.k = b.k = 0  # (the k of the distance formula: a division by zero before any device work)
        with pytest.raises(ZeroDivisionError):
            sa.within(sb, 0.5, [1], [0])
        with pytest.raises(ZeroDivisionError):
            sa.threshold_clusters(0.5, [1, 2])
        a.k = b.k = 8
        assert sa.within(sb, 2.0, [1], [0, 1]).index.tolist() == [0, 1]  # the context is usable afterwards
    finally:
        a.close()
        b.close()


def test_c_entries_refuse_bad_arguments_and_leave_the_context_usable(ctx):
    L = ctx._L
    d = tie_matrix(40, 2)
    p = _lib.ptr(d, C.c_double)
    out = C.c_void_p(0xDEAD)
    lab, cnt = np.full(40, 7, np.uint32), C.c_uint32(99)
    big = 65535 * 8 + 1  # one row more than the square entries take (tests/test_gpu_clusters.py, test_gpu_cophenet.py)

    S = distance.make_source

    def given(n, on_device=0, handle=d.ctypes.data):
        """the matrix d (or no matrix) as a caller's n x n matrix"""
        return S(_lib.SRC_GIVEN, handle, n, on_device=on_device)

    def refused(q, r, *args):
        """dvs_within's code, with *out NULL afterwards whatever it held"""
        out.value = 0xDEAD
        rc = L.dvs_within(ctx._h, q, r, *args, C.byref(out))
        assert not out.value, rc
        return rc

    def clusters_refused(src, radius):
        """dvs_threshold_clusters' code, with the labels and the count untouched"""
        lab[:], cnt.value = 7, 99
        rc = L.dvs_threshold_clusters(ctx._h, src, radius, _lib.ptr(lab, C.c_uint32), C.byref(cnt))
        assert (lab == 7).all() and cnt.value == 99, rc
        return rc

    assert refused(given(40), None, float("nan"), 0, 0) == _lib.ERR_VALUE
    assert refused(given(40), None, 0.1, 2, 0) == _lib.ERR_VALUE            # an unknown flag bit
    assert refused(given(40, handle=None), None, 0.1, 0, 0) == _lib.ERR_VALUE
    assert refused(given(40, 1), None, 0.1, 0, 0) == _lib.ERR_VALUE         # a host array is not device memory
    assert refused(given(big), None, 0.1, 0, 0) == _lib.ERR_UNSUPPORTED     # (refused before a cell is read)
    assert L.dvs_within(ctx._h, given(40), None, 0.1, 0, 0, None) == _lib.ERR_VALUE
    assert clusters_refused(given(40), float("nan")) == _lib.ERR_VALUE
    assert clusters_refused(given(40, 1), 0.1) == _lib.ERR_VALUE            # a host array is not device memory
    assert clusters_refused(given(big), 0.1) == _lib.ERR_UNSUPPORTED
    assert L.dvs_threshold_clusters(ctx._h, given(40), 0.1, None, C.byref(cnt)) == _lib.ERR_VALUE
    assert L.dvs_threshold_clusters(ctx._h, given(40), 0.1, _lib.ptr(lab, C.c_uint32), None) == _lib.ERR_VALUE
    assert (lab == 7).all() and cnt.value == 99
    with pytest.raises(NotImplementedError):  # the same through the Python layer: a matrix of `big` rows is never made,
        distance.run_within(ctx, given(big), None, 0.1, 0, 0)                   # the entry refuses the number
    with pytest.raises(NotImplementedError):
        distance.run_threshold_clusters(ctx, given(big), 0.1)
    assert L.dvs_threshold_clusters(ctx._h, given(0), 0.1, None, None) == _lib.OK  # n == 0: nothing written
    assert L.dvs_threshold_clusters(ctx._h, given(1), 0.1, _lib.ptr(lab, C.c_uint32), C.byref(cnt)) == _lib.OK
    assert lab[0] == 0 and cnt.value == 1
    assert L.dvs_within(ctx._h, given(0), None, 0.1, 0, 0, C.byref(out)) == _lib.OK and out.value  # an empty list
    rows, pairs = C.c_uint32(9), C.c_uint64(9)
    assert L.dvs_pairs_info(out, C.byref(rows), C.byref(pairs)) == _lib.OK and (rows.value, pairs.value) == (0, 0)
    L.dvs_pairs_destroy(out)
    m = ctx.build_matrix(_seqs(np.random.default_rng(1), 10), 3, 4)
    other = ctx.build_matrix(_seqs(np.random.default_rng(1), 10), 4, 4)
    try:
        with pytest.raises(ValueError, match="bins"):
            distance.matrix_within(m, other, 0.1)
        many = np.zeros(big, np.uint32)  # row 0, `big` times over: a reference list beyond the square entries' row limit
        u32 = lambda a: _lib.ptr(a, C.c_uint32)  # noqa: E731
        for kind in (_lib.SRC_JSD, _lib.SRC_EUCLIDEAN):
            all10 = S(kind, m._h, 10)
            assert refused(S(kind, m._h, 11), all10, 0.1, 0, 0) == _lib.ERR_VALUE  # more rows than the handle holds
            assert refused(S(kind, m._h, 2, np.array([0, 10], np.uint32)), all10, 0.1, 0, 0) == _lib.ERR_VALUE
            assert refused(all10, S(kind, m._h, big, many), 0.1, 0, 0) == _lib.ERR_UNSUPPORTED
            assert refused(all10, all10, float("nan"), 0, 0) == _lib.ERR_VALUE
            assert refused(all10, S(kind, None, 10), 0.1, 0, 0) == _lib.ERR_VALUE
            lab[:], cnt.value = 7, 99
            f = L.dvs_threshold_clusters
            assert f(ctx._h, S(kind, m._h, big, many), 0.1, u32(np.full(big, 7, np.uint32)), C.byref(cnt)) == _lib.ERR_UNSUPPORTED
            assert f(ctx._h, S(kind, m._h, 11), 0.1, u32(lab), C.byref(cnt)) == _lib.ERR_VALUE
            assert f(ctx._h, all10, float("nan"), u32(lab), C.byref(cnt)) == _lib.ERR_VALUE
            assert (lab == 7).all() and cnt.value == 99
        with pytest.raises(NotImplementedError):
            distance.matrix_within(m, m, 0.1, "jsd", r_rows=many)
        with pytest.raises(NotImplementedError):
            distance.matrix_threshold_clusters(m, 0.1, "euclidean", rows=many)
        sk = distance.Sketches(_seqs(np.random.default_rng(2), 10), 8, 20, ctx=ctx)
        try:
            mash = {"k": 8, "sketch_size": 20}
            all10 = S(_lib.SRC_MASH, sk._h, 10, **mash)
            assert refused(all10, S(_lib.SRC_MASH, sk._h, big, many, **mash), 0.1, 0, 0) == _lib.ERR_UNSUPPORTED
            assert refused(S(_lib.SRC_MASH, sk._h, 11, **mash), all10, 0.1, 0, 0) == _lib.ERR_VALUE
            lab[:], cnt.value = 7, 99
            assert L.dvs_threshold_clusters(ctx._h, S(_lib.SRC_MASH, sk._h, big, many, **mash), 0.1,
                                            u32(np.full(big, 7, np.uint32)), C.byref(cnt)) == _lib.ERR_UNSUPPORTED and cnt.value == 99
        finally:
            sk.close()
        nb = distance.matrix_within(m, m, float("inf"), "jsd", q_rows=[], r_rows=None)
        assert nb.row_start.tolist() == [0] and nb.index.size == 0
        nb = distance.matrix_within(m, m, float("inf"), "jsd", q_rows=[1, 2], r_rows=[])
        assert nb.row_start.tolist() == [0, 0, 0]
        assert distance.matrix_within(m, m, float("inf")).row_start[-1] == 100  # usable afterwards
    finally:
        m.close()
        other.close()
    assert_within(cluster.within(d, 4 / 64, ctx=ctx), d, 4 / 64, True)


def test_the_source_check_refuses_before_any_device_work(ctx):
    """what every entry checks of its dvs_source before anything else (DVS_ERR_VALUE), and the combinations no entry
    serves (DVS_ERR_UNSUPPORTED): the code, a message, and the context usable afterwards.  10 rows at k = 3; every output
    is poisoned and must come back untouched -- nothing was launched, nothing written"""
    L, S = ctx._L, distance.make_source
    u32, f64 = (lambda a: _lib.ptr(a, C.c_uint32)), (lambda a: _lib.ptr(a, C.c_double))
    seqs = _seqs(np.random.default_rng(5), 10)
    m, sk = ctx.build_matrix(seqs, 3, 4), distance.Sketches(seqs, 3, 20, ctx=ctx)
    d = tie_matrix(10, 3)
    other = d.copy()
    rows = np.array([0, 2, 4], np.uint32)
    mash = {"k": 3, "sketch_size": 20}
    jsd, euc, sketches, given = S(_lib.SRC_JSD, m._h, 10), S(_lib.SRC_EUCLIDEAN, m._h, 10), S(_lib.SRC_MASH, sk._h, 10, **mash), \
        S(_lib.SRC_GIVEN, d.ctypes.data, 10)
    dist, idx = np.full((10, 10), 7.0), np.full((10, 10), 7, np.uint32)
    tree = (np.full(18, 7, np.uint32), np.full(9, 7.0), np.full(9, 7, np.uint32))
    nj = (np.full(24, 7, np.uint32), np.full(24, 7.0))
    seeds, cnt, cover = np.zeros(1, np.uint32), C.c_uint32(7), C.c_double(7.0)
    mm = (np.full(10, 7, np.uint32), np.full(10, 7.0), np.full(10, 7, np.uint32), np.full(10, 7.0))
    out = C.c_void_p()

    ops = {  # every entry over one source, or over a (queries, references) pair
        "distances": lambda s: L.dvs_distances(ctx._h, s, f64(dist)),
        "linkage": lambda s: L.dvs_linkage(ctx._h, s, 2, u32(tree[0]), f64(tree[1]), u32(tree[2])),
        "nj": lambda s: L.dvs_nj(ctx._h, s, u32(nj[0]), f64(nj[1])),
        "maxmin": lambda s: L.dvs_maxmin(ctx._h, s, u32(seeds), 1, 3, 0, 0.0, u32(mm[0]), f64(mm[1]), C.byref(cnt), u32(mm[2]),
                                         f64(mm[3]), C.byref(cover)),
        "cluster_scores": lambda s: L.dvs_cluster_scores(ctx._h, s, u32(np.zeros(10, np.uint32)), 1, f64(dist), None, None, None,
                                                         None, None),
        "cophenet": lambda s: L.dvs_cophenet(ctx._h, s, u32(np.zeros(18, np.uint32)), f64(np.zeros(9)), C.byref(cover), None, None),
        "threshold_clusters": lambda s: L.dvs_threshold_clusters(ctx._h, s, 0.1, u32(idx), C.byref(cnt)),
    }
    pair_ops = {
        "cross_distances": lambda q, r: L.dvs_cross_distances(ctx._h, q, r, f64(dist)),
        "nearest": lambda q, r: L.dvs_nearest(ctx._h, q, r, 1, u32(idx), f64(dist)),
        "within": lambda q, r: L.dvs_within(ctx._h, q, r, 0.1, 0, 0, C.byref(out)),
    }

    def refused(rc, code, what):
        assert rc == code, (what, rc)
        assert L.dvs_last_error(ctx._h), what  # a message
        assert (dist == 7.0).all() and (idx == 7).all() and cnt.value == 7 and cover.value == 7.0 and not out.value, what
        assert all((a == 7).all() for a in (*tree, *nj, *mm)), what

    try:
        bad = {"an unknown kind": S(4, m._h, 10), "a null matrix": S(_lib.SRC_JSD, None, 10),
               "null sketches": S(_lib.SRC_MASH, None, 10, **mash), "a null caller's matrix": S(_lib.SRC_GIVEN, None, 10),
               "a caller's matrix with a row list": S(_lib.SRC_GIVEN, d.ctypes.data, 3, rows)}
        for what, src in bad.items():
            for op, call in ops.items():
                refused(call(src), _lib.ERR_VALUE, (op, what))
                refused(call(None), _lib.ERR_VALUE, (op, "no source"))
            for op, call in pair_ops.items():
                refused(call(src, src), _lib.ERR_VALUE, (op, what))
                refused(call(jsd, src), _lib.ERR_VALUE, (op, what, "as the references"))
                refused(call(jsd, None), _lib.ERR_VALUE, (op, "no references"))
        for op, call in pair_ops.items():
            refused(call(jsd, euc), _lib.ERR_VALUE, (op, "jsd against euclidean"))
            refused(call(sketches, jsd), _lib.ERR_VALUE, (op, "mash against jsd"))
            refused(call(given, jsd), _lib.ERR_VALUE, (op, "a caller's matrix against jsd"))
            refused(call(sketches, S(_lib.SRC_MASH, sk._h, 10, k=4, sketch_size=20)), _lib.ERR_VALUE, (op, "another k"))
            refused(call(sketches, S(_lib.SRC_MASH, sk._h, 10, k=3, sketch_size=21)), _lib.ERR_VALUE, (op, "another sketch size"))
        # the combinations no entry has served
        for op in ("distances", "cross_distances", "nearest"):
            rc = ops[op](given) if op in ops else pair_ops[op](given, given)
            refused(rc, _lib.ERR_UNSUPPORTED, (op, "a caller's matrix"))
            assert f"dvs_{op}".encode() in L.dvs_last_error(ctx._h) and b"given" in L.dvs_last_error(ctx._h)
        for kind, handle, extra in ((_lib.SRC_JSD, m._h, {}), (_lib.SRC_EUCLIDEAN, m._h, {}), (_lib.SRC_MASH, sk._h, mash)):
            for op in ("distances", "linkage", "nj"):
                refused(ops[op](S(kind, handle, 3, rows, **extra)), _lib.ERR_UNSUPPORTED, (op, kind, "a row list"))
                refused(ops[op](S(kind, handle, 9, **extra)), _lib.ERR_UNSUPPORTED, (op, kind, "9 rows of 10"))
                assert f"dvs_{op}".encode() in L.dvs_last_error(ctx._h)
            refused(ops["maxmin"](S(kind, handle, 3, rows, **extra)), _lib.ERR_UNSUPPORTED, ("maxmin", kind, "a row list"))
            assert b"dvs_maxmin" in L.dvs_last_error(ctx._h)
        refused(pair_ops["within"](given, S(_lib.SRC_GIVEN, other.ctypes.data, 10)), _lib.ERR_UNSUPPORTED, "within: two matrices")
        assert b"dvs_within" in L.dvs_last_error(ctx._h) and b"given" in L.dvs_last_error(ctx._h)
        # the same context serves valid calls of every kind afterwards
        assert_within(cluster.within(d, 4 / 64, ctx=ctx), d, 4 / 64, True)
        assert pair_ops["within"](given, given) == _lib.OK and out.value  # the same matrix named twice is the matrix against itself
        L.dvs_pairs_destroy(out)
        assert same_bits(distance.matrix_cross_distances(m, m, "jsd"), distance.matrix_jsd_distances(m))  # (every row has k-mers)
        assert np.array_equal(sk.distances(), distance.DeviceSide(sk, "mash").distances())
        assert distance.matrix_maxmin(m, 3, mode="euclidean").picks.size == 3
    finally:
        m.close()
        sk.close()
