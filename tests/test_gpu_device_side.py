"""One distance.DeviceSide serving every one of its fifteen operations over the distances of a batch, one after another,
on the GPU: each result the bits of the public function of the mode for the same sequences, for a side that owns its
handle and for one that wraps a count matrix or the sketches of the caller's -- whose own methods, where `Sketches` has
one, give the same bits again.  The batch is 35 ragged sequences: two 32-row tiles with a ragged edge."""
import numpy as np
import pytest

from diverseseq_amd import cluster, distance, engine

pytestmark = pytest.mark.gpu

N, K, SKETCH = 35, 4, 20
KW = {"mash": dict(k=K, sketch_size=SKETCH), "euclidean": dict(k=K), "jsd": dict(k=K)}


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def seqs():
    rng = np.random.default_rng(35)
    return [rng.integers(0, 4, int(n), dtype=np.uint8) for n in rng.integers(60, 121, N)]


def same_bits(got, want, what):
    """every array of two results (an array, or a tuple of arrays, floats and None) bit for bit"""
    if isinstance(got, np.ndarray):
        got, want = (got,), (want,)
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None, (what, i)
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i)
        assert g.tobytes() == w.tobytes(), (what, i)


def serve_everything(dev, seqs, mode, ctx, what, sketches=None):
    """all fifteen operations of `dev`, each against the function over sequences of the mode; sketches: the
    `distance.Sketches` that `dev` wraps, whose own methods must give the same bits"""
    args = distance.mode_args(mode, K, KW[mode].get("sketch_size"), 4, False)

    def also(name, got, *a, **kw):
        if sketches is not None:
            same_bits(got, getattr(sketches, name)(*a, **kw), f"{what} Sketches.{name}")

    assert dev.mode == mode and dev.n == N and dev.ctx is ctx
    d = dev.distances()
    same_bits(d, distance.MODES[mode][0](seqs, *args, ctx=ctx), f"{what} distances")
    also("distances", d)
    Z = dev.linkage("average")
    same_bits(Z, distance.MODES[mode][1](seqs, *args, method="average", ctx=ctx), f"{what} linkage")
    also("linkage", Z, "average")
    labels = cluster.cut_tree(Z, n_clusters=3)
    assert labels.max() >= 1  # (a cut never separates merges of equal height: two clusters at least here)
    scores = dev.cluster_scores(labels)
    same_bits(scores, distance.cluster_scores(seqs, labels, mode, ctx=ctx, **KW[mode]), f"{what} cluster_scores")
    also("cluster_scores", scores, labels)
    coph = dev.cophenet(Z)
    same_bits(coph, distance.cophenet(seqs, Z, mode, ctx=ctx, **KW[mode]), f"{what} cophenet")
    also("cophenet", coph, Z)
    same_bits(dev.nj(), distance.NJ_MODES[mode](seqs, *args, ctx=ctx), f"{what} nj")
    picks = dev.maxmin(5)
    same_bits(picks, distance.MAXMIN_MODES[mode](seqs, *args, n_select=5, ctx=ctx), f"{what} maxmin")
    also("maxmin", picks, 5)
    cross = dev.cross_distances(dev)
    same_bits(cross, distance.CROSS_MODES[mode][0](seqs, seqs, *args, ctx=ctx), f"{what} cross_distances")
    also("cross_distances", cross, sketches)
    off = ~np.eye(N, dtype=bool)
    assert not np.isnan(d).any()
    same_bits(cross[off], d[off], f"{what} cross_distances against distances")
    near = dev.nearest(dev, 2)
    same_bits(near, distance.CROSS_MODES[mode][1](seqs, seqs, 2, *args, ctx=ctx), f"{what} nearest")
    also("nearest", near, sketches, 2)
    radius = float(np.median(d[off]))
    close = dev.within(dev, radius, skip_self=True)
    assert 0 < close.index.size < N * (N - 1)  # (the median: about half of the pairs, from both of their ends)
    same_bits(close, distance.neighbours(seqs, radius, mode, ctx=ctx, **KW[mode]), f"{what} within")
    also("within", close, sketches, radius, skip_self=True)
    groups = dev.threshold_clusters(radius)
    same_bits(groups, distance.threshold_clusters(seqs, radius, mode, ctx=ctx, **KW[mode]), f"{what} threshold_clusters")
    also("threshold_clusters", groups, radius)
    fit = dev.pcoa(2)
    same_bits(fit, distance.PCOA_MODES[mode](seqs, *args, n_axes=2, ctx=ctx), f"{what} pcoa")
    same_bits(dev.pcoa_project(fit, dev), distance.pcoa_project(fit, seqs, seqs, mode, ctx=ctx, **KW[mode]),
              f"{what} pcoa_project")
    medoids = dev.kmedoids(3)
    same_bits(medoids, distance.KMEDOIDS_MODES[mode](seqs, *args, n_medoids=3, ctx=ctx), f"{what} kmedoids")
    also("kmedoids", medoids, 3)
    same_bits(dev.mst(), distance.MST_MODES[mode](seqs, *args, ctx=ctx), f"{what} mst")
    grouping = [i % 3 for i in range(N)]
    test = dev.permanova(grouping, permutations=19, seed=1)
    same_bits(test, distance.PERMANOVA_MODES[mode](seqs, *args, grouping=grouping, permutations=19, seed=1, ctx=ctx),
              f"{what} permanova")
    also("permanova", test, grouping, permutations=19, seed=1)
    same_bits(dev.distances(), d, f"{what} distances, again")  # (the handle is as it was)


@pytest.mark.parametrize("mode", ["mash", "euclidean", "jsd"])
def test_one_owning_side_serves_every_operation(ctx, seqs, mode):
    args = distance.mode_args(mode, K, KW[mode].get("sketch_size"), 4, False)
    with distance.device_side(seqs, mode, *args, ctx=ctx) as dev:
        handle = dev.handle
        serve_everything(dev, seqs, mode, ctx, f"{mode} owning")
    assert not handle._h  # closed with the side


@pytest.mark.parametrize("mode", ["euclidean", "jsd"])
def test_a_wrapping_side_leaves_the_matrix_to_its_owner(ctx, seqs, mode):
    m = ctx.build_matrix(seqs, K)
    try:
        totals = m.totals()
        with distance.DeviceSide(m, mode) as dev:
            serve_everything(dev, seqs, mode, ctx, f"{mode} wrapping")
        dev.close()
        assert m._h and np.array_equal(m.totals(), totals)  # still usable
        assert np.array_equal(totals, [s.size - K + 1 for s in seqs])
    finally:
        m.close()


def test_a_wrapping_side_leaves_the_sketches_to_their_owner(ctx, seqs):
    sk = distance.Sketches(seqs, K, SKETCH, ctx=ctx)
    try:
        before = sk.to_host()
        with distance.DeviceSide(sk, "mash") as dev:
            serve_everything(dev, seqs, "mash", ctx, "mash wrapping", sketches=sk)
        assert sk._h
        same_bits(sk.to_host(), before, "the sketches after the wrapper is closed")
    finally:
        sk.close()
