"""Canonical k-mer count rows on the device (csrc/canon.hip: dvs_matrix_fold_canonical) against the yardstick of
tests/test_canonical_host.py, which pins it and the cases on the CPU: a numpy fold of `oracle.count_kmers`.

  * the fold: counts and totals bit for bit, entropies within 1e-11 of `oracle.entropy` of the folded frequency row, for
    k = 1 .. 8 (k = 8: rows gathered from global memory), both count widths, 1 / 63 / 64 / 65 / 257 rows, rows without a
    valid k-mer first, inside and last, no rows at all, more rows than the grid has row groups, every build route that
    takes canonical=, and the source matrix left as it was;
  * strand invariance: the same folded bits with a seeded subset of the sequences reverse-complemented;
  * selections over the folded matrix against the oracle's merges over the yardstick's frequency rows (members and
    order exact, floats within 1e-6 relative), delta_jsd of folded queries, and the same through _dvs and the apps;
  * distances of the folded matrix inside the band of tests/test_distance_truth_host.py; canonical= in the functions
    over sequences giving what the folded matrix gives;
  * the same bits on poisoned blocks; the errors, with the context usable after each."""
import ctypes as C

import numpy as np
import pytest

import oracle
from diverseseq_amd import _dvs, apps, cluster, distance, engine
from test_blocks_host import POISON, assert_same_outputs
from test_canonical_host import (C_OF_K, ENTROPY_TOL, MANY_ROWS, N_ROWS, SELECT_KS, SELECT_RTOL, family200, family_queries,
                                 family_reference, fold_counts, folded, folded_freqs, folded_of_counts, many_rows,
                                 plain_counts, ragged, revcomp, strand_subset, with_a_long_row, yardstick_bins)
from test_distance_truth_host import EUCLID_RTOL, tol_derived, truth_euclid_rows, truth_jsd_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_folded(f, ref, k, width, what=""):
    counts, totals, ent = ref
    assert f.is_canonical and f.k == k and f.num_states == 4 and f.count_bytes == width, what
    assert f.nrows == counts.shape[0] and f.nbins == C_OF_K[k - 1] == counts.shape[1], what
    got = f.counts()
    assert got.dtype == np.uint32 and np.array_equal(got, counts), (what, "folded counts differ")
    assert np.array_equal(f.totals(), totals), what
    h = f.entropy()
    worst = float(np.abs(h - ent).max()) if ent.size else 0.0
    print(f"{what}: k = {k}, {f.nrows} rows, worst |H - oracle.entropy| = {worst:.3g}")
    assert worst <= ENTROPY_TOL, what
    assert (_bits(h[totals == 0]) == 0).all(), what  # (+0.0 for a row without a valid k-mer)


def fold_and_check(ctx, seqs, k, width, what):
    """build, fold, hold the fold to the yardstick and the source to what it was before"""
    seqs = list(seqs)
    m = ctx.build_matrix(seqs, k)
    try:
        assert m.count_bytes == width and not m.is_canonical, what
        before = (m.counts(), m.totals(), m.entropy())
        f = m.canonical()
        try:
            assert_folded(f, folded_of_counts(before[0], k), k, width, what)
            assert np.array_equal(before[0], plain_counts(seqs, k)), what
        finally:
            f.close()
        after = (m.counts(), m.totals(), m.entropy())
        assert all((np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all()
                   for a, b in zip(before, after)), (what, "the source matrix changed")
        assert not m.is_canonical
    finally:
        m.close()


# --------------------------------------------------------------------------------------------- the fold
@pytest.mark.parametrize("k,width", [(k, w) for k in range(1, 9) for w in (2, 4) if w == 4 or k <= 6])
def test_fold_against_the_yardstick(ctx, monkeypatch, k, width):
    """k = 2, 4, 6, 8 have palindromes; k <= 4 folds a row per wave, k = 8 gathers from global memory (256 KB rows);
    k = 7 and 8 have 32-bit rows only (count rows beyond 4096 bins always are)"""
    if width == 4:
        monkeypatch.setenv("DVS_COUNTS_U32", "1")
    for n in N_ROWS if k <= 6 else (1, 65):
        fold_and_check(ctx, ragged(n), k, width, f"ragged({n})")


@pytest.mark.parametrize("k", [3, 6])
def test_fold_of_a_row_of_many_tiles(ctx, k):
    """one sequence of 40 000 bases makes every row 32-bit without the switch, and its own row the sum of several
    tiles (global atomics, row_stats_kernel) that the fold waits for"""
    fold_and_check(ctx, with_a_long_row(), k, 4, "with_a_long_row")


@pytest.mark.parametrize("shape", MANY_ROWS, ids=lambda s: f"{s[0]}x{s[1]}-k{s[2]}")
def test_fold_of_more_rows_than_the_grid_has_groups(ctx, shape):
    """the only shapes beyond 300 rows: a workgroup takes a second group of rows only when there are more groups than
    eight workgroups a CU, and stages into LDS the last group's gathers have just left"""
    n, length, k = shape
    fold_and_check(ctx, many_rows(n, length), k, 2, f"many_rows({n}, {length})")


@pytest.mark.parametrize("k", [2, 7])
def test_fold_of_no_rows(ctx, k):
    m = ctx.build_matrix([], k)
    f = m.canonical()
    assert f.nrows == 0 and f.nbins == C_OF_K[k - 1] and f.is_canonical
    assert f.counts().shape == (0, C_OF_K[k - 1]) and f.totals().size == 0 and f.entropy().size == 0
    f.close()
    m.close()
    g = ctx.build_matrix([], k, canonical=True)
    assert g.nrows == 0 and g.is_canonical
    g.close()


def _fasta(seqs) -> bytes:
    return "".join(f">s{i}\n" + "".join("TCAGN"[min(int(c), 4)] for c in s) + "\n" for i, s in enumerate(seqs)).encode()


@pytest.mark.parametrize("route", ["host", "concat", "device", "packed", "seqbatch", "seqbatch_packed"])
def test_every_build_route_takes_canonical(ctx, route):
    k = 5
    seqs = list(ragged(65))
    ref = folded(seqs, k)
    data, offsets = engine.concat(seqs)
    keep = None
    if route == "host":
        f = ctx.build_matrix(seqs, k, canonical=True)
    elif route == "concat":
        f = ctx.build_matrix_concat(data, offsets, k, 4, canonical=True)
    elif route == "device":  # (a device pointer of the library's own: the encoded bases of an ingested batch)
        keep = ctx.encode_fasta(_fasta(seqs))
        f = ctx.build_matrix_device(keep.dev_ptr, keep.offsets, k, canonical=True)
    elif route == "packed":
        keep = ctx.pack_host(data)
        f = ctx.build_matrix_packed(keep, offsets, k, canonical=True)
    else:
        keep = ctx.encode_fasta(_fasta(seqs))
        assert keep.nseq == len(seqs)
        if route == "seqbatch_packed":
            keep.pack()
        f = keep.build_matrix(k, canonical=True)
    try:
        assert_folded(f, ref, k, 2, route)
    finally:
        f.close()
        if hasattr(keep, "close"):
            keep.close()


@pytest.mark.parametrize("width", [2, 4], ids=["u16", "u32"])
@pytest.mark.parametrize("k", [2, 5, 6])
def test_fold_is_strand_invariant(ctx, monkeypatch, k, width):
    if width == 4:
        monkeypatch.setenv("DVS_COUNTS_U32", "1")
    seqs = list(ragged(257))
    flip = strand_subset(len(seqs))
    other = [revcomp(s) if f else s for s, f in zip(seqs, flip)]
    a, b = ctx.build_matrix(seqs, k, canonical=True), ctx.build_matrix(other, k, canonical=True)
    plain_a, plain_b = ctx.build_matrix(seqs, k), ctx.build_matrix(other, k)
    try:
        assert a.count_bytes == width
        assert np.array_equal(a.counts(), b.counts()) and np.array_equal(a.totals(), b.totals())
        assert (_bits(a.entropy()) == _bits(b.entropy())).all()
        assert not np.array_equal(plain_a.counts(), plain_b.counts())
        da, db = distance.matrix_jsd_distances(a), distance.matrix_jsd_distances(b)
        assert (_bits(da) == _bits(db)).all()
    finally:
        for m in (a, b, plain_a, plain_b):
            m.close()


# --------------------------------------------------------------------------------------------- selections
def assert_selection(sel, sr, what):
    labels, deltas, ents, _ = sr.members()
    got = sel.members(with_freqs=False)
    s = sel.summary()
    assert s.size == sr.size and got.positions.tolist() == labels.tolist(), (what, got.positions.tolist(), labels.tolist())
    np.testing.assert_allclose(got.delta_jsd, deltas, rtol=SELECT_RTOL, atol=1e-12, err_msg=what)
    np.testing.assert_allclose(got.entropy, ents, rtol=SELECT_RTOL, atol=1e-12, err_msg=what)
    for name in ("total_jsd", "mean_delta_jsd", "std_delta_jsd", "cov_delta_jsd"):
        want = getattr(sr, name)
        assert abs(getattr(s, name) - want) <= SELECT_RTOL * abs(want) + 1e-12, (what, name, getattr(s, name), want)


@pytest.mark.parametrize("k", SELECT_KS)
def test_selections_over_the_folded_matrix(ctx, k):
    seqs = list(family200())
    f = ctx.build_matrix(seqs, k, canonical=True)
    q = ctx.build_matrix(list(family_queries()), k, canonical=True)
    plain_q = ctx.build_matrix(list(family_queries()), k)
    try:
        sel = f.nmost(10)
        assert_selection(sel, family_reference(k, "nmost"), f"nmost k={k}")
        # delta_jsd of folded queries against the selected set
        sr = family_reference(k, "nmost")
        want = np.array([sr.delta_jsd(row) for row in folded_freqs(list(family_queries()), k)])
        got = sel.delta_jsd(q, np.full(q.nrows, 0xFFFFFFFF, dtype=np.uint32))
        np.testing.assert_allclose(got, want, rtol=SELECT_RTOL, atol=1e-12)
        with pytest.raises(ValueError, match="bins"):  # an unfolded query matrix: the existing refusal
            sel.delta_jsd(plain_q)
        sel.close()
        for stat in ("stdev", "cov"):
            sel = f.max_divergent(5, 30, stat)
            assert_selection(sel, family_reference(k, stat), f"max {stat} k={k}")
            sel.close()
    finally:
        for m in (f, q, plain_q):
            m.close()


@pytest.mark.parametrize("k", SELECT_KS)
def test_selections_through_the_python_layers(k):
    seqs = list(family200())
    names = [f"s{i}" for i in range(len(seqs))]
    store = _dvs.make_zarr_store()
    for name, s in zip(names, seqs):
        store.write(name, s.tobytes())
    sr = family_reference(k, "nmost")
    r = _dvs.nmost_divergent(store, n=10, k=k, seqids=names, canonical=True)
    assert r.canonical and r.record_names == [names[i] for i in sr.members()[0]]
    assert abs(r.total_jsd - sr.total_jsd) <= SELECT_RTOL * sr.total_jsd
    assert len(r.records[0][1]) == C_OF_K[k - 1]
    srm = family_reference(k, "stdev")
    rm = _dvs.max_divergent(store, min_size=5, max_size=30, k=k, seqids=names, canonical=True)
    assert rm.canonical and rm.record_names == [names[i] for i in srm.members()[0]]
    # the merge of two canonical results: the oracle's merge of their rows
    merged = _dvs.final_nmost([r, rm], n=10)
    rows = np.array([rec[1] for res in (r, rm) for rec in res.records])
    ids = [rec[0] for res in (r, rm) for rec in res.records]
    label_of = {}
    labels = np.array([label_of.setdefault(i, len(label_of)) for i in ids], dtype=np.uint32)
    want = oracle.final_nmost(rows, 10, labels=labels)
    first = {lab: i for i, lab in reversed(list(enumerate(labels.tolist())))}
    assert merged.canonical and sorted(merged.record_names) == sorted(ids[first[int(lab)]] for lab in want.members()[0])
    assert abs(merged.total_jsd - want.total_jsd) <= SELECT_RTOL * want.total_jsd
    # the delta-JSD calculator folds its queries
    calc = _dvs.get_delta_jsd_calculator([(names[i], seqs[i].tobytes()) for i in sr.members()[0]], k, canonical=True)
    setref = oracle.SummedRecords.new(folded_freqs([seqs[i] for i in sr.members()[0]], k))
    for j, (qseq, row) in enumerate(zip(family_queries(), folded_freqs(list(family_queries()), k))):
        got = calc.delta_jsd(f"q{j}", qseq.tobytes())
        assert abs(got - setref.delta_jsd(row)) <= SELECT_RTOL * abs(setref.delta_jsd(row)) + 1e-12
    assert calc.get_result().canonical
    # the app: the reference's seeded shuffle of the ids, then the same selection
    order = list(names)
    np.random.default_rng(3).shuffle(order)
    at = {name: i for i, name in enumerate(names)}
    want_app = oracle.final_nmost(folded_freqs([seqs[at[name]] for name in order], k), 10)
    picked = apps.dvs_nmost(n=10, k=k, seed=3, canonical=True).main(dict(zip(names, seqs)))
    assert set(picked) == {order[i] for i in want_app.members()[0]}
    name, delta = apps.dvs_delta_jsd({names[i]: seqs[i] for i in sr.members()[0]}, k=k, canonical=True).main(
        ("q", family_queries()[4]))
    assert abs(delta - setref.delta_jsd(folded_freqs([family_queries()[4]], k)[0])) <= SELECT_RTOL


# --------------------------------------------------------------------------------------------- distances
@pytest.mark.parametrize("width", [2, 4], ids=["u16", "u32"])
@pytest.mark.parametrize("k", [3, 6])
def test_distances_of_the_folded_matrix_against_the_truth(ctx, monkeypatch, k, width):
    """the band of tests/test_distance_truth_host.py: a JSD cell within tol_derived(nbins) of the long-double truth, a
    euclidean cell within 1e-12 relative, the truth taken over the yardstick's folded counts"""
    if width == 4:
        monkeypatch.setenv("DVS_COUNTS_U32", "1")
    seqs = list(ragged(65))
    counts, totals, _ = folded(seqs, k)
    live = np.flatnonzero(totals > 0)
    pairs = np.array([(i, j) for a, i in enumerate(live) for j in live[a + 1:]])
    f = ctx.build_matrix(seqs, k, canonical=True)
    try:
        assert f.count_bytes == width
        dj, de = distance.matrix_jsd_distances(f), distance.matrix_euclidean_distances(f)
    finally:
        f.close()
    err = np.abs(dj[pairs[:, 0], pairs[:, 1]].astype(np.longdouble) - truth_jsd_rows(counts, pairs))
    print(f"k = {k}: {len(pairs)} cells, worst |jsd - truth| = {float(err.max()):.3g}, bound {tol_derived(counts.shape[1]):.3g}")
    assert float(err.max()) <= tol_derived(counts.shape[1])
    truth = truth_euclid_rows(counts, pairs)
    rel = np.abs(de[pairs[:, 0], pairs[:, 1]].astype(np.longdouble) - truth) / truth
    print(f"k = {k}: worst relative |euclid - truth| = {float(rel.max()):.3g}")
    assert (truth > 0).all() and float(rel.max()) <= EUCLID_RTOL
    dead = np.flatnonzero(totals == 0)
    off = ~np.eye(len(seqs), dtype=bool)
    assert np.isnan(dj[dead][:, live]).all() and not np.isnan(dj[np.ix_(live, live)]).any() and (dj[~off] == 0).all()


def test_canonical_keyword_is_the_folded_matrix(ctx):
    k = 4
    seqs = [s for s in ragged(65) if oracle.count_kmers(s, 4, k).sum()]  # (a tree refuses rows without a valid k-mer)
    queries = [s for s in ragged(63, 2) if oracle.count_kmers(s, 4, k).sum()][:20]
    f, fq = ctx.build_matrix(seqs, k, canonical=True), ctx.build_matrix(queries, k, canonical=True)
    plain = ctx.build_matrix(seqs, k)
    try:
        for mode in ("jsd", "euclidean"):
            side = distance.DeviceSide(f, mode)
            square = distance.MODES[mode][0](seqs, k, ctx=ctx, canonical=True)
            assert (_bits(square) == _bits(side.distances())).all()
            cross = distance.cross_distances(queries, seqs, mode, k=k, ctx=ctx, canonical=True)
            assert (_bits(cross) == _bits(distance.matrix_cross_distances(fq, f, mode))).all()
            idx, dist = distance.nearest(queries, seqs, 3, mode, k=k, ctx=ctx, canonical=True)
            widx, wdist = distance.matrix_nearest(fq, f, 3, mode)
            assert np.array_equal(idx, widx) and (_bits(dist) == _bits(wdist)).all()
            z = distance.MODES[mode][1](seqs, k, method="average", ctx=ctx, canonical=True)
            assert np.array_equal(z, side.linkage("average"))
            mm = distance.maxmin(seqs, 6, mode, k=k, ctx=ctx, canonical=True)
            want = distance.matrix_maxmin(f, 6, mode=mode)
            assert np.array_equal(mm.picks, want.picks) and (_bits(mm.dist) == _bits(want.dist)).all()
            tree = distance.NJ_MODES[mode](seqs, k, ctx=ctx, canonical=True)
            assert np.array_equal(tree.children, side.nj().children)
            labels = np.arange(len(seqs)) % 4
            sc = distance.cluster_scores(seqs, labels, mode, k=k, ctx=ctx, canonical=True)
            assert (_bits(sc.within) == _bits(side.cluster_scores(labels).within)).all()
            co = distance.cophenet(seqs, z, mode, k=k, ctx=ctx, canonical=True)
            assert _bits(co.correlation) == _bits(side.cophenet(z).correlation)
        # one side folded and one not: the existing refusal on unequal nbins
        with pytest.raises(ValueError, match="nbins|bins"):
            distance.matrix_cross_distances(plain, f, "jsd")
        # the tree entry points and apps over sequences
        named = {f"s{i}": s for i, s in enumerate(seqs)}
        z = distance.DeviceSide(f, "jsd").linkage("average")
        newick = cluster.ctree(named, k=k, sketch_size=None, distance_mode="jsd", canonical=True)
        assert newick == cluster.linkage_to_newick(list(named), z)
        assert newick != cluster.ctree(named, k=k, sketch_size=None, distance_mode="jsd")
        assert apps.dvs_ctree(k=k, sketch_size=None, distance_mode="jsd", canonical=True).main(named) == newick
        assert cluster.ctree_clusters(named, n_clusters=3, k=k, sketch_size=None, distance_mode="jsd", canonical=True)[0] == newick
        assert cluster.ctree_cophenet(named, k=k, sketch_size=None, distance_mode="jsd", canonical=True)[0] == newick
        both = cluster.compare_linkages(named, ("average",), k=k, sketch_size=None, distance_mode="jsd", canonical=True)
        assert np.array_equal(both["average"][0], z)
        text, tree = cluster.nj_tree(named, k=k, sketch_size=None, distance_mode="jsd", canonical=True)
        assert np.array_equal(tree.children, distance.DeviceSide(f, "jsd").nj().children)
        names, d = apps.dvs_dist("jsd", k=k, sketch_size=None, canonical=True).main(named)
        assert (_bits(d) == _bits(distance.matrix_jsd_distances(f))).all()
    finally:
        for m in (f, fq, plain):
            m.close()


# --------------------------------------------------------------------------------------------- blocks
def _fold_then_select(c):
    k = 4
    f = c.build_matrix(list(family200()), k, canonical=True)
    q = c.build_matrix(list(family_queries()), k, canonical=True)
    sel = f.nmost(10)
    mem = sel.members()
    out = {"counts": f.counts(), "totals": f.totals(), "entropy": f.entropy(), "positions": mem.positions,
           "delta_jsd": mem.delta_jsd, "kfreqs": mem.kfreqs, "total_jsd": np.array([sel.summary().total_jsd]),
           "query_delta": sel.delta_jsd(q, np.full(q.nrows, 0xFFFFFFFF, dtype=np.uint32)),
           "wide_counts": None}
    wide = c.build_matrix(list(ragged(5)), 8, canonical=True)  # (the rows gathered from global memory)
    out["wide_counts"] = wide.counts()
    for h in (sel, q, f, wide):
        h.close()
    return out


def _fresh(runs):
    c = engine.Context(0)
    try:
        return [_fold_then_select(c) for _ in range(runs)]
    finally:
        c.close()


def test_fold_then_select_on_poisoned_blocks(monkeypatch):
    """every block the fold takes (the folded rows, totals, entropies, the table of representatives) full of 0xFF, on a
    fresh context and again on the blocks that run hands back: the bits of the run without the knob"""
    clean, = _fresh(1)
    assert np.array_equal(clean["counts"], folded(list(family200()), 4)[0])
    monkeypatch.setenv("DVS_TEST_KNOBS", POISON)
    first, again = _fresh(2)
    assert_same_outputs(first, clean, "poisoned, fresh context")
    assert_same_outputs(again, clean, "poisoned, the first run's blocks again")


# --------------------------------------------------------------------------------------------- errors
def test_fold_refusals_leave_the_context_usable(ctx):
    seqs = list(ragged(5))
    ref = folded(seqs, 3)
    L = ctx._L

    def still_works():
        f = ctx.build_matrix(seqs, 3, canonical=True)
        assert_folded(f, ref, 3, 2, "after a refusal")
        f.close()

    m = ctx.build_matrix(seqs, 3)
    out = C.c_void_p()
    for args in ((None, m._h, C.byref(out)), (ctx._h, None, C.byref(out)), (ctx._h, m._h, None)):
        assert L.dvs_matrix_fold_canonical(*args) == 1  # DVS_ERR_VALUE
        still_works()
    assert "null argument" in L.dvs_last_error(ctx._h).decode()
    freqs = ctx.matrix_from_freqs(np.full((3, 16), 1 / 16))
    with pytest.raises(ValueError, match="frequency matrix"):
        freqs.canonical()
    still_works()
    five = ctx.build_matrix([np.array([0, 1, 2, 3, 4, 0, 1], np.uint8)] * 3, 2, 5)
    with pytest.raises(ValueError, match="four states"):
        five.canonical()
    still_works()
    f = m.canonical()
    with pytest.raises(ValueError, match="already canonical"):
        f.canonical()
    still_works()
    assert L.dvs_matrix_is_canonical(None) == 0
    for h in (m, freqs, five, f):
        h.close()
