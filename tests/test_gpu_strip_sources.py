"""The one seam between a source and a consumer of its distances strip by strip (csrc/crossdist.hip, the strip driver;
the consumers in csrc/nearest.hip, pcoa.hip, clusters.hip, cophenet.hip and within.hip): the twin of
tests/test_gpu_square_sources.py.  The seven entries give the same bits whatever the strip height -- 7 rows (ten
strips, the last of two rows), 32 (three strips, the last of one row) or no limit (one strip) -- from every kind of
source they take: mash, euclidean, jsd; the last four also a caller's matrix on the host or on the device.  The handle
sources are also run with a query and a reference list of 33 rows in no order.  A call an entry refuses raises what it
always raised and leaves the context serving the next one.

m = n = 65: one row past two 32-row tiles and one past a wavefront.  Row 11 of the sequences is a copy of row 5: a zero
off the diagonal, and a tie.  Every entry is called through one function, `call`, with the sources the case makes; the
tree, the labels and the fit are fixed tables of the test's own (a caterpillar tree over a shuffled leaf order, labels
i * 7 % 4, a seeded fit with one axis of negative eigenvalue): any well-formed input shows a strip seam."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from diverseseq_amd import _lib, distance, engine
from test_blocks_host import assert_same_outputs, seqs257

pytestmark = pytest.mark.gpu

N = 65
MODES = {"mash": (6, 400, 4, False), "euclidean": (3, 4), "jsd": (3, 4)}  # (mash at k = 12: every distance but one is 1)
ENTRIES = ("cross_distances", "nearest", "pcoa_project", "cluster_scores", "cophenet", "within", "threshold_clusters")
TAKE_GIVEN = ENTRIES[3:]
SQUARE = ("cluster_scores", "cophenet", "threshold_clusters")  # one source: queries = references
STRIPS = (7, 32)
Q_ROWS = np.random.default_rng(33).permutation(N)[:33].astype(np.uint32)
R_ROWS = np.random.default_rng(34).permutation(N)[:33].astype(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def tables(n: int) -> types.SimpleNamespace:
    """what the entries take beside their sources, for n reference rows"""
    rng = np.random.default_rng(n)
    leaves = rng.permutation(n)
    Z = np.zeros((n - 1, 4))
    for i in range(n - 1):  # a caterpillar: leaf leaves[i + 1] joins everything before it at height i + 1
        Z[i] = (leaves[0] if i == 0 else n + i - 1, leaves[i + 1], (i + 1) / 64, i + 2)
    pairs, heights = distance.check_linkage_matrix(Z, n)
    return types.SimpleNamespace(
        pairs=pairs, heights=heights, labels=distance.check_labels(np.arange(n) * 7 % 4, n),
        values=np.array([2.0, 0.5, -0.25]), vectors=np.ascontiguousarray(rng.normal(size=(n, 3))), row_means=rng.random(n))


def call(ctx, entry, q, r, radius, *, kk=5, max_pairs=0) -> dict:
    """the entry over the sources q, r (r is q for the entries that take one source) -> its outputs"""
    L, f64, u32 = ctx._L, C.c_double, C.c_uint32
    m, n = q.n, r.n
    t = tables(n)
    if entry == "cross_distances":
        dist = np.zeros((m, n))
        ctx.check(L.dvs_cross_distances(ctx._h, q, r, _lib.ptr(dist, f64)))
        return {"dist": dist}
    if entry == "nearest":
        idx, dist = np.zeros((m, kk), dtype=np.uint32), np.zeros((m, kk))
        ctx.check(L.dvs_nearest(ctx._h, q, r, kk, _lib.ptr(idx, u32), _lib.ptr(dist, f64)))
        return {"idx": idx, "dist": dist}
    if entry == "pcoa_project":
        coords = np.zeros((m, 3))
        ctx.check(L.dvs_pcoa_project(ctx._h, q, r, 3, _lib.ptr(t.values, f64), _lib.ptr(t.vectors, f64),
                                     _lib.ptr(t.row_means, f64), _lib.ptr(coords, f64)))
        return {"coords": coords}
    if entry == "cluster_scores":
        return distance.run_cluster_scores(ctx, q, t.labels)._asdict()
    if entry == "cophenet":
        return distance.run_cophenet(ctx, q, t.pairs, t.heights, True)._asdict()
    if entry == "within":
        return distance.run_within(ctx, q, r, radius, 0, max_pairs)._asdict()
    return distance.run_threshold_clusters(ctx, q, radius)._asdict()


def given(d, on_device: int = 0) -> _lib.Source:
    """a caller's matrix as a source: a host array, or a device tensor"""
    if on_device:
        return distance.make_source(_lib.SRC_GIVEN, d.data_ptr(), N, on_device=1, keep=d)
    return distance.make_source(_lib.SRC_GIVEN, d.ctypes.data, N, keep=d)


@pytest.fixture(scope="module")
def world(ctx):
    """mode -> (the side, its `distances()`, a radius half of its cells are within, one a fiftieth are: the threshold
    clusters'), and the one-strip results as they are first computed"""
    sides = {}
    for mode, args in MODES.items():
        side = distance.device_side(list(seqs257(True)[:N]), mode, *args, ctx=ctx)
        d = side.distances()
        d.setflags(write=False)
        above = d[np.triu_indices(N, 1)]
        sides[mode] = (side, d, float(np.median(above)), float(np.quantile(above, 0.02)))

    def sources(mode, listed):
        side = sides[mode][0]
        if not listed:
            return side._source(), side._source()
        return side._source((Q_ROWS, Q_ROWS.size)), side._source((R_ROWS, R_ROWS.size))

    def run(entry, mode, listed=False):
        q, r = sources(mode, listed)
        return call(ctx, entry, r if entry in SQUARE else q, r, sides[mode][3 if entry == "threshold_clusters" else 2])

    first = functools.lru_cache(maxsize=None)(run)
    yield types.SimpleNamespace(sides=sides, run=run, first=first)
    for side, *_ in sides.values():
        side.close()


def test_the_inputs_are_what_the_cases_need(world):
    for mode, (side, d, radius, low) in world.sides.items():
        assert d.shape == (N, N) and np.isfinite(d).all() and d[11, 5] == 0.0 and d[5, 11] == 0.0, mode
        assert np.array_equal(d[11, :5], d[5, :5]) and radius > low > 0.0, mode  # (the tie)
        got = world.first("threshold_clusters", mode)
        assert 1 < got["n_clusters"] < N and 0 < world.first("within", mode)["row_start"][-1] < N * N, mode
    assert sorted(Q_ROWS.tolist()) != Q_ROWS.tolist() and sorted(R_ROWS.tolist()) != R_ROWS.tolist()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("entry", ENTRIES)
def test_strip_heights_agree(ctx, world, monkeypatch, entry, mode):
    import torch

    side, d, radius, low = world.sides[mode]
    cases = {"handle": lambda: world.run(entry, mode), "handle, row lists": lambda: world.run(entry, mode, True)}
    if entry in TAKE_GIVEN:
        host, device = given(np.ascontiguousarray(d)), given(torch.from_numpy(d.copy()).to("cuda:0"), 1)
        torch.cuda.synchronize()
        r = low if entry == "threshold_clusters" else radius
        cases["host matrix"] = lambda: call(ctx, entry, host, host, r)
        cases["device matrix"] = lambda: call(ctx, entry, device, device, r)
    want = {name: run() for name, run in cases.items()}  # no knob: one strip
    assert_same_outputs(want["handle"], world.first(entry, mode), (entry, mode, "twice"))
    if entry in TAKE_GIVEN:  # the handle's matrix is the caller's: the same cells, off the diagonal (`within` reads it)
        assert_same_outputs(want["device matrix"], want["host matrix"], (entry, mode, "host and device"))
        if entry in SQUARE:
            assert_same_outputs(want["host matrix"], want["handle"], (entry, mode, "host and handle"))
    for strip in STRIPS:
        monkeypatch.setenv("DVS_CROSS_STRIP_ROWS", str(strip))
        for name, run in cases.items():
            assert_same_outputs(run(), want[name], (entry, mode, name, strip))


def refusals(ctx, world):
    """name -> (the entries it is tried on, the exception, its message, the call).  A host pointer said to be device
    memory: the runtime either refuses the pointer or reports it as host memory, device -2 -- dvs_given_on_device's two
    messages, as in tests/test_gpu_square_sources.py"""
    side, d, radius, _ = world.sides["jsd"]
    host = np.ascontiguousarray(d)
    whole = side._source()
    other = np.ascontiguousarray(d.T.copy())
    bad_rows = Q_ROWS.copy()
    bad_rows[20] = N
    listed = side._source((bad_rows, bad_rows.size))
    return {
        "a caller's matrix": (ENTRIES[:3], NotImplementedError, "dvs_{entry}: the matrix of a given source",
                              lambda e: call(ctx, e, given(host), given(host), radius)),
        "another matrix as references": (("within",), NotImplementedError,
                                         "dvs_within: another matrix as the references of a given source",
                                         lambda e: call(ctx, e, given(host), given(other), radius)),
        "n_nearest = 65": (("nearest",), NotImplementedError, "65 nearest: 64 at most",
                           lambda e: call(ctx, e, whole, whole, radius, kk=65)),
        "a row-list entry equal to n": (ENTRIES, ValueError, f"row list: entry 20 is row {N} of a handle that holds {N}",
                                        lambda e: call(ctx, e, listed, listed if e in SQUARE else whole, radius)),
        "a host pointer as a device matrix": (TAKE_GIVEN, ValueError,
                                              "the distance matrix is (not device memory|on device -?[0-9]+, the context)",
                                              lambda e: call(ctx, e, *[distance.make_source(
                                                  _lib.SRC_GIVEN, host.ctypes.data, N, on_device=1, keep=host)] * 2, radius)),
        "max_pairs = 1": (("within",), NotImplementedError, "more than max_pairs = 1",
                          lambda e: call(ctx, e, whole, whole, radius, max_pairs=1)),
    }


@pytest.mark.parametrize("name", ["a caller's matrix", "another matrix as references", "n_nearest = 65",
                                  "a row-list entry equal to n", "a host pointer as a device matrix", "max_pairs = 1"])
def test_a_refusal_leaves_the_context_usable(ctx, world, name):
    entries, exc, message, refused = refusals(ctx, world)[name]
    for entry in entries:
        with pytest.raises(exc, match=message.format(entry=entry)):
            refused(entry)
        assert_same_outputs(world.run(entry, "jsd"), world.first(entry, "jsd"), (entry, "behind", name))
