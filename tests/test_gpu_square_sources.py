"""The one seam between a source and a consumer of its whole n x n matrix (csrc/rowdist.hip, the square driver): the
linkage tree, the neighbour-joining tree, the principal coordinates and k-medoids give the same bits whichever way the
matrix arrives -- measured by the library from a mash, euclidean or jsd source, uploaded from the caller's host array,
or used where it is in the caller's device memory -- and a call the driver refuses leaves the context serving the next
one.

n = 65: one row past two 32-row tiles and one past a wavefront.  Row 11 of the sequences is a copy of row 5: a zero off
the diagonal, and a tie.  Results only are compared (tests/test_blocks_host.py assert_same_outputs): no work counters,
nothing of PCoA's or k-medoids' info.

mash: the staged arrival runs the stage's kernel, `distances()` the pair kernel on the caller's diagonal.  On the
commit before the driver the four consumers gave the same bits over either (these 65 rows, and the first 257), so mash
is in the staged comparison too."""
import functools

import numpy as np
import pytest

from diverseseq_amd import _lib, cluster, distance, engine
from test_blocks_host import assert_same_outputs, seqs257

pytestmark = pytest.mark.gpu

N = 65
MODES = {"mash": (12, 400, 4, False), "euclidean": (3, 4), "jsd": (3, 4)}
CONSUMERS = ("linkage", "nj", "pcoa", "kmedoids")
BIG = 200_000  # 320 GB of matrix: more than the device holds (tests/test_gpu_kmedoids.py)


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def _tree(t) -> dict:
    return {"children": t.children, "lengths": t.lengths}


def _fit(f) -> dict:
    return {name: getattr(f, name) for name in ("values", "vectors", "coordinates", "residuals", "row_means")}


def _medoids(r) -> dict:
    return {name: getattr(r, name) for name in ("medoids", "labels", "dist", "second", "swaps", "td")}


def staged(side, consumer) -> dict:
    """the consumer over the side's own source"""
    if consumer == "linkage":
        return {"Z": side.linkage("average")}
    if consumer == "nj":
        return _tree(side.nj())
    if consumer == "pcoa":
        return _fit(side.pcoa(2, strict=False))
    return _medoids(side.kmedoids(3, init="build"))


def given(ctx, consumer, d) -> dict:
    """the consumer over a caller's matrix: a host array, or a device tensor (the two trees overwrite theirs)"""
    if consumer == "linkage":
        return {"Z": cluster.linkage(d, "average", ctx=ctx)}
    if consumer == "nj":
        return _tree(cluster.neighbor_joining(d, ctx=ctx))
    if consumer == "pcoa":
        return _fit(cluster.pcoa(d, 2, strict=False, ctx=ctx))
    return _medoids(cluster.kmedoids(d, 3, init="build", ctx=ctx))


def raw_given(ctx, consumer, src, n):
    """the same calls over a dvs_source of the test's making"""
    if consumer == "linkage":
        return distance.run_linkage(ctx, src, distance.linkage_method_code("average"))
    if consumer == "nj":
        return distance.run_nj(ctx, src)
    if consumer == "pcoa":
        return distance.run_pcoa(ctx, src, 2, 1e-8, 0, False)
    return distance.run_kmedoids(ctx, src, 3, None, 300)


@pytest.fixture(scope="module")
def arrivals(ctx):
    """mode -> (the side, its `distances()`), and the staged results as they are first computed"""
    sides = {}
    for mode, args in MODES.items():
        side = distance.device_side(list(seqs257(True)[:N]), mode, *args, ctx=ctx)
        d = side.distances()
        d.setflags(write=False)
        sides[mode] = (side, d)
    first = functools.lru_cache(maxsize=None)(lambda mode, consumer: staged(sides[mode][0], consumer))
    yield sides, first
    for side, _ in sides.values():
        side.close()


def test_the_inputs_are_what_the_cases_need(arrivals):
    sides, _ = arrivals
    for mode, (side, d) in sides.items():
        assert d.shape == (N, N) and np.isfinite(d).all() and d[11, 5] == 0.0 and d[5, 11] == 0.0, mode
        assert np.array_equal(d[11, :5], d[5, :5]), mode  # (the tie)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("consumer", CONSUMERS)
def test_arrivals_agree(ctx, arrivals, consumer, mode):
    import torch

    sides, first = arrivals
    d = sides[mode][1]
    want = first(mode, consumer)
    assert_same_outputs(given(ctx, consumer, d), want, (consumer, mode, "host"))
    on_device = torch.from_numpy(d.copy()).to("cuda:0")  # (a fresh copy each time: the two trees overwrite it)
    assert_same_outputs(given(ctx, consumer, on_device), want, (consumer, mode, "device"))


@pytest.mark.parametrize("consumer", CONSUMERS)
def test_a_refusal_leaves_the_context_usable(ctx, arrivals, consumer):
    sides, first = arrivals
    side, d = sides["jsd"]
    want = first("jsd", consumer)
    host = np.ascontiguousarray(d)
    # DVS_ERR_VALUE from the pointer check (either of its two refusals): a host pointer said to be device memory
    with pytest.raises(ValueError, match="the distance matrix is (not device memory|on device)"):
        raw_given(ctx, consumer, distance.make_source(_lib.SRC_GIVEN, host.ctypes.data, N, on_device=1, keep=host), N)
    assert_same_outputs(staged(side, consumer), want, (consumer, "behind DVS_ERR_VALUE"))
    with pytest.raises(MemoryError):  # DVS_ERR_NOMEM; the pointer is never read
        raw_given(ctx, consumer, distance.make_source(_lib.SRC_GIVEN, host.ctypes.data, BIG, keep=host), BIG)
    assert_same_outputs(staged(side, consumer), want, (consumer, "behind DVS_ERR_NOMEM"))
