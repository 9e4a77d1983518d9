"""distance.DeviceSide without a GPU and without a call into the library: who closes the handle and when, over stand-in
handles in the style of test_cross_host's `_Matrix`."""
import numpy as np
import pytest

from diverseseq_amd import distance
from test_cross_host import _NoContext


class _Handle:
    """stands in for a Sketches or a count matrix: counts its close() calls"""
    ctx = _NoContext()
    n = nrows = 5

    def __init__(self):
        self.closed = 0

    def close(self):
        self.closed += 1


SEQS = [np.arange(30, dtype=np.uint8) % 4 for _ in range(3)]


@pytest.mark.parametrize("mode", ["mash", "euclidean", "jsd"])
def test_an_owning_side_closes_its_handle_exactly_once(mode):
    h = _Handle()
    dev = distance.DeviceSide(h, mode, owns=True)
    assert dev.mode == mode and dev.n == 5 and dev.ctx is h.ctx and dev.handle is h
    assert h.closed == 0
    for _ in range(3):
        dev.close()
        assert h.closed == 1


@pytest.mark.parametrize("mode", ["mash", "euclidean", "jsd"])
def test_a_wrapping_side_never_closes_the_handle(mode):
    h = _Handle()
    dev = distance.DeviceSide(h, mode)
    dev.close()
    with distance.DeviceSide(h, mode) as again:
        assert again.handle is h
    dev.close()
    assert h.closed == 0


def test_leaving_a_with_block_closes_the_side():
    h = _Handle()
    with distance.DeviceSide(h, "jsd", owns=True) as dev:
        assert h.closed == 0
    assert h.closed == 1
    dev.close()
    assert h.closed == 1
    h = _Handle()
    with pytest.raises(KeyError):
        with distance.DeviceSide(h, "mash", owns=True):
            raise KeyError("inside")
    assert h.closed == 1


def test_device_side_owns_what_it_builds(monkeypatch):
    made = []

    class _Sketches(_Handle):
        def __init__(self, seqs, *args, ctx=None):
            super().__init__()
            made.append((self, args, ctx))

    class _Context:
        def build_matrix(self, seqs, *args):
            made.append((_Handle(), args, self))
            return made[-1][0]

    monkeypatch.setattr(distance._sides, "Sketches", _Sketches)  # (where device_side looks it up)
    ctx = _Context()
    for mode, args in (("mash", (3, 10, 4, False)), ("euclidean", (3, 4)), ("jsd", (3, 4))):
        with distance.device_side(SEQS, mode, *args, ctx=ctx) as dev:
            h, got_args, got_ctx = made[-1]
            assert dev.handle is h and dev.mode == mode and got_args == args and got_ctx is ctx and h.closed == 0
        assert h.closed == 1
    assert len(made) == 3


def test_a_failure_building_the_second_side_closes_the_first(monkeypatch):
    made = []

    class _Sketches(_Handle):  # fails on its second construction
        def __init__(self, seqs, *args, ctx=None):
            if made:
                raise RuntimeError("the second side")
            super().__init__()
            made.append(self)

    monkeypatch.setattr(distance._sides, "Sketches", _Sketches)  # (where device_side looks it up)
    for fn, extra in ((distance.mash_cross_distances, ()), (distance.mash_nearest, (1,))):
        made.clear()
        with pytest.raises(RuntimeError, match="the second side") as info:
            fn(SEQS, SEQS, *extra, 3, 10, ctx=_NoContext())
        assert len(made) == 1 and made[0].closed == 1, fn.__name__  # closed when the exception arrives
        assert info.type is RuntimeError

    class _Context:  # the count-matrix modes: the same for a context whose second build fails
        def __init__(self):
            self.built = []

        def build_matrix(self, seqs, *args):
            if self.built:
                raise RuntimeError("the second side")
            self.built.append(_Handle())
            return self.built[0]

    for fn, extra in ((distance.jsd_cross_distances, ()), (distance.euclidean_nearest, (1,))):
        ctx = _Context()
        with pytest.raises(RuntimeError, match="the second side"):
            fn(SEQS, SEQS, *extra, 3, ctx=ctx)
        assert len(ctx.built) == 1 and ctx.built[0].closed == 1, fn.__name__


def test_an_unknown_mode_is_check_mode_args_error():
    with pytest.raises(ValueError) as want:
        distance.check_mode_args("manhattan", None, False)
    with pytest.raises(ValueError) as got:
        distance.DeviceSide(_Handle(), "manhattan")
    assert str(got.value) == str(want.value) == "Unexpected distance 'manhattan'."
    with pytest.raises(ValueError) as got:
        distance.device_side(SEQS, "manhattan", 3, 4, ctx=_NoContext())  # (before anything is built)
    assert str(got.value) == str(want.value)


def test_sides_of_two_modes_do_not_meet():
    a, b = distance.DeviceSide(_Handle(), "jsd"), distance.DeviceSide(_Handle(), "euclidean")
    with pytest.raises(ValueError, match="mode"):
        a.cross_distances(b)
    with pytest.raises(ValueError, match="mode"):
        a.nearest(b, 1)
