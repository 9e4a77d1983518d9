"""Every operation family on blocks full of 0xFF bytes (DVS_TEST_KNOBS=poison_blocks: csrc/api.cpp dvs_dev_alloc and
dvs_pinned_get fill what they hand out).  A case of tests/test_blocks_host.py runs on a fresh context without the knob
and is held to its CPU reference there; then, with the knob, on a fresh context and again on that same context -- the
second run gets the first one's blocks back from the cache, poisoned again -- and every output must be the first run's
bit for bit, NaN for NaN.  A read before the first write, which zeros or the last call's values would hide, shows up
as a different bit.  No tolerance appears here: the only inexact comparison is the one against the CPU reference, by
that family's own bound.  The error cases raise what they raise without the knob."""
import pytest

from diverseseq_amd import engine
from test_blocks_host import CASES, ERROR_CASES, POISON, assert_same_outputs, cases_of

pytestmark = pytest.mark.gpu


def _fresh(case, runs: int = 1) -> list:
    ctx = engine.Context(0)
    try:
        return [case.run(ctx) for _ in range(runs)]
    finally:
        ctx.close()


def _case_under_poison(monkeypatch, name):
    case = CASES[name]
    for var, value in case.env.items():
        monkeypatch.setenv(var, value)
    clean, = _fresh(case)
    case.check(clean)
    monkeypatch.setenv("DVS_TEST_KNOBS", POISON)
    first, again = _fresh(case, 2)
    assert_same_outputs(first, clean, f"{name}: poisoned, fresh context")
    assert_same_outputs(again, clean, f"{name}: poisoned, the first run's blocks again")


@pytest.mark.parametrize("name", cases_of("distances"))
def test_distances(monkeypatch, name):
    _case_under_poison(monkeypatch, name)


@pytest.mark.parametrize("name", cases_of("trees"))
def test_trees(monkeypatch, name):
    _case_under_poison(monkeypatch, name)


@pytest.mark.parametrize("name", cases_of("cophenet_clusters"))
def test_cophenet_clusters(monkeypatch, name):
    _case_under_poison(monkeypatch, name)


@pytest.mark.parametrize("name", cases_of("maxmin"))
def test_maxmin(monkeypatch, name):
    _case_under_poison(monkeypatch, name)


@pytest.mark.parametrize("name", cases_of("sketches"))
def test_sketches(monkeypatch, name):
    _case_under_poison(monkeypatch, name)


@pytest.mark.parametrize("name", cases_of("histograms"))
def test_histograms(monkeypatch, name):
    _case_under_poison(monkeypatch, name)


@pytest.mark.parametrize("name", cases_of("ingest"))
def test_ingest(monkeypatch, name):
    _case_under_poison(monkeypatch, name)


@pytest.mark.parametrize("name", cases_of("selections"))
def test_selections(monkeypatch, name):
    _case_under_poison(monkeypatch, name)


@pytest.mark.parametrize("name", cases_of("neighbours"))
def test_neighbours(monkeypatch, name):
    _case_under_poison(monkeypatch, name)


@pytest.mark.parametrize("name", cases_of("ordination"))
def test_ordination(monkeypatch, name):
    _case_under_poison(monkeypatch, name)


@pytest.mark.parametrize("name", cases_of("medoids"))
def test_medoids(monkeypatch, name):
    _case_under_poison(monkeypatch, name)


@pytest.mark.parametrize("name", cases_of("spanning"))
def test_spanning(monkeypatch, name):
    _case_under_poison(monkeypatch, name)


@pytest.mark.parametrize("name", cases_of("groups"))
def test_groups(monkeypatch, name):
    _case_under_poison(monkeypatch, name)


@pytest.mark.parametrize("name", list(ERROR_CASES))
def test_error_cases_raise_the_same(monkeypatch, name):
    """... and the case that asks for blocks of the same sizes right behind the failing call gives its clean bits"""
    err = ERROR_CASES[name]
    follower = CASES[err.follower]
    for var, value in follower.env.items():
        monkeypatch.setenv(var, value)
    clean, = _fresh(follower)
    raised = []
    for knob in (None, POISON):
        if knob:
            monkeypatch.setenv("DVS_TEST_KNOBS", knob)
        ctx = engine.Context(0)
        try:
            with pytest.raises(err.raises) as info:
                err.run(ctx)
            raised.append(type(info.value))
            assert_same_outputs(follower.run(ctx), clean, f"{err.follower} behind {name}, knob {knob}")
        finally:
            ctx.close()
    assert raised[0] is raised[1]
