"""Every operation when a request for memory is refused in the middle of a call (DVS_TEST_KNOBS=refuse_block_<i>:
csrc/api.cpp counts a context's requests to dvs_dev_alloc, dvs_pinned_get and dvs_pinned_grow and refuses number i, once,
with the library's ordinary DVS_ERR_NOMEM).  A case of tests/test_blocks_host.py runs on a fresh context without the
knob, is held to its CPU reference there, and the context's gates say how many requests R it made and what it leaves
outstanding once its handles are closed (L0 device blocks: the context's own tables; P0 pinned pages).  Then, for EVERY
i = 1 .. R, on a fresh context with poison_blocks and refuse_block_<i>:

  * the case raises MemoryError with the knob's wording, which dvs_last_error repeats -- or it returns the clean run's
    outputs bit for bit (an optional request, whose fallback was taken); anything else fails;
  * nothing more than L0 blocks and P0 pages is outstanding afterwards (less is possible: a table of the context's
    that was the refused request is not there yet);
  * the same context -- the knob's one shot spent -- runs the case again: the clean bits, and exactly L0 and P0.  Its
    blocks are the failed run's, poisoned again: a kernel of the failed call still writing into a block that went back,
    or state left half-updated, is a differing bit here.

With i = R + 1 nothing is refused, the outputs are the clean ones and R requests are counted: R is the count, and the
walk left none out.  No index is sampled and none is left out.  Nothing here is a tolerance: the one inexact comparison
is the case's own check against its CPU reference.  R is printed (pytest -s; DESIGN.md 3.1 has the table) and not
asserted: it may follow the device's CU count."""
import gc

import pytest

from diverseseq_amd import engine
from test_blocks_host import CASES, ERROR_CASES, POISON, REFUSE, assert_same_outputs

pytestmark = pytest.mark.gpu


def _counts(ctx) -> dict:
    """the gates' figures once everything the case dropped has been collected"""
    gc.collect()
    return ctx.block_stats()


def _last_error(ctx) -> str:
    return (ctx._L.dvs_last_error(ctx._h) or b"").decode(errors="replace")


def _refused_run(case, ctx, i: int):
    """the case under refuse_block_<i>: its outputs, or None after the MemoryError that names the knob"""
    try:
        return case.run(ctx)
    except MemoryError as err:
        text = str(err)
    assert f"{REFUSE}{i}" in text and "refused by the test knob" in text, text
    return None


@pytest.mark.parametrize("name", list(CASES))
def test_every_request_refused_in_turn(monkeypatch, name):
    case = CASES[name]
    for var, value in case.env.items():
        monkeypatch.setenv(var, value)
    ctx = engine.Context(0)
    try:
        clean = case.run(ctx)
        base = _counts(ctx)
    finally:
        ctx.close()
    case.check(clean)
    R, L0, P0 = base["requests"], base["live_blocks"], base["pinned_out"]
    print(f"\nrefused blocks: {name}: R = {R}, L0 = {L0}, P0 = {P0}")
    assert R >= 1
    fallbacks = []
    for i in range(1, R + 2):
        monkeypatch.setenv("DVS_TEST_KNOBS", f"{POISON},{REFUSE}{i}")
        ctx = engine.Context(0)  # (reads the knob, counts from zero)
        try:
            what = f"{name}, request {i} of {R}"
            got = _refused_run(case, ctx, i)
            after = _counts(ctx)
            if got is None:
                assert i <= R, f"{what}: refused, but the clean run made only {R} requests"
                assert f"{REFUSE}{i}" in _last_error(ctx), (what, _last_error(ctx))
            else:
                assert_same_outputs(got, clean, f"{what}: not raised, so the fallback's bits")
                if i <= R:
                    fallbacks.append(i)
            assert after["live_blocks"] <= L0 and after["pinned_out"] <= P0, (what, "left outstanding", after, base)
            if i == R + 1:
                assert after["requests"] == R, (what, after)
                continue
            again = case.run(ctx)
            assert_same_outputs(again, clean, f"{what}: the same context again")
            after = _counts(ctx)
            assert (after["live_blocks"], after["pinned_out"]) == (L0, P0), (what, "after the follower", after, base)
        finally:
            ctx.close()
    print(f"refused blocks: {name}: optional requests (the fallback's bits) at {fallbacks}")


@pytest.mark.parametrize("name", list(ERROR_CASES))
def test_the_librarys_own_refusals_leave_nothing_outstanding(name):
    """an error case raises what it raises, and leaves what a context that ran only its set-up leaves"""
    err = ERROR_CASES[name]
    ctx = engine.Context(0)
    try:
        err.setup(ctx)
        want = _counts(ctx)
    finally:
        ctx.close()
    ctx = engine.Context(0)
    try:
        with pytest.raises(err.raises):
            err.run(ctx)
        got = _counts(ctx)
        assert (got["live_blocks"], got["live_bytes"], got["pinned_out"]) == \
               (want["live_blocks"], want["live_bytes"], want["pinned_out"]), (name, got, want)
    finally:
        ctx.close()
