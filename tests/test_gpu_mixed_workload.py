"""One context serving an interleaved workload: every case of tests/test_blocks_host.py in the schedules pinned
there, on ONE engine.Context that is never trimmed, each output bit-equal to the same case on a context of its own.
The test knobs are off: this is about which block the cache hands to whom, and about what ran on the context just
before.  Every square matrix has 257 rows, so its 257 x 257 x 8 = 528 392-byte block (532 480 in the cache's 4 KiB
classes) passes between the mash, jsd, euclidean, linkage, neighbour-joining, cophenet and max-min calls; the 257-entry
lists (1 028 and 2 056 bytes), the flag and status words, the sync blocks and every other block of 4 KiB or less fall
into the one 4 096-byte class and collide by construction."""
import numpy as np
import pytest

from diverseseq_amd import engine
from test_blocks_host import (CASES, ERROR_CASES, assert_same_outputs, largest_block, schedule_kept_handles, schedule_orders,
                              schedule_with_errors)

pytestmark = pytest.mark.gpu


class _Env:
    """the case's switches for the length of its run (the conftest's monkeypatch re-reads them in the live contexts)"""

    def __init__(self, monkeypatch, case):
        self.mp, self.case = monkeypatch, case

    def __enter__(self):
        for var, value in self.case.env.items():
            self.mp.setenv(var, value)

    def __exit__(self, *exc):
        for var in self.case.env:
            self.mp.delenv(var)


@pytest.fixture(scope="module")
def baseline():
    """every case's outputs from a context of its own, closed afterwards; computed once, never changed"""
    import os

    out = {}
    for name, case in CASES.items():
        saved = {var: os.environ.get(var) for var in case.env}
        os.environ.update(case.env)
        try:
            ctx = engine.Context(0)  # (a new context reads the switches as they are now)
            try:
                out[name] = case.run(ctx)
            finally:
                ctx.close()
        finally:
            for var, old in saved.items():
                if old is None:
                    os.environ.pop(var, None)
                else:
                    os.environ[var] = old
    engine.refresh_all_knobs()
    return out


def _run(monkeypatch, ctx, name, baseline, what, keep=None):
    case = CASES[name]
    with _Env(monkeypatch, case):
        got = case.run(ctx, keep)
    assert_same_outputs(got, baseline[name], f"{what}: {name}")


def test_baseline_is_the_reference(baseline):
    """the clean outputs the schedules are compared with are the CPU references' (each family's own comparison)"""
    for name, case in CASES.items():
        case.check(baseline[name])


@pytest.mark.parametrize("order", ["ascending", "reversed", "shuffled"])
def test_three_orders_on_one_context(monkeypatch, baseline, order):
    """(a)"""
    ctx = engine.Context(0)
    try:
        for name in schedule_orders()[order]:
            _run(monkeypatch, ctx, name, baseline, order)
    finally:
        ctx.close()


def test_shuffle_with_handles_kept_alive(monkeypatch, baseline):
    """(b) matrices, sketches, selections, packed planes and sequence batches stay open and are closed later in
    another seeded order -- the last of them after the context's owner has dropped it -- so that blocks return to the
    cache at other moments than in (a)"""
    rng = np.random.default_rng(20_261)
    ctx = engine.Context(0)
    handles = []
    try:
        for step in schedule_kept_handles():
            if step[0] == "run":
                _run(monkeypatch, ctx, step[1], baseline, "handles kept", keep=handles)
            elif step[0] == "close":
                picked = rng.permutation(len(handles))[: int(round(step[1] * len(handles)))]
                for i in picked:
                    handles[i].close()
                handles = [h for i, h in enumerate(handles) if i not in set(picked.tolist())]
            else:
                ctx.close()  # (the owner is gone; the open handles keep the context's caches alive)
        assert handles == []
    finally:
        for h in handles:
            h.close()
        ctx.close()


def test_shuffle_with_error_cases_interleaved(monkeypatch, baseline):
    """(c) every failing call directly in front of a case that asks for blocks of the same sizes"""
    ctx = engine.Context(0)
    try:
        for kind, name in schedule_with_errors():
            if kind == "error":
                with pytest.raises(ERROR_CASES[name].raises):
                    ERROR_CASES[name].run(ctx)
            else:
                _run(monkeypatch, ctx, name, baseline, "errors interleaved")
    finally:
        ctx.close()


def test_shuffle_on_a_callers_stream(monkeypatch, baseline):
    """(d) the context's stream is the caller's (tests/test_gpu_parity.py's row-sharded workers make theirs so)"""
    import torch

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = engine.Context(0, stream=stream.cuda_stream)
        try:
            for name in schedule_orders()["shuffled"]:
                _run(monkeypatch, ctx, name, baseline, "caller's stream")
        finally:
            ctx.close()
    torch.cuda.synchronize()


def test_the_cache_keeps_its_blocks_and_does_not_grow(monkeypatch, baseline):
    """Two conditions on free device memory around a second pass on a warmed context.  The cache does not grow: the
    second pass lowers free memory by no more than the largest single block of the table (one block of margin: other
    processes share the card).  And the blocks are kept, not freed: releasing the cache afterwards (dvs_ctx_trim) gives
    back at least one 257 x 257 matrix block (the table's blocks add up to more than 40 MB -- the 25 MB count rows of
    k = 8, two 8 MB record lists of the ingest -- so a neighbour taking one largest block in between leaves this true).  Conditions, not measurements; that a kept block is also the one handed
    out again is what every bit-equal output above rests on."""
    import torch

    ctx = engine.Context(0)
    try:
        for name in schedule_orders()["ascending"]:
            _run(monkeypatch, ctx, name, baseline, "warm-up")
        ctx.sync()
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        for name in schedule_orders()["ascending"]:
            _run(monkeypatch, ctx, name, baseline, "second pass")
        ctx.sync()
        torch.cuda.synchronize()
        after = torch.cuda.mem_get_info()[0]
        ctx.check(ctx._L.dvs_ctx_trim(ctx._h))
        trimmed = torch.cuda.mem_get_info()[0]
        print(f"free device memory: {before} before the second pass, {after} after it, {trimmed} with the cache released; "
              f"largest block {largest_block()}")
        assert before - after <= largest_block()
        assert trimmed - after >= 257 * 257 * 8
    finally:
        ctx.close()
