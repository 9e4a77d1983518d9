"""Scan decisions at the band edges, on every tier and engine path (cases and crafting: tests/test_bands_host.py).

Every stream holds rows whose exact score is the threshold plus a crafted margin: multiples of FAST_BAND and of
coarse_band(B), and a NEAR-ZERO pair 25 to 1000 times closer to the threshold than FAST_BAND yet well outside the
arbiter's sel_band.  A tier that decided such a row by itself, or whose state were slightly off on one code path, would
accept or reject it wrongly, so each test asks for

  1. the engine the case is about (summary().engine),
  2. the oracle's members, order, rows and floats (_assert_selection),
  3. the oracle's accept count: every single decision, also for a crafted row that a later row evicts,
  4. no arbitration (the crafted margins are outside sel_band) -- except in the arbiter cases, which sit inside it,
  5. against the same prefix without the crafted rows: rows_rechecked grows by at least the rows within
     0.6 x FAST_BAND, and rows_coarse_passed by those within 0.6 x coarse_band(B) where the path taken has a COARSE tier.

Each test prints its achieved margins in units of their band and the two counters' growth (pytest -s)."""
import numpy as np
import pytest

from test_bands_host import (ARBITER_K6, ARBITER_MULTS, B4096_COUNT_CASES, FAST_BAND, FREQS_K6, HEAD_SPLIT_AT, K5, MAX_K4,
                             OTHER_SEQ_CASES, OWN14, SMALL13, STRADDLE, coarse_band, crafted, head_stream, in_units,
                             oracle_whole, sure_within)
from test_gpu_configs import _device_build
from test_gpu_parity import RTOL, _assert_selection

pytestmark = pytest.mark.gpu

NO_PERSIST = {"DVS_NO_PERSIST": "1"}
WAVE_ROWS = {"DVS_PERSIST_WG_ROUNDS": "0"}        # a row per wave throughout (p_scan_rows)
WG_ROWS = {"DVS_PERSIST_WG_ROUNDS": "100000"}     # a row per workgroup throughout (p_scan_rows_wg, _wg_stream)
NO_COARSE = {"DVS_PERSIST_NO_COARSE": "1"}        # api.cpp: persist_no_coarse
ENVS_4096 = ({}, WAVE_ROWS, WG_ROWS, NO_PERSIST, NO_COARSE)
ENVS_OTHER = ({}, NO_PERSIST)
# 1024 and 256 bins meet the COARSE tier in the row-per-wave scan only (p_scan_rows_wg wants B a multiple of 2048)
WAVE_ONLY_COARSE = (K5,) + MAX_K4


def _env_id(env):
    return "-".join(f"{k[4:].lower()}{v}" for k, v in env.items()) or "default"


def _params(cases, envs, extra=()):
    out = [pytest.param(c, e, id=f"{c.name}-{_env_id(e)}") for c in cases for e in envs]
    return out + [pytest.param(c, e, id=f"{c.name}-{_env_id(e)}") for c, e in extra]


@pytest.fixture(scope="module")
def ctx():
    from diverseseq_amd import engine

    return engine.default_context()


def _build(ctx, case, c, nrows=None):
    if c.rows is not None:
        return ctx.matrix_from_freqs(c.rows[:nrows])
    return ctx.build_matrix(c.seqs[:nrows], case.k, case.states)


def _select(m, case):
    if case.mode[0] == "nmost":
        return m.nmost(case.n)
    return m.max_divergent(case.n, case.mode[1], case.mode[2])


def _run(ctx, case, env, monkeypatch, arbiter=False):
    for k_, v_ in tuple(case.env) + tuple(env.items()):
        monkeypatch.setenv(k_, v_)
    c = crafted(case)
    exp, _ = oracle_whole(case)
    m = _build(ctx, case, c)
    assert m.count_bytes == (0 if c.rows is not None else case.count_bytes)
    sel = _select(m, case)
    s = sel.summary()
    m0 = _build(ctx, case, c, case.nprefix)  # the same prefix without the crafted rows: what the bands cost on ordinary input
    sel0 = _select(m0, case)
    s0 = sel0.summary()
    d_fast, d_coarse = s.rows_rechecked - s0.rows_rechecked, s.rows_coarse_passed - s0.rows_coarse_passed
    print(f"\n{case.name} [{_env_id(env)}] engine {s.engine} accepts {s.n_accepts} (oracle {c.accepts}) arbitrated {s.n_arbitrated}"
          f" rows_rechecked +{d_fast} rows_coarse_passed +{d_coarse}\n  margins / band: {' '.join(in_units(c))}")
    persistent = case.engine == 1 and "DVS_NO_PERSIST" not in env
    assert s.engine == (1 if persistent else 0)
    _assert_selection(sel, exp)
    assert s.n_accepts == c.accepts
    if not arbiter:
        assert s.n_arbitrated == 0
        assert sure_within(c, FAST_BAND) >= (4 if case.two else 6)
        # The persistent engine's `max` works the rows behind a tentative push out in BATCHES while the set is below
        # max_size (persist.hip, "BATCH: the rows behind the event"): a batch scores its rows in f64 outright, no tier
        # sees them and neither counter moves (max_k6_stdev: 5 of its 7 rows inside FAST_BAND were listed by the FAST
        # tier, 2 went through batches).  There the counters are asked only for the rows that meet a full set; the
        # decisions themselves are held by the ids and the accept count above.
        full = case.mode[1] if persistent and case.mode[0] == "max" else 0
        sure_fast = sure_within(c, FAST_BAND, full)
        assert d_fast >= sure_fast, (s.rows_rechecked, s0.rows_rechecked, sure_fast)
        coarse_here = persistent and case.coarse and "DVS_PERSIST_NO_COARSE" not in env and \
            (case.nbins == 4096 or env == WAVE_ROWS)
        if coarse_here:
            assert sure_within(c, coarse_band(case.nbins)) >= sure_within(c, FAST_BAND) + 4
            sure_coarse = sure_within(c, coarse_band(case.nbins), full)
            assert d_coarse >= sure_coarse, (s.rows_coarse_passed, s0.rows_coarse_passed, sure_coarse)
    for x in (sel, sel0, m, m0):
        x.close()
    return s


@pytest.mark.parametrize("case,env", _params(B4096_COUNT_CASES, ENVS_4096))
def test_band_edges_on_4096_bin_count_rows(ctx, case, env, monkeypatch):
    """SMALL at its last set size, OWN at its first and beyond one wave's argmin, 32-bit counts (coarse4(uint4)) and
    rows of unequal totals: both row mappings of the persistent scan, the scan without its COARSE tier, and the
    multi-launch engine (reference src/records.rs:86-92, `jsd > total_jsd + EPSILON`)"""
    _run(ctx, case, env, monkeypatch)


@pytest.mark.parametrize("case,env", _params(OTHER_SEQ_CASES, ENVS_OTHER, [(c, WAVE_ROWS) for c in WAVE_ONLY_COARSE]))
def test_band_edges_on_the_other_shapes_and_modes(ctx, case, env, monkeypatch):
    """sparse rows (zero bins of sl, the eps clamps), coarse_band(B) below 4096 bins, 400 / 125 / 8000 bins (scalar loops
    and tails, the not-cached instantiation), `max` on the persistent engine (stdev and cov) and on the multi-launch
    max_batch kernels"""
    _run(ctx, case, env, monkeypatch)


@pytest.mark.parametrize("env", ENVS_OTHER, ids=_env_id)
def test_band_edges_on_frequency_rows(ctx, env, monkeypatch):
    """T = double: the scan has the FAST tier only; margins bisected to the target"""
    _run(ctx, FREQS_K6, env, monkeypatch)


@pytest.mark.parametrize("env", ENVS_OTHER, ids=_env_id)
@pytest.mark.parametrize("case", ARBITER_K6, ids=lambda c: c.name)
def test_the_edge_of_the_arbiters_band(ctx, case, env, monkeypatch):
    """frequency rows at +-0.25 x sel_band_min(4096) = +-9.1e-13 from the threshold: inside sel_band whatever the
    entropy, so the launch must stop and the host arbiter replay the reference (n_arbitrated >= 1); at +-3 x
    sel_band_min the device may decide or arbitrate -- either way the oracle's ids and accept count"""
    s = _run(ctx, case, env, monkeypatch, arbiter=True)
    if case is ARBITER_K6[ARBITER_MULTS.index(0.25)]:
        assert s.n_arbitrated >= 1


@pytest.mark.parametrize("case", (OWN14, K5), ids=lambda c: c.name)
def test_band_edges_in_the_stepwise_mode(ctx, case):
    """the exact (row-sharded) mode's fast step and its all-f32 tier at world 1, driven as
    test_gpu_parity.test_exact_mode_fast_step_shapes drives it: the oracle's ids and accept count"""
    import torch

    from diverseseq_amd import parallel

    c = crafted(case)
    exp, acc = oracle_whole(case)
    dev = torch.device("cuda", 0)
    m = ctx.build_matrix(c.seqs, case.k, case.states)
    _, order = parallel.shard_order(len(c.seqs), case.n, 0, 1, block=32)
    sel = parallel.nmost_exact(ctx, m, order, case.n, dev, 1)
    s, mem = sel.summary(), sel.members(with_freqs=False)
    elab, edelta, _, _ = exp.members()
    print(f"\n{case.name} [stepwise] accepts {s.n_accepts} (oracle {acc}) arbitrated {s.n_arbitrated} rows_rechecked {s.rows_rechecked}"
          f"\n  margins / band: {' '.join(in_units(c))}")
    assert mem.positions.tolist() == elab.tolist()
    assert s.n_accepts == acc == c.accepts
    np.testing.assert_allclose(mem.delta_jsd, edelta, rtol=RTOL, atol=1e-13)
    np.testing.assert_allclose(s.total_jsd, exp.total_jsd, rtol=RTOL)
    sel.close()
    m.close()


@pytest.mark.parametrize("env", ({}, {"DVS_NO_HEAD_PHASE": "1"}, {"DVS_PERSIST_NO_SEEDED": "1"}), ids=_env_id)
@pytest.mark.parametrize("case", (SMALL13, STRADDLE), ids=lambda c: c.name)
def test_band_edges_in_the_head_phase_and_across_the_hand_over(case, env, monkeypatch):
    """a device-resident build of 17 600 rows is split at row 1024 and the persistent engine walks the head rows on the
    head CUs (test_gpu_configs.test_head_phase_of_a_split_build_vs_oracle): the small13 stream has every crafted row
    inside the head phase, the straddling one at positions 1020 .. 1030, on both sides of the hand-over to the
    full-grid launch; the same with the head phase and the seeded start switched off"""
    from diverseseq_amd import engine

    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    seqs, exp, acc = head_stream(case)
    c = crafted(case)
    assert (max(c.positions) < HEAD_SPLIT_AT) == (case is SMALL13)
    cx = engine.Context(0)  # (the CU split is a property of the context: a fresh one sees the knobs)
    cx.set_timing(True)
    try:
        m, keep = _device_build(cx, seqs, case.k)
        assert m.count_bytes == 2
        sel = m.nmost(case.n)
        s = sel.summary()
        print(f"\n{case.name} [head, {_env_id(env)}] accepts {s.n_accepts} (oracle {acc}) arbitrated {s.n_arbitrated} launches {s.scan_launches}"
              f" rows_rechecked {s.rows_rechecked} rows_coarse_passed {s.rows_coarse_passed}\n  margins / band: {' '.join(in_units(c))}")
        _assert_selection(sel, exp)
        assert s.engine == 1 and s.n_arbitrated == 0
        assert s.n_accepts == acc
        if not env:
            assert s.scan_launches == 2, "head phase + full-grid launch expected"
        assert s.rows_rechecked >= sure_within(c, FAST_BAND)
        sel.close()
        m.close()
    finally:
        cx.close()
    del keep
