"""The table of tests/hist_path_cases.py, pinned on the CPU before it is used on the device: the rule by which
csrc/kmer_hist.hip maps a build's shape to an instantiation of kmer_hist_kernel<NS4, LDS_HIST, PK16, OUT16, PACKED>,
restated here, says that the cases reach each of the twelve instantiations the file holds -- as a whole-row launch and
as a tile launch wherever both exist -- and the oracle computes every case."""
import numpy as np
import pytest

import oracle
from hist_path_cases import CASES, LDS_HIST_BYTES, N_SHORT, TILE_LEN, U16_MAX_BINS, UNIFORM_LEN, case_seqs, expected

#                <NS4, LDS_HIST, PK16, OUT16, PACKED>
ROWS_16BIT = {(1, 1, 1, 1, 1), (1, 1, 1, 1, 0), (0, 1, 1, 1, 0)}
ROWS_PACKED_COUNTERS = {(1, 1, 1, 0, 1), (1, 1, 1, 0, 0), (0, 1, 1, 0, 0)}
PLAIN = {(1, 1, 0, 0, 1), (1, 0, 0, 0, 1), (1, 1, 0, 0, 0), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 0, 0, 0)}
# (four states: the bin count is a multiple of four, so a whole row with an LDS histogram has packed counters)
PLAIN_WHOLE = PLAIN - {(1, 1, 0, 0, 1), (1, 1, 0, 0, 0)}


def windows(seq, k):
    return max(len(seq) - k + 1, 0)


def launches(case):
    """the selection rule of dvs_matrix_fill_counts -> (the whole-row instantiation, the tile one or None, matrix kind)"""
    B = case.nbins
    packed = case.form == "packed"
    ns4 = case.states == 4
    n_long = sum(windows(s, case.k) > TILE_LEN for s in case_seqs(case))
    lds_hist = 4 * B <= LDS_HIST_BYTES
    pk16 = lds_hist and B % 4 == 0
    kind2 = n_long == 0 and B <= U16_MAX_BINS and B % 4 == 0 and not case.counts_u32
    if kind2:
        whole = (int(ns4), 1, 1, 1, int(packed))
    elif pk16:
        whole = (int(ns4), 1, 1, 0, int(packed))
    else:
        whole = (int(ns4), int(lds_hist), 0, 0, int(packed))
    tiles = (int(ns4), int(lds_hist), 0, 0, int(packed)) if n_long else None
    return whole, tiles, 2 if kind2 else 0


def test_twelve_instantiations():
    assert len(ROWS_16BIT | ROWS_PACKED_COUNTERS | PLAIN) == 12
    assert not (ROWS_16BIT & ROWS_PACKED_COUNTERS) and not (PLAIN & (ROWS_16BIT | ROWS_PACKED_COUNTERS))


def test_the_table_reaches_every_instantiation():
    whole = {launches(c)[0] for c in CASES}
    tiles = {launches(c)[1] for c in CASES} - {None}
    assert whole == ROWS_16BIT | ROWS_PACKED_COUNTERS | PLAIN_WHOLE, sorted(whole)
    assert tiles == PLAIN, sorted(tiles)
    assert len({c.name for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_takes_the_path_it_is_listed_for(case):
    whole, tiles, kind = launches(case)
    use = case.name.split("_")[0]
    assert (tiles is not None) == case.long_row == (use == "tiles")
    assert whole in {"u16": ROWS_16BIT, "pk32": ROWS_PACKED_COUNTERS, "odd": {(0, 1, 0, 0, 0)},
                     "wide": {(1, 0, 0, 0, 0), (1, 0, 0, 0, 1), (0, 0, 0, 0, 0)},
                     "tiles": ROWS_PACKED_COUNTERS | PLAIN_WHOLE}[use]
    assert (kind == 2) == (use == "u16")
    assert whole[4] == (case.form == "packed") and whole[0] == (case.states == 4)
    if case.name.startswith("tiles_wide") or use == "wide":
        assert 4 * case.nbins > LDS_HIST_BYTES
    if case.name == "pk32_s4_k7_bytes":
        assert 4 * case.nbins == LDS_HIST_BYTES and not case.counts_u32  # (past 4 096 bins the rows are 32-bit anyway)
    if case.form == "packed":
        assert case.states == 4
    seqs = case_seqs(case)
    lens = [len(s) for s in seqs]
    if case.form == "uniform":  # one length, a single tile each: the build keeps no offsets on the device
        assert lens == [UNIFORM_LEN] * N_SHORT and UNIFORM_LEN < TILE_LEN + case.k
    else:
        assert len(set(lens)) > 2
    if case.long_row:
        assert len(seqs) == N_SHORT + 1 and windows(seqs[2], case.k) == TILE_LEN + case.k  # two tiles, short rows around
        lens.pop(2)
    assert all(20 <= n <= 700 for n in lens) and len(lens) == N_SHORT


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_oracle_computes_the_case(case):
    seqs = case_seqs(case)
    counts, totals, ent = expected(case)
    assert counts.shape == (len(seqs), case.nbins) and counts.dtype == np.uint64
    for s, t in zip(seqs, totals):  # windows without an invalid symbol, counted independently
        bad = np.flatnonzero(s >= case.states)
        ok = np.ones(windows(s, case.k), dtype=bool)
        for b in bad:
            ok[max(b - case.k + 1, 0): b + 1] = False
        assert t == ok.sum() and t > 0
    assert any((s >= case.states).any() for s in seqs)
    assert np.isfinite(ent).all() and (ent >= 0).all() and (ent <= np.log2(case.nbins) + 1e-12).all()
    assert abs(ent[0] - oracle.entropy(counts[0] / totals[0])) <= 1e-12
    if case.long_row:  # (three invalid symbols cost at most 3 k windows)
        assert totals[2] >= TILE_LEN + case.k - 3 * case.k
