"""The count-matrix build paths, one case each: (launch use x input form x histogram placement) at the smallest shape
that takes the path.  Shared by tests/test_hist_paths_host.py (the selection rule restated, the table checked against it
on the CPU) and tests/test_gpu_hist_paths.py (every case against the oracle on the device).

csrc/kmer_hist.hip launches kmer_hist_kernel<NS4, LDS_HIST, PK16, OUT16, PACKED> in three uses:
  * 16-bit rows (matrix kind 2): whole sequences, packed 16-bit LDS counters that leave as they are;
  * 32-bit whole rows from packed LDS counters;
  * everything else: the tiles of long rows, and whole rows whose bin count is no multiple of four or whose histogram
    does not fit 64 KiB of LDS (the row itself then takes global atomics).
A build launches the whole-row kernel over every sequence, and the tile kernel when some row is long (more than
TILE_LEN windows)."""
import functools
from typing import NamedTuple

import numpy as np

import oracle

TILE_LEN = 32_768      # windows of a whole-row workgroup (csrc/kmer_hist.hip)
LDS_HIST_BYTES = 65_536
U16_MAX_BINS = 4_096   # dvs_hist_rows_fit_u16
N_SHORT = 7            # the ragged handful
UNIFORM_LEN = 333      # one length for every sequence: no offsets on the device


class Case(NamedTuple):
    name: str
    states: int
    k: int
    form: str              # "bytes", "packed", "uniform" (bytes, one length), "device" (bytes in HBM, build not waited for)
    long_row: bool = False
    counts_u32: bool = False   # run under DVS_COUNTS_U32=1

    @property
    def nbins(self):
        return self.states ** self.k


def _forms(name, states, k, forms, **kw):
    return tuple(Case(f"{name}_{f}", states, k, f, **kw) for f in forms)


CASES = (
    # 16-bit rows: bytes (also of one length, also device-resident and unwaited) / packed / other alphabet
    _forms("u16_s4_k3", 4, 3, ("bytes", "uniform", "device", "packed"))
    + _forms("u16_s20_k2", 20, 2, ("bytes",))
    # 32-bit rows from packed LDS counters: the three above with 32-bit rows asked for, and 16 384 bins (exactly 64 KiB)
    + _forms("pk32_s4_k3", 4, 3, ("bytes", "uniform", "packed"), counts_u32=True)
    + _forms("pk32_s20_k2", 20, 2, ("bytes",), counts_u32=True)
    + _forms("pk32_s4_k7", 4, 7, ("bytes",))
    # whole rows, LDS histogram, a bin count that is no multiple of four
    + _forms("odd_s5_k2", 5, 2, ("bytes", "uniform"))
    # whole rows, global atomics
    + _forms("wide_s4_k8", 4, 8, ("bytes", "uniform", "packed"))
    + _forms("wide_s20_k4", 20, 4, ("bytes",))
    # tiles of a long row, LDS histogram
    + _forms("tiles_s4_k3", 4, 3, ("bytes", "packed"), long_row=True)
    + _forms("tiles_s20_k2", 20, 2, ("bytes",), long_row=True)
    # tiles of a long row, global atomics
    + _forms("tiles_wide_s4_k8", 4, 8, ("bytes", "packed"), long_row=True)
    + _forms("tiles_wide_s20_k4", 20, 4, ("bytes",), long_row=True)
)


def _seed(case):
    return 1000 * case.states + 10 * case.k + case.long_row


@functools.lru_cache(maxsize=None)
def case_seqs(case: Case):
    """a ragged handful of 20 to 700 symbols, some of them invalid (the value `states`); "uniform": one length; a long
    row -- 32 768 + k windows: two tiles, the second of k windows -- between the short ones"""
    rng = np.random.default_rng(_seed(case))
    lens = [UNIFORM_LEN] * N_SHORT if case.form == "uniform" else [20, 700] + rng.integers(20, 701, size=N_SHORT - 2).tolist()
    seqs = [rng.integers(0, case.states, size=n, dtype=np.uint8) for n in lens]
    for s in seqs[1::2]:
        s[rng.integers(0, s.size, size=3)] = case.states
    if case.long_row:
        long = rng.integers(0, case.states, size=TILE_LEN + case.k + case.k - 1, dtype=np.uint8)
        long[[100, TILE_LEN - 1, TILE_LEN + case.k // 2]] = case.states  # (one of them across the tile edge)
        seqs.insert(2, long)
    return tuple(seqs)


@functools.lru_cache(maxsize=None)
def expected(case: Case):
    """the oracle's (counts uint64 [n, B], totals uint64 [n], entropies f64 [n]; NaN where the total is 0)"""
    seqs = case_seqs(case)
    counts = np.stack([oracle.count_kmers(s, case.states, case.k) for s in seqs])
    totals = counts.sum(axis=1)
    ent = np.array([oracle.to_kfreqs(s, case.states, case.k)[1] if t else np.nan for s, t in zip(seqs, totals)])
    return counts, totals, ent
