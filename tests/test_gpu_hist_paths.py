"""Every count-matrix build path against the oracle (reference src/record.rs:31-141): the cases of
tests/hist_path_cases.py -- one per launch use, input form and histogram placement of csrc/kmer_hist.hip, which
tests/test_hist_paths_host.py shows to reach each of the twelve kmer_hist_kernel instantiations -- counts bit for bit,
totals exact, entropies to the 1e-11 of tests/test_gpu_parity.py."""
import numpy as np
import pytest

from hist_path_cases import CASES, case_seqs, expected
from test_gpu_parity import TIGHT
from test_hist_paths_host import launches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from diverseseq_amd import engine

    return engine.default_context()


def _build(ctx, case):
    """-> (the matrix, what has to outlive it)"""
    from diverseseq_amd import engine

    data, offsets = engine.concat(list(case_seqs(case)))
    if case.form == "packed":
        p = ctx.pack_host(data)
        return ctx.build_matrix_packed(p, offsets, case.k), p
    if case.form == "device":  # (the build is not waited for; 16 bytes of slack behind the last base)
        import torch

        t = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to("cuda:0")
        torch.cuda.synchronize()
        return ctx.build_matrix_device(t.data_ptr(), offsets, case.k, case.states), t
    return ctx.build_matrix_concat(data, offsets, case.k, case.states), None


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_build_path_vs_oracle(ctx, monkeypatch, case):
    if case.counts_u32:
        monkeypatch.setenv("DVS_COUNTS_U32", "1")
    counts, totals, ent = expected(case)
    m, keep = _build(ctx, case)
    try:
        assert m.nbins == case.nbins and m.count_bytes == (2 if launches(case)[2] == 2 else 4)
        got = m.counts()
        assert got.shape == counts.shape and (got == counts).all(), f"{case.name}: k-mer counts differ"
        assert (m.totals() == totals).all()
        H = m.entropy()
        worst = float(np.max(np.abs(H - ent) / np.maximum(1.0, np.abs(ent))))
        print(f"{case.name}: largest entropy difference {worst:.3g} (relative to max(1, H))")
        assert worst <= TIGHT
    finally:
        m.close()
        if case.form == "packed":
            keep.close()
