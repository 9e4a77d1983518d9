"""One sequence source behind the builds (include/dvs_hip.h dvs_seqs): the same sequences handed over as host bytes,
as a device pointer, as packed planes and as an ingested FASTA file (byte form and packed in place) give ONE count
matrix -- the matrix-side counterpart of test_gpu_sketch.py::test_every_entry_point_gives_one_answer -- and the
source's own refusals, each with its message."""
import ctypes as C

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

LENGTHS = (0, 2, 15, 16, 17, 50, 40_000)  # around k, around a packed word of 16 bases, and one of two histogram tiles


@pytest.fixture(scope="module")
def ctx():
    from diverseseq_amd import engine

    return engine.default_context()


def _sequences():
    """symbols >= 4 at the seams: a word's last and first base, and both sides of the long one's tile seam (a tile is
    32 768 windows)"""
    rng = np.random.default_rng(41)
    seqs = [rng.integers(0, 4, size=n, dtype=np.uint8) for n in LENGTHS]
    seqs[2][7] = 4
    seqs[4][[15, 16]] = (5, 4)
    seqs[5][[0, 31, 32, 49]] = (4, 5, 4, 5)
    seqs[6][[3, 32_767, 32_768, 39_999]] = (4, 5, 4, 4)
    seqs[6][rng.integers(0, 40_000, size=40)] = 4
    return seqs


def _fasta(seqs) -> bytes:
    return "".join(f">s{i}\n" + "".join("TCAG-N"[c] for c in q) + "\n" for i, q in enumerate(seqs)).encode()


def _outputs(m):
    out = m.counts().astype(np.uint64), m.totals().copy(), m.entropy().view(np.uint64).copy()
    m.close()
    return out


def _five_forms(ctx, seqs, k):
    """-> {form: (counts, totals, the entropies' bits)}"""
    import torch

    from diverseseq_amd import engine

    data, offsets = engine.concat(seqs)
    dev = torch.zeros(data.size + 16, dtype=torch.uint8, device="cuda:0")
    dev[: data.size] = torch.from_numpy(data.copy()).to("cuda:0")
    torch.cuda.synchronize()
    got = {"host bytes": _outputs(ctx.build_matrix(seqs, k)),
           "device pointer": _outputs(ctx.build_matrix_device(dev.data_ptr(), offsets, k))}
    p = ctx.pack_host(data)
    got["packed planes"] = _outputs(ctx.build_matrix_packed(p, offsets, k))
    p.close()
    for pack in (False, True):
        b = ctx.encode_fasta(_fasta(seqs))
        assert (b.offsets == offsets).all()
        if pack:
            b.pack()
        got["ingested, packed in place" if pack else "ingested, byte form"] = _outputs(b.build_matrix(k))
        b.close()
    return got


@pytest.mark.parametrize("long_one", [True, False])
@pytest.mark.parametrize("k", [3, 7])
def test_every_source_form_gives_one_matrix(ctx, k, long_one):
    """k = 3 and k = 7 over the whole set (the sequence of two tiles makes every row 32-bit) and over the set without
    its long sequence, where k = 3 gives 16-bit rows: counts, totals and the bits of the entropies are equal across the
    five forms, and the counts are the oracle's"""
    seqs = _sequences() if long_one else _sequences()[:-1]
    if not long_one and k == 3:
        m = ctx.build_matrix(seqs, k)
        assert m.count_bytes == 2
        m.close()
    exp = np.stack([oracle.count_kmers(s, 4, k) for s in seqs]).astype(np.uint64)
    got = _five_forms(ctx, seqs, k)
    assert len(got) == 5
    ref = got["host bytes"]
    for form, (counts, totals, bits) in got.items():
        assert (counts == exp).all(), (form, k)
        assert (totals == exp.sum(axis=1)).all(), (form, k)
        assert (bits == ref[2]).all(), (form, k)


@pytest.mark.parametrize("k", [3, 7])
def test_five_states_from_host_and_device_bytes(ctx, k):
    """the byte forms take any alphabet: five states (symbol 4 counts, 5 does not) from both sides of PCIe"""
    import torch

    from diverseseq_amd import engine

    seqs = _sequences()
    data, offsets = engine.concat(seqs)
    dev = torch.zeros(data.size + 16, dtype=torch.uint8, device="cuda:0")
    dev[: data.size] = torch.from_numpy(data.copy()).to("cuda:0")
    torch.cuda.synchronize()
    host = _outputs(ctx.build_matrix(seqs, k, 5))
    device = _outputs(ctx.build_matrix_device(dev.data_ptr(), offsets, k, 5))
    for a, b in zip(host, device):
        assert (a == b).all()
    assert (host[0][5] == oracle.count_kmers(seqs[5], 5, k)).all()


def test_refusals_of_the_source(ctx):
    """an unknown kind, a NULL handle, a misaligned device pointer (the histogram's requirement, not the sketcher's)
    and five states over packed words: refused with their messages, nothing built, and the context works afterwards"""
    import torch

    from diverseseq_amd import _lib, distance, engine

    L = ctx._L
    seqs = _sequences()
    data, offsets = engine.concat(seqs)
    exp = oracle.count_kmers(seqs[5], 4, 3)

    def refused(seqs_struct, code, message, num_states=4):
        for entry, args in ((L.dvs_matrix_build, (3, num_states)), (L.dvs_sketches_build, (8, 64, num_states, 0))):
            h = C.c_void_p()
            assert entry(ctx._h, seqs_struct, *args, C.byref(h)) == code, entry.__name__
            assert message in L.dvs_last_error(ctx._h).decode(), entry.__name__
            assert not h.value
        m = ctx.build_matrix(seqs, 3)
        assert (m.counts()[5] == exp).all()
        m.close()

    refused(_lib.make_seqs(7, data.ctypes.data, offsets, keep=data), _lib.ERR_VALUE, "unknown sequence source kind 7")
    for kind in (_lib.SEQ_HOST, _lib.SEQ_DEVICE, _lib.SEQ_PACKED):
        refused(_lib.make_seqs(kind, None, offsets), _lib.ERR_VALUE, "null argument")
    refused(_lib.make_seqs(_lib.SEQ_BATCH, None), _lib.ERR_VALUE, "null argument")
    refused(None, _lib.ERR_VALUE, "null argument")

    p = ctx.pack_host(data)
    refused(_lib.make_seqs(_lib.SEQ_PACKED, p._h, offsets), _lib.ERR_VALUE, "a packed batch holds four-state sequences", 5)
    with pytest.raises(ValueError, match="a packed batch holds four-state sequences"):
        distance.Sketches(None, 8, 64, 5, ctx=ctx, packed=p, offsets=offsets)
    p.close()
    b = ctx.encode_fasta(_fasta(seqs)).pack()
    refused(_lib.make_seqs(_lib.SEQ_BATCH, b._h), _lib.ERR_VALUE, "a packed batch holds four-state sequences", 5)
    with pytest.raises(ValueError, match="a packed batch holds four-state sequences"):
        b.build_matrix(3, 5)
    b.close()

    # the same bytes at an aligned address and one byte further on
    dev = torch.zeros(data.size + 48, dtype=torch.uint8, device="cuda:0")
    staged = torch.from_numpy(data.copy()).to("cuda:0")
    dev[: data.size] = staged
    odd = torch.zeros(data.size + 48, dtype=torch.uint8, device="cuda:0")
    odd[1: data.size + 1] = staged
    torch.cuda.synchronize()
    assert dev.data_ptr() % 16 == 0 and (odd.data_ptr() + 1) % 16 == 1
    with pytest.raises(ValueError, match="device sequence buffer must be 16-byte aligned"):
        ctx.build_matrix_device(odd.data_ptr() + 1, offsets, 3)
    sketches = []
    for ptr in (dev.data_ptr(), odd.data_ptr() + 1):
        h = distance.Sketches(None, 8, 64, 4, True, ctx=ctx, dev_ptr=ptr, offsets=offsets)
        sketches.append(h.to_host())
        h.close()
    np.testing.assert_array_equal(sketches[0][1], sketches[1][1])
    np.testing.assert_array_equal(sketches[0][0], sketches[1][0])
    assert sketches[0][0][6, : sketches[0][1][6]].tolist() == oracle.mash_sketch(seqs[6], 8, 64, 4, True).tolist()
