"""The device FASTA ingest (csrc/ingest.hip) at every seam of its scans and uploads: the files of
tests/ingest_cases.py put the bytes that carry state -- a newline in front of '>', the '\\r' of a CRLF, a '>'
inside a line, an empty record, the end of the file -- on the 16-byte, 4 KiB and 128 KiB boundaries, on the seams
between upload chunks (DVS_TEST_KNOBS=ingest_chunk_<n>) and on the start of block 256, where the single-block
scans begin their second trip.  Every comparison is exact, against records the builder knows by construction
(pinned to the oracle's parser by tests/test_ingest_seams_host.py)."""
import ctypes as C

import numpy as np
import pytest

import ingest_cases as ic
import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from diverseseq_amd import engine

    return engine.default_context()


_LUTS = {}


def _lut(moltype="dna"):
    if moltype not in _LUTS:
        _LUTS[moltype] = oracle.str2arr(bytes(range(256)).decode("latin1"), moltype)
    return _LUTS[moltype]


def _same(b, lay, join, lut, labels=True, what=""):
    """the batch holds exactly what the layout says: records, offsets, header positions, every code, the labels
    (labels: True they are the layout's, False there are none, None they are not read)"""
    codes, offsets = ic.expected(lay, join, lut)
    nrec = len(lay.labels)
    assert b.nrecords == nrec and b.nseq == (min(nrec, 1) if join else nrec), (what, b.nrecords, b.nseq, nrec)
    hp = np.asarray(lay.header_positions, dtype=np.uint64)
    assert b.header_positions.size == hp.size
    assert (b.header_positions == hp).all(), (what, "header", int(np.flatnonzero(b.header_positions != hp)[0]))
    assert b.offsets.size == offsets.size
    assert (b.offsets == offsets).all(), (what, "offset", int(np.flatnonzero(b.offsets != offsets)[0]))
    got = b.codes()
    assert got.size == codes.size == b.total, (what, got.size, codes.size)
    assert (got == codes).all(), (what, "code", int(np.flatnonzero(got != codes)[0]))
    if labels is True:
        assert b.labels == lay.labels, what
    elif labels is False:
        assert b.labels is None
    return got


def _encode_and_check(ctx, lay, lut=None, moltype="dna", what=""):
    out = []
    for join in (False, True):
        b = ctx.encode_fasta(lay.raw, join_records=join, moltype=moltype)
        out.append((_same(b, lay, join, _lut(moltype) if lut is None else lut, what=(what, join)), b.offsets.copy(),
                    b.header_positions.copy()))
        b.close()
    return out


def _against_oracle(ctx, raw, moltype="dna"):
    """as _check of test_ingest.py"""
    for join in (False, True):
        labels, seqs = oracle.load_fasta(raw.tobytes(), join_records=join, moltype=moltype)
        b = ctx.encode_fasta(raw, join_records=join, moltype=moltype)
        assert b.labels == labels and b.nseq == len(seqs)
        exp_off = np.concatenate([[0], np.cumsum([s.size for s in seqs])]).astype(np.uint64) if seqs else np.zeros(1, np.uint64)
        assert b.offsets.tolist() == exp_off.tolist()
        got, exp = b.codes(), (np.concatenate(seqs) if seqs else np.zeros(0, np.uint8))
        assert got.size == exp.size
        assert (got == exp).all(), int(np.flatnonzero(got != exp)[0])
        b.close()


def _streamed_and_whole(ctx, monkeypatch, case, lut=None, moltype="dna"):
    """the case under its chunk knob (streamed where its size reaches three chunks) and with DVS_INGEST_NO_STREAM:
    both exactly the builder's records, hence the same arrays"""
    monkeypatch.setenv("DVS_TEST_KNOBS", case.knob)
    a = _encode_and_check(ctx, case.layout, lut, moltype, what=(case.name, "streamed" if case.streamed else "one copy"))
    monkeypatch.setenv("DVS_INGEST_NO_STREAM", "1")
    b = _encode_and_check(ctx, case.layout, lut, moltype, what=(case.name, "no stream"))
    for x, y in zip(a, b):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    monkeypatch.delenv("DVS_INGEST_NO_STREAM")
    monkeypatch.delenv("DVS_TEST_KNOBS")
    return a


# ------------------------------------------------------------------ thread, tile and block seams, one copy
@pytest.mark.parametrize("case", ic.ONE_COPY, ids=repr)
def test_thread_and_tile_seams(ctx, case):
    """every pattern at every split on multiples of 16 B (away from the 4 KiB lines) and of 4 KiB (away from the
    128 KiB lines); against the builder and against the oracle"""
    assert not case.streamed
    _encode_and_check(ctx, case.layout, what=case.name)
    _against_oracle(ctx, case.layout.raw)


# ------------------------------------------------------------------ block seams (one copy) and chunk seams (streamed)
@pytest.mark.parametrize("case", ic.CHUNK1 + ic.CHUNK2 + ic.THRESHOLD, ids=repr)
def test_block_and_chunk_seams(ctx, monkeypatch, case):
    """the same patterns on multiples of 128 KiB: streamed in chunks of one block (every multiple is a chunk seam)
    and of two blocks (every even one is), six chunks and more so that the four copy events are reused, the last
    chunk one byte, one block or a whole one; each file again in one copy, where the same bytes sit on block seams.
    Three chunks exactly are streamed, one block less is not."""
    _streamed_and_whole(ctx, monkeypatch, case)


@pytest.mark.parametrize("level,kind", list(ic.ENDING_CASES), ids=lambda v: str(v))
def test_the_file_ends_on_a_seam(ctx, monkeypatch, level, kind):
    """the file stops exactly on a boundary, one byte before it and one byte behind it, its last bytes a base, LF,
    CRLF, a lone '>', '>name' without a newline or the inside of a header"""
    for case in ic.ENDING_CASES[(level, kind)]:
        if case.chunk:
            assert case.streamed
            _streamed_and_whole(ctx, monkeypatch, case)
        else:
            _encode_and_check(ctx, case.layout, what=case.name)
            if case.layout.raw.size < 20_000:
                _against_oracle(ctx, case.layout.raw)


# ------------------------------------------------------------------ the same bytes from the device
@pytest.mark.parametrize("case", [ic.ONE_COPY[0], ic.ONE_COPY[2], ic.BLOCK_SEAMS[3], ic.BLOCK_SEAMS[14]], ids=repr)
def test_bytes_already_on_the_device(ctx, case):
    """encode_fasta(None, dev_ptr=, nbytes=): no labels, everything else as from the host; the bytes are left alone"""
    import torch

    lay = case.layout
    t = torch.from_numpy(lay.raw.copy()).cuda()
    for join in (False, True):
        b = ctx.encode_fasta(None, join_records=join, dev_ptr=t.data_ptr(), nbytes=t.numel())
        _same(b, lay, join, _lut(), labels=False, what=(case.name, "device", join))
        b.close()
    assert np.array_equal(t.cpu().numpy(), lay.raw)


# ------------------------------------------------------------------ second trip of the single-block scans
@pytest.mark.parametrize("name", ic.SECOND_TRIP)
def test_second_trip_of_the_single_block_scans(ctx, name):
    """257 blocks (the 256 blocks of a trip are a compile-time constant, so this cannot be smaller): a pattern at
    every split on block 256's start, whose carries are the first trip's totals; from the host (one copy: under
    96 MiB) and from the device; against the builder"""
    import torch

    t, first, tail = None, None, ic.BLOCK  # (the files share all but their last 100 KB of filler)
    for _, split in ic.splits(name):
        lay = ic.second_trip(name, split)
        assert lay.raw.size == ic.TRIP * ic.BLOCK + 40 and not ic.streams(lay.raw.size)
        if t is None:
            t, first = torch.from_numpy(lay.raw.copy()).cuda(), lay.raw
        else:
            assert np.array_equal(lay.raw[:-tail], first[:-tail])
            t[-tail:] = torch.from_numpy(lay.raw[-tail:].copy()).cuda()
        for join in (False, True):
            b = ctx.encode_fasta(lay.raw, join_records=join)
            # (the labels -- tens of thousands of host slices -- are read at one split per pattern)
            _same(b, lay, join, _lut(), labels=True if split == 1 and not join else None, what=(name, split, "host", join))
            b.close()
            b = ctx.encode_fasta(None, join_records=join, dev_ptr=t.data_ptr(), nbytes=t.numel())
            _same(b, lay, join, _lut(), labels=False, what=(name, split, "device", join))
            b.close()
    assert np.array_equal(t[-tail:].cpu().numpy(), lay.raw[-tail:])


# ------------------------------------------------------------------ overflow of the record arrays
@pytest.mark.parametrize("streamed", [False, True], ids=["one_copy", "streamed"])
def test_record_arrays_overflow_on_a_seam_file(ctx, monkeypatch, streamed):
    """room for 1, 3 and nrec - 1 records: the flag is raised and the last pass repeated over the whole file; room
    for nrec: no overflow; the arrays are those of the run without the knob"""
    case = ic.CHUNK1[2]
    lay, nrec = case.layout, len(case.layout.labels)
    assert nrec > 100 and case.streamed
    base = case.knob if streamed else ""
    if base:
        monkeypatch.setenv("DVS_TEST_KNOBS", base)
    plain = _encode_and_check(ctx, lay, what="no reccap")
    for cap in (1, 3, nrec - 1, nrec):
        monkeypatch.setenv("DVS_TEST_KNOBS", ",".join(k for k in (base, f"ingest_reccap_{cap}") if k))
        got = _encode_and_check(ctx, lay, what=("reccap", cap))
        for x, y in zip(plain, got):
            assert all(np.array_equal(p, q) for p, q in zip(x, y)), cap


# ------------------------------------------------------------------ alphabets
@pytest.mark.parametrize("case", ic.RNA, ids=repr)
def test_rna_table_on_seam_files(ctx, monkeypatch, case):
    """moltype="rna": U and T are both index 0, as in the oracle's table"""
    assert _lut("rna")[ord("U")] == _lut("rna")[ord("t")] == 0
    if case.chunk:
        _streamed_and_whole(ctx, monkeypatch, case, moltype="rna")
    else:
        _encode_and_check(ctx, case.layout, moltype="rna", what=case.name)
        _against_oracle(ctx, case.layout.raw, "rna")


@pytest.mark.parametrize("moltype", ["dna", "rna"])
def test_all_256_byte_values(ctx, moltype):
    """sequence lines of every byte value: '\\n' only ends a line, '>' only sits inside one; against oracle.str2arr"""
    lay = ic.ALL_BYTES.layout
    for join in (False, True):
        texts = ["-".join(lay.seq_texts)] if join else lay.seq_texts
        b = ctx.encode_fasta(lay.raw, join_records=join, moltype=moltype)
        got = b.sequences()
        assert len(got) == len(texts) and b.labels == lay.labels
        for g, t in zip(got, texts):
            e = oracle.str2arr(t, moltype)
            assert g.size == e.size
            assert (g == e).all(), int(np.flatnonzero(g != e)[0])
        b.close()
    _encode_and_check(ctx, lay, moltype=moltype)


def _encode_with_table(ctx, raw, lut, join):
    from diverseseq_amd import _lib, engine

    h = C.c_void_p()
    ctx.check(ctx._L.dvs_seqbatch_from_fasta(ctx._h, C.c_void_p(raw.ctypes.data), 0, raw.size, _lib.ptr(lut, C.c_uint8), int(join),
                                             C.byref(h)))
    return engine.SeqBatch(ctx, h, raw)


@pytest.mark.parametrize("case", ic.CUSTOM_TABLE, ids=repr)
def test_a_callers_own_table(ctx, monkeypatch, case):
    """a 20-state + gap table through dvs_seqbatch_from_fasta: the codes are the numpy lookup of the parsed texts,
    the joined batch carries lut['-'] between records, and such a batch does not pack"""
    lay, lut = case.layout, ic.PROTEIN_LUT
    if case.knob:
        monkeypatch.setenv("DVS_TEST_KNOBS", case.knob)
        assert case.streamed
    recs = oracle.parse_fasta(lay.raw.tobytes())
    for join in (False, True):
        b = _encode_with_table(ctx, lay.raw, lut, join)
        got = _same(b, lay, join, lut, what=(case.name, join))
        texts = ["-".join(s for _, s in recs)] if join else [s for _, s in recs]
        exp = lut[np.frombuffer("".join(texts).encode("latin1"), dtype=np.uint8)]
        assert np.array_equal(got, exp)
        if join:
            ends = np.cumsum([len(s) + 1 for _, s in recs])[:-1] - 1   # the gap behind every record but the last
            assert (got[ends] == lut[ord("-")]).all() and lut[ord("-")] == 20
        with pytest.raises(ValueError, match="DNA / RNA alphabet"):
            b.pack()
        assert b.packed is None and np.array_equal(b.codes(), got)
        b.close()


# ------------------------------------------------------------------ downstream of a seam file
def test_counts_and_pack_downstream_of_a_streamed_seam_file(ctx, monkeypatch):
    """the batch of a file streamed in 1-block chunks feeds the histogram and the pack kernel: k-mer counts of the
    builder's sequences (joined: no k-mer spans a gap), the packed form reads every symbol >= 4 as invalid, and
    poisoned device blocks change no bit"""
    case = ic.DOWNSTREAM
    lay, lut = case.layout, _lut()
    monkeypatch.setenv("DVS_TEST_KNOBS", case.knob)
    assert case.streamed
    seqs = [lut[np.frombuffer(t, dtype=np.uint8)] for t in lay._texts]
    kept = {}
    for join in (False, True):
        b = ctx.encode_fasta(lay.raw, join_records=join)
        kept[join] = _same(b, lay, join, lut, what=("downstream", join))
        for k in (3, 6):
            m = b.build_matrix(k)
            counts = m.counts()
            per_record = np.stack([oracle.count_kmers(s, 4, k) for s in seqs])
            if join:
                assert counts.shape[0] == 1
                assert (counts[0] == per_record.sum(axis=0)).all()  # nothing counted across a gap
                assert (counts[0] == oracle.count_kmers(kept[True], 4, k)).all()
            else:
                assert counts.shape == per_record.shape
                assert (counts == per_record).all(), int(np.flatnonzero((counts != per_record).any(axis=1))[0])
            m.close()
        b.pack()
        assert b.packed is not None
        exp = np.where(kept[join] >= 4, 255, kept[join]).astype(np.uint8)
        got = b.codes()
        assert (got == exp).all(), int(np.flatnonzero(got != exp)[0])
        m = b.build_matrix(3)
        assert (m.counts().sum(axis=0) == np.stack([oracle.count_kmers(s, 4, 3) for s in seqs]).sum(axis=0)).all()
        m.close()
        b.close()
    monkeypatch.setenv("DVS_TEST_KNOBS", "poison_blocks," + case.knob)
    for join in (False, True):
        b = ctx.encode_fasta(lay.raw, join_records=join)
        assert np.array_equal(_same(b, lay, join, lut, what=("poisoned", join)), kept[join])
        b.close()


# ------------------------------------------------------------------ GenBank
def test_genbank_with_crlf_empty_and_without_records(ctx):
    from test_ingest import GENBANK

    for raw in (GENBANK.replace(b"\n", b"\r\n"), b"", b"no records here\n", b"no records here\r\n"):
        for join in (False, True):
            labels, seqs = oracle.load_genbank(raw, join_records=join)
            b = ctx.encode_genbank(raw, join_records=join)
            assert b.labels == labels and b.nseq == len(seqs) and b.nrecords == len(labels)
            got = b.sequences()
            assert len(got) == len(seqs)
            for g, e in zip(got, seqs):
                assert np.array_equal(g, e)
            b.close()
    assert oracle.load_genbank(GENBANK.replace(b"\n", b"\r\n"))[0] == ["SCU49845", "NOSEQ", "SECOND"]


# ------------------------------------------------------------------ labels
def test_labels_of_long_crlf_unterminated_and_non_utf8_headers(ctx):
    """headers of 300 and 5 000 bytes (the window of SeqBatch.labels grows 256 -> 4 096 -> 65 536), a CRLF header,
    bytes >= 0x80 that are not UTF-8, and a header that ends the file without a newline: the oracle's labels"""
    lay = ic.Layout(900)
    for name in ("h300", "b", "h5000", "x80", "h300", "c"):
        lay.place_next(ic.THREAD, name, 1)
    lay.fill(lay.pos + 200)
    lay.run([("ws", b"\r\n"), ("hdr", b"the last header, cut by the end of the file \xe9", b"")])
    lay.finish()
    labels = oracle.load_fasta(lay.raw.tobytes())[0]
    assert max(len(x) for x in labels) == 4999 and sorted(len(x) for x in labels)[-3:-1] == [299, 299]
    assert "�" in labels[-1] and any("�" in x for x in labels[:-1]) and "h2" in labels and "" in labels
    for join in (False, True):
        b = ctx.encode_fasta(lay.raw, join_records=join)
        assert b.labels == labels == lay.labels
        _same(b, lay, join, _lut())
        b.close()
    b = ctx.encode_fasta(lay.raw.tobytes())  # (bytes, as a caller hands a file over)
    assert b.labels == labels
    b.close()
