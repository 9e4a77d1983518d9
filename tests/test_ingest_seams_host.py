"""The seam files of tests/ingest_cases.py against the oracle's FASTA parser: what the builder says a file
holds (labels, sequence texts, header positions) is what oracle.load_fasta reads from its bytes, and every
placement sits on the boundary its case names.  tests/test_gpu_ingest_seams.py imports the same case lists, so
the device is compared with records that were pinned here."""
import numpy as np
import pytest

import ingest_cases as ic
import oracle


def _pin(lay, moltype="dna"):
    raw = lay.raw.tobytes()
    labels, seqs = oracle.load_fasta(raw, moltype=moltype)
    assert labels == lay.labels
    texts = lay.seq_texts
    assert len(seqs) == len(texts)
    for i, (s, t) in enumerate(zip(seqs, texts)):
        assert np.array_equal(s, oracle.str2arr(t, moltype)), i
    jl, js = oracle.load_fasta(raw, join_records=True, moltype=moltype)
    assert jl == lay.labels and len(js) == (1 if texts else 0)
    if texts:
        assert np.array_equal(js[0], oracle.str2arr("-".join(texts), moltype))
    # the header positions: every one a '>' behind a newline (or at the file's start), and no other such byte
    hp = np.asarray(lay.header_positions, dtype=np.int64)
    gt = np.flatnonzero(lay.raw == ord(">"))
    initial = gt[(gt == 0) | (lay.raw[np.maximum(gt, 1) - 1] == 10)]
    assert hp.tolist() == initial.tolist()
    # ... and the byte lookup the device tests compare with is the oracle's str2arr
    lut = oracle.str2arr(bytes(range(256)).decode("latin1"), moltype)
    for join in (False, True):
        codes, offsets = ic.expected(lay, join, lut)
        exp = js if join else seqs
        assert offsets.tolist() == np.concatenate([[0], np.cumsum([s.size for s in exp])]).astype(np.uint64).tolist()
        assert np.array_equal(codes, np.concatenate(exp) if exp else np.zeros(0, np.uint8))


def test_the_pattern_table():
    """the literal bytes of the issue's table are what the token programs write; every split of every short
    pattern is in the list that the seam files are cut from"""
    assert ic.literal(ic.PATTERNS["a"]) == b"\n>h1 some text\n"
    assert ic.literal(ic.PATTERNS["b"]) == b"\r\n>h2\r\n"
    assert ic.literal(ic.PATTERNS["c"]) == b"\n>\n"
    assert ic.literal(ic.PATTERNS["d"]) == b"\n>e1\n>e2\n"
    assert ic.literal(ic.PATTERNS["e"]) == b"AC>GT"
    assert ic.literal(ic.PATTERNS["f"]) == b"\n \t\n\n\x00\n"
    assert ic.literal(ic.PATTERNS["g"]) == b"N-?ryacguU"
    assert len(ic.literal(ic.PATTERNS["h300"])) == 302 and len(ic.literal(ic.PATTERNS["h5000"])) == 5002
    assert len(ic.literal(ic.PATTERNS["i_tile"])) == ic.TILE + 42 and len(ic.literal(ic.PATTERNS["j_block"])) == ic.BLOCK + 40
    assert len(ic.SHORT_SPLITS) == sum(len(ic.LITERAL[n]) + 1 for n in ic.SHORT) == 63
    with pytest.raises(UnicodeDecodeError):
        ic.PATTERNS["x80"][1][1].decode("utf8")


def test_build_places_every_pattern_or_fails():
    raw, labels, texts = ic.build([(4096, "a", 1), (8192, "e", 2), (8192 + 160, "d", 4)], filler=3, size=9000, front=30)
    assert raw.size == 9000 and raw[4095] == 10 and raw[4096] == ord(">") and bytes(raw[8190:8195]) == b"AC>GT"
    assert labels.count("h1 some text") == 1 and labels[-2:] == ["e1", "e2"] and texts[-2] == ""
    assert oracle.parse_fasta(raw.tobytes()) == list(zip(labels, texts))
    with pytest.raises(AssertionError):  # no room: the second placement would start inside the first
        ic.build([(4096, "a", 1), (4100, "e", 0)])
    with pytest.raises(AssertionError):  # a header that ends the file is the last thing in it
        lay = ic.Layout(0)
        lay.place(100, "gt", 2, ic.ENDINGS["gt"])
        lay.fill(200)


@pytest.mark.parametrize("case", ic.SMALL_CASES, ids=repr)
def test_seam_files_hold_what_the_builder_says(case):
    lay = case.layout
    assert lay.raw.size <= 1_750_000
    _pin(lay)
    for off, name, split, lit in lay.placed:
        assert bytes(lay.raw[off - split: off - split + len(lit)]) == lit
        assert off % (case.unit if case.unit <= ic.BLOCK else ic.BLOCK) == 0 or name in ic.ENDINGS


@pytest.mark.parametrize("case", ic.RNA, ids=repr)
def test_rna_cases(case):
    assert any(name == "g" for _, name, _, _ in case.layout.placed)
    _pin(case.layout, "rna")


@pytest.mark.parametrize("case", ic.CUSTOM_TABLE, ids=repr)
def test_custom_table_cases(case):
    """yardstick: oracle.parse_fasta and a numpy lookup in the caller's table"""
    lay = case.layout
    recs = oracle.parse_fasta(lay.raw.tobytes())
    assert [lab for lab, _ in recs] == lay.labels and [s for _, s in recs] == lay.seq_texts
    for join in (False, True):
        codes, offsets = ic.expected(lay, join, ic.PROTEIN_LUT)
        texts = ["-".join(s for _, s in recs)] if join else [s for _, s in recs]
        assert np.array_equal(codes, ic.PROTEIN_LUT[np.frombuffer("".join(texts).encode("latin1"), dtype=np.uint8)])
        assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(t) for t in texts])]).tolist()
    assert ic.PROTEIN_LUT[ord("-")] == 20 and (codes == 20).sum() >= len(recs) - 1
    assert case.streamed == (case.chunk == 1)


def test_where_the_placements_sit():
    """each case's conditions: the boundary its placements are on, the coarser one they avoid, and the whole table
    of splits on every kind of seam"""
    thread, thread_crlf, tile = ic.ONE_COPY
    for case in ic.ONE_COPY:
        for off, name, split, _ in case.layout.placed:
            assert off % case.unit == 0 and off % case.skip != 0, (case, name, split)
        assert set(case.on_unit()) >= set(ic.SHORT_SPLITS) and not case.streamed and case.knob is None
    assert 300_000 <= thread.layout.raw.size <= 600_000 and 300_000 <= tile.layout.raw.size <= 700_000
    assert b"\r\n" in thread_crlf.layout.raw.tobytes() and b"\r\n>f" in thread_crlf.layout.raw.tobytes()
    # text in front of the first header crosses the first boundary of its level
    assert thread.layout.header_positions[0] > ic.THREAD and tile.layout.header_positions[0] > ic.TILE
    assert ic.BLOCK_SEAMS[13].name == "front_text" and ic.BLOCK_SEAMS[13].layout.header_positions[0] > 2 * ic.BLOCK
    # a whole tile / block inside one header, and inside one line of sequence
    for case, unit in ((tile, ic.TILE), (ic.BLOCK_SEAMS[14], ic.BLOCK)):
        raw, inside = case.layout.raw, {"i": 0, "j": 0}
        for off, name, split, lit in case.layout.placed:
            if name[0] in "ij" and 0 < split <= 40:
                assert 10 not in raw[off:off + unit].tolist() and raw[off - split] in (10, ord("A"))
                inside[name[0]] += 1
        assert inside["i"] >= 1 and inside["j"] >= 1
    # block seams (one copy) and the seams of 1-block chunks: every split on a multiple of BLOCK
    on_block = [p for c in ic.BLOCK_SEAMS for p in c.on_unit()]
    assert set(on_block) >= set(ic.SHORT_SPLITS)
    assert [c.layout is b.layout for c, b in zip(ic.CHUNK1, ic.BLOCK_SEAMS)] == [True] * len(ic.BLOCK_SEAMS)
    # the seams of 2-block chunks: every split on a multiple of 2 BLOCK, in the same files
    on_chunk2 = [p for c in ic.CHUNK2 for p in c.on_unit()]
    assert set(on_chunk2) >= set(ic.SHORT_SPLITS)
    for c in ic.CHUNK1 + ic.CHUNK2:
        nb = -(-c.layout.raw.size // ic.BLOCK)
        assert c.streamed and nb >= 6 * c.chunk, c   # six chunks and more: the four copy events (NSLOT) are reused
    for c in ic.BLOCK_SEAMS:
        assert not c.streamed and c.knob is None
    # the last chunk: one byte, one block of two, a whole one
    last = {c.layout.raw.size % (2 * ic.BLOCK) for c in ic.CHUNK2}
    assert {1, ic.BLOCK, 0} <= last
    assert {1, 0} <= {c.layout.raw.size % ic.BLOCK for c in ic.CHUNK1}


def test_the_streaming_threshold_cases():
    t3, t2, s6, s5 = ic.THRESHOLD
    assert t3.layout.raw.size == 3 * ic.BLOCK and t3.streamed and t3.knob == "ingest_chunk_1"
    assert t2.layout.raw.size == 2 * ic.BLOCK and not t2.streamed
    assert s6.layout.raw.size == 6 * ic.BLOCK and s6.streamed and s6.knob == "ingest_chunk_2"
    assert s5.layout.raw.size == 5 * ic.BLOCK and not s5.streamed
    assert not ic.streams(96 * 2**20 - ic.BLOCK) and ic.streams(96 * 2**20 - ic.BLOCK + 1)  # without a knob: 768 blocks, 96 MiB
    assert ic.streams(3 * ic.BLOCK - 1, 1) and not ic.streams(2 * ic.BLOCK, 1)


def test_the_endings():
    """each file stops exactly on its boundary, one byte before it and one byte behind it, with the named last bytes"""
    assert set(ic.ENDINGS) == {"base", "lf", "crlf", "gt", "gtname", "inheader"}
    for lv in ("thread", "tile", "block", "chunk1"):
        assert {k for l, k in ic.ENDING_CASES if l == lv} == set(ic.ENDINGS)
    for (level, kind), cases in ic.ENDING_CASES.items():
        boundary, unit, chunk = ic.ENDING_LEVELS[level]
        assert boundary % unit == 0 and [c.layout.raw.size - boundary for c in cases] == [-1, 0, 1]
        for c in cases:
            raw = c.layout.raw.tobytes()
            assert raw.endswith(ic.literal(ic.ENDINGS[kind])) and c.chunk == chunk
            assert c.streamed == (chunk > 0)
            if kind in ("gt", "gtname", "inheader"):
                assert c.layout.header_positions[-1] == len(raw) - len(ic.literal(ic.ENDINGS[kind])) + 1
                assert c.layout.seq_texts[-1] == ""
        if level == "chunk1":
            assert all(c.layout is b.layout for c, b in zip(cases, ic.ENDING_CASES[("block", kind)]))
    inh = len(ic.literal(ic.ENDINGS["inheader"]))
    assert inh > 3 * ic.THREAD  # the header's '>' lies in another thread's bytes than the end of the file


def test_the_all_bytes_file():
    lay = ic.ALL_BYTES.layout
    assert set(lay.raw.tolist()) == set(range(256)) and lay.raw.size > 2 * ic.TILE
    raw = lay.raw
    gt = np.flatnonzero(raw == ord(">"))
    inner = gt[raw[gt - 1] != 10]
    assert inner.size == 36 and len(lay.labels) == 3
    for t in lay.seq_texts:
        assert len(t) == 12 * (255 - 4)  # every byte but '\n' and the four other white-space bytes, per line


def test_the_second_trip_file_is_what_the_builder_says_at_a_small_scale():
    """the 33 MiB file itself is not parsed by the oracle; the same construction (np.tile'd records, a clone per
    placement) is, with a short prefix"""
    block = ic.Layout(801)
    block.fill(5_002)
    block.ws(b"\n")
    block.finish()
    pre = ic.Layout(802)
    pre.bulk(block, 7)
    for name, split in (("a", 1), ("d", 4), ("e", 2)):
        lay = pre.clone()
        lay.place(40_000, name, split)
        lay.fill(40_040)
        lay.finish([(name, split)])
        assert lay.raw.size == 40_040
        _pin(lay)
    assert pre.pos == 7 * block.raw.size and len(pre._parts) == 1
    assert len(ic.SECOND_TRIP) == 4 and ic.TRIP == 256
