"""FASTA files whose state-carrying bytes sit on the seams of the device ingest (csrc/ingest.hip), with the
records they hold known by construction: the 16 bytes of a thread, the 4 KiB step of a block, the 128 KiB
block, the 256-block trip of the single-block scans and the upload chunk of the streamed path.

A file is laid out by `Layout` from three kinds of token -- ("ws", bytes) white space, ("seq", bytes)
sequence characters, ("hdr", label, eol) a header line -- and the layout books what each token means as it
writes it, so labels, sequence texts and header positions never come from parsing the bytes.  A placement
(offset, pattern, split) pads the filler in front of it so that pattern[split] is the byte at `offset`.
tests/test_ingest_seams_host.py pins every small case against the oracle's parser;
tests/test_gpu_ingest_seams.py runs the same cases on the device."""
import functools

import numpy as np

THREAD = 16              # bytes per thread
TILE = 4096              # bytes per block-wide step
BLOCK = 131072           # bytes per block
TRIP = 256               # blocks per trip of the single-block scans

_WS = b"\n\r \t\x00"

# ---------------------------------------------------------------------------------------------- patterns
PATTERNS = {
    "a": [("ws", b"\n"), ("hdr", b"h1 some text", b"\n")],                   # a header start
    "b": [("ws", b"\r\n"), ("hdr", b"h2", b"\r\n")],                         # CRLF around a header
    "c": [("ws", b"\n"), ("hdr", b"", b"\n")],                               # an empty label
    "d": [("ws", b"\n"), ("hdr", b"e1", b"\n"), ("hdr", b"e2", b"\n")],      # an empty record, then another
    "e": [("seq", b"AC>GT")],                                                # '>' not at a line start
    "f": [("ws", b"\n \t\n\n\x00\n")],                                       # white space only
    "g": [("seq", b"N-?ryacguU")],                                           # mixed codes, both cases
}
LITERAL = {
    "a": b"\n>h1 some text\n", "b": b"\r\n>h2\r\n", "c": b"\n>\n", "d": b"\n>e1\n>e2\n", "e": b"AC>GT",
    "f": b"\n \t\n\n\x00\n", "g": b"N-?ryacguU",
}
SHORT = "abcdefg"


def header_pattern(n, tag=b"long header "):
    """'\\n', then a header line of n bytes from its '>' to the byte before its newline, then '\\n'"""
    label = (tag * (n // len(tag) + 1))[: n - 1]
    return [("ws", b"\n"), ("hdr", label, b"\n")]


def sequence_pattern(n):
    """n sequence characters without a line break"""
    return [("seq", (b"ACGTTGCAAC" * (n // 10 + 1))[:n])]


PATTERNS["h300"], PATTERNS["h5000"] = header_pattern(300), header_pattern(5000)      # the growth of labels' window
PATTERNS["i_tile"], PATTERNS["i_block"] = header_pattern(TILE + 40), header_pattern(BLOCK + 40)  # a unit inside a header
PATTERNS["j_tile"], PATTERNS["j_block"] = sequence_pattern(TILE + 40), sequence_pattern(BLOCK + 40)  # a unit, no line break
PATTERNS["x80"] = [("ws", b"\n"), ("hdr", b"caf\xe9 \xff\xfe not utf8 \xc3", b"\n")]  # a label that is not UTF-8

# the last bytes of a file
ENDINGS = {
    "base": [("seq", b"ACG")],
    "lf": [("seq", b"AC"), ("ws", b"\n")],
    "crlf": [("seq", b"AC"), ("ws", b"\r\n")],
    "gt": [("ws", b"\n"), ("hdr", b"", b"")],                                  # '>' alone at a line start
    "gtname": [("ws", b"\n"), ("hdr", b"name", b"")],                          # '>name' without a newline
    "inheader": [("ws", b"\n"), ("hdr", b"a header that began well before the end of the file", b"")],
}


def literal(tokens):
    return b"".join(t[1] if t[0] != "hdr" else b">" + t[1] + t[2] for t in tokens)


for _n, _b in LITERAL.items():
    assert literal(PATTERNS[_n]) == _b, _n


def splits(name):
    """every split of a short pattern: it begins exactly at the boundary (0), every cut inside it, and it ends
    one byte before the boundary (its length)"""
    return [(name, s) for s in range(len(literal(PATTERNS[name])) + 1)]


SHORT_SPLITS = [p for n in SHORT for p in splits(n)]


def long_splits(name, inner):
    """a long pattern's interior is uniform: its first bytes, `inner` cuts inside it and its last bytes"""
    n = len(literal(PATTERNS[name]))
    return [(name, s) for s in (0, 1, 2, *inner, n - 1, n)]


def streams(nbytes, chunk_blocks=TRIP):
    """the host driver's rule: a host file of at least three chunks is uploaded chunk by chunk"""
    return -(-nbytes // BLOCK) >= 3 * chunk_blocks


# ---------------------------------------------------------------------------------------------- the layout
class Layout:
    def __init__(self, seed, alphabet=b"ACGT", crlf=False):
        self.rng = np.random.default_rng(seed)
        self._pool = np.frombuffer(alphabet, dtype=np.uint8)[self.rng.integers(0, len(alphabet), size=1 << 16)].tobytes()
        self._eol = b"\r\n" if crlf else b"\n"
        self._parts, self.pos, self.line_start = [], 0, True
        self.labels, self._texts, self.header_positions = [], [], []
        self.placed = []                      # (offset, name, split, literal)
        self._nfill, self._since, self._next_hdr, self._open_header = 0, 0, 0, False
        self.raw, self.common, self._common_codes = None, 0, {}

    def clone(self):
        """an unfinished layout to go on from (the bytes written so far are shared, the books are copied)"""
        c = Layout.__new__(Layout)
        c.__dict__.update(self.__dict__)
        c.rng = np.random.default_rng(self.pos)
        c._parts, c.labels, c.header_positions = list(self._parts), list(self.labels), list(self.header_positions)
        c._texts, c.placed = [list(t) for t in self._texts], list(self.placed)
        c.common = max(0, len(self._texts) - 1)  # records every clone holds alike: `expected` looks them up once
        return c

    # -- tokens
    def _emit(self, b):
        assert not self._open_header, "nothing may follow a header that ends the file"
        self._parts.append(b)
        self.pos += len(b)

    def ws(self, b):
        assert b and all(ch in _WS for ch in b)
        self._emit(b)
        self.line_start = b.endswith(b"\n")

    def seq(self, b):
        assert b and not (self.line_start and b[:1] == b">") and not any(ch in _WS for ch in b[:64])
        self._emit(b)
        self.line_start = False
        if self._texts:                       # (text in front of the first header belongs to no record)
            self._texts[-1].append(b)

    def hdr(self, label, eol):
        assert self.line_start and b"\n" not in label and eol in (b"", b"\n", b"\r\n")
        self.header_positions.append(self.pos)
        self._emit(b">" + label + eol)
        self.labels.append((label + eol).decode("utf8", "replace").strip())
        self._texts.append([])
        self.line_start, self._open_header = bool(eol), not eol
        self._since = 0

    def run(self, tokens):
        for t in tokens:
            getattr(self, t[0])(*t[1:])

    # -- filler: records of lines of varying width, up to exactly `target`
    def _take(self, n):
        o = int(self.rng.integers(0, len(self._pool) - n))
        return self._pool[o:o + n]

    def fill(self, target, headers=True):
        assert target >= self.pos, ("no room in front of offset", target, self.pos)
        while self.pos < target:
            rem = target - self.pos
            if headers and self.line_start and self._since >= self._next_hdr and rem > 64:
                self.hdr(b"f%d filler record" % self._nfill, self._eol)
                self._nfill += 1
                self._next_hdr = int(self.rng.integers(1, 40))
                continue
            w = int(self.rng.integers(1, 120))
            if rem < w + len(self._eol):
                self.seq(self._take(rem))
            else:
                self.seq(self._take(w))
                self.ws(self._eol)
                self._since += 1

    def place(self, offset, name, split, tokens=None):
        tokens = PATTERNS[name] if tokens is None else tokens
        lit = literal(tokens)
        assert 0 <= split <= len(lit)
        self.fill(offset - split)
        self.run(tokens)
        self.placed.append((offset, name, split, lit))

    def place_next(self, unit, name, split, skip=0, gap=96):
        """the placement on the first multiple of `unit` (no multiple of `skip`) with room for `gap` bytes of filler"""
        offset = -(-(self.pos + gap + split) // unit) * unit
        while skip and offset % skip == 0:
            offset += unit
        self.place(offset, name, split)

    def bulk(self, block, reps):
        """`reps` copies of a finished layout of whole records, as one np.tile"""
        assert self.line_start and block.raw[0] == ord(">") and block.raw[-1] == 10
        for r in range(reps):
            base = self.pos + r * block.raw.size
            self.header_positions += [base + p for p in block.header_positions]
            self._texts += [[t] for t in block._texts]
        self.labels += block.labels * reps
        self._emit(np.tile(block.raw, reps).tobytes())

    def finish(self, expect_placed=None):
        raw = b"".join(self._parts)
        assert len(raw) == self.pos
        for offset, name, split, lit in self.placed:  # every pattern lies where it was asked for
            assert raw[offset - split: offset - split + len(lit)] == lit, (name, offset, split)
        if expect_placed is not None:                 # ... and none was dropped
            assert [(n, s) for _, n, s, _ in self.placed] == list(expect_placed)
        self.raw = np.frombuffer(raw, dtype=np.uint8)
        self._texts = [b"".join(t) for t in self._texts]
        self._parts = None
        return self

    @property
    def seq_texts(self):
        return [t.decode("latin1") for t in self._texts]


def _start(seed, front, alphabet=b"ACGT", crlf=False):
    lay = Layout(seed, alphabet, crlf)
    if front:                                 # text in front of the first header: lines that belong to no record
        lay.fill(front, headers=False)
        lay.ws(b"\n")
    return lay


def build(placements, filler=0, size=0, front=0, alphabet=b"ACGT", crlf=False):
    """placements: (offset, pattern name, split) in ascending order; filler: the seed of the filler records;
    size: the file is filled up to this length; front: bytes of text in front of the first header.
    -> (raw uint8, labels, seq_texts); build_layout gives the Layout (header_positions, placed) instead"""
    lay = build_layout(placements, filler, size, front, alphabet, crlf)
    return lay.raw, lay.labels, lay.seq_texts


def build_layout(placements, filler=0, size=0, front=0, alphabet=b"ACGT", crlf=False):
    lay = _start(filler, front, alphabet, crlf)
    for offset, name, split in placements:
        lay.place(offset, name, split)
    if size:
        lay.fill(size)
    return lay.finish([(n, s) for _, n, s in placements])


def packed_on(unit, items, seed, skip=0, front=0, size=0, tail=None, alphabet=b"ACGT", crlf=False):
    """`items` = (name, split) laid one after the other on successive multiples of `unit` (no multiple of `skip`);
    tail: the file ends that many bytes behind the first multiple of BLOCK behind the last placement"""
    lay = _start(seed, front, alphabet, crlf)
    for name, split in items:
        lay.place_next(unit, name, split, skip, 96 + (int(lay.rng.integers(0, 900)) if unit < TILE else 0))
    if tail is not None:
        size = -(-(lay.pos + 64) // BLOCK) * BLOCK + tail
    if size:
        lay.fill(max(size, lay.pos))
    return lay.finish(items)


# ---------------------------------------------------------------------------------------------- the cases
class Case:
    """name; layout: the finished Layout (built once per maker, however many cases share it); unit: the boundary
    its placements sit on; skip: the coarser unit they keep away from; chunk: the blocks per upload chunk it runs
    with (0: no knob, one copy)"""

    def __init__(self, name, make, unit, chunk=0, skip=0):
        self.name, self.unit, self.chunk, self.skip = name, unit, chunk, skip
        self.make = make if hasattr(make, "cache_info") else functools.lru_cache(maxsize=None)(make)

    @property
    def layout(self):
        return self.make()

    @property
    def knob(self):
        return f"ingest_chunk_{self.chunk}" if self.chunk else None

    @property
    def streamed(self):
        """whether the file reaches the streaming threshold under the knob it runs with"""
        return bool(self.chunk) and streams(self.layout.raw.size, self.chunk)

    def on_unit(self):
        return [(n, s) for off, n, s, _ in self.layout.placed if off % self.unit == 0 and not (self.skip and off % self.skip == 0)]

    def __repr__(self):
        return self.name


_H = long_splits("h300", (150,)) + long_splits("h5000", (256, 257, 2500, 4096, 4097))
_X = splits("x80")[:4]

# thread and tile seams: one file each carries the whole table (one copy, no knob)
ONE_COPY = [
    Case("thread", lambda: packed_on(THREAD, SHORT_SPLITS + _H + _X, 101, skip=TILE, front=40, size=300_000), THREAD, skip=TILE),
    Case("thread_crlf", lambda: packed_on(THREAD, SHORT_SPLITS, 102, skip=TILE, size=100_000, crlf=True), THREAD, skip=TILE),
    Case("tile", lambda: packed_on(TILE, SHORT_SPLITS + _H + _X + long_splits("i_tile", (20, 39)) + long_splits("j_tile", (20, 39)),
                                   103, skip=BLOCK, front=TILE + 100, tail=777), TILE, skip=BLOCK),
]


def _seam_file(i):
    """file i of 13: the five even multiples of BLOCK inside it (the seams of 2-block chunks) carry SHORT_SPLITS[5 i ...],
    the six odd ones another stretch of the table; 12 blocks and a tail of 1 byte, one block, nothing or 70 001 bytes"""
    n = len(SHORT_SPLITS)
    even = [SHORT_SPLITS[(5 * i + j) % n] for j in range(5)]
    odd = [SHORT_SPLITS[(6 * i + j + 32) % n] for j in range(6)]
    lay, items = Layout(200 + i), []
    for b in range(1, 12):
        items.append(even[b // 2 - 1] if b % 2 == 0 else odd[b // 2])
        lay.place(b * BLOCK, *items[-1])
    lay.fill(12 * BLOCK + (1, BLOCK, 0, 70_001)[i % 4])
    return lay.finish(items)


def _front_text():
    """text in front of the first header across the first seam of the blocks and of the 2-block chunks"""
    lay = _start(250, 2 * BLOCK + 100)
    lay.place(3 * BLOCK, "a", 1)
    lay.fill(12 * BLOCK + 1)
    return lay.finish([("a", 1)])


_SEAMS = [Case(f"seam{i:02d}", functools.partial(_seam_file, i), BLOCK) for i in range(13)] + [Case("front_text", _front_text, BLOCK)]
# block seams, one copy: the files of the chunk seams without the knob, and the long patterns
BLOCK_SEAMS = _SEAMS + [
    Case("long_units", lambda: packed_on(BLOCK, [("i_block", 20), ("i_block", 0), ("j_block", 20), ("j_block", BLOCK + 40)], 301,
                                         tail=1), BLOCK),
    Case("long_headers", lambda: packed_on(BLOCK, [("h300", 1), ("h300", 150), ("h300", 301), ("h5000", 2), ("h5000", 257),
                                                   ("h5000", 4999), ("x80", 3)], 302, tail=5), BLOCK),
]
# chunk seams: every multiple of BLOCK with 1-block chunks, the even ones with 2-block chunks
CHUNK1 = [Case(c.name + "_c1", c.make, BLOCK, chunk=1) for c in BLOCK_SEAMS]
CHUNK2 = [Case(c.name + "_c2", c.make, 2 * BLOCK, chunk=2) for c in _SEAMS]


def _exact(nblocks, seed):
    """a file of exactly nblocks blocks with a pattern cut by every seam inside it"""
    def make():
        items = [("a", 1), ("b", 1), ("d", 5), ("e", 2), ("a", 2)][: nblocks - 1]
        lay = Layout(seed)
        for b, (name, split) in enumerate(items, 1):
            lay.place(b * BLOCK, name, split)
        lay.fill(nblocks * BLOCK)
        return lay.finish(items)
    return make


# the threshold: three chunks are streamed, one block less is not
THRESHOLD = [Case("three_chunks_c1", _exact(3, 401), BLOCK, chunk=1), Case("two_blocks_c1", _exact(2, 402), BLOCK, chunk=1),
             Case("three_chunks_c2", _exact(6, 403), BLOCK, chunk=2), Case("five_blocks_c2", _exact(5, 404), BLOCK, chunk=2)]

# the boundary a file ends on (or one byte either side), and the chunk knob it runs with
ENDING_LEVELS = {"thread": (2 * TILE + 7 * THREAD, THREAD, 0), "tile": (3 * TILE, TILE, 0), "block": (3 * BLOCK, BLOCK, 0),
                 "chunk1": (3 * BLOCK, BLOCK, 1), "chunk2": (6 * BLOCK, 2 * BLOCK, 2)}


@functools.lru_cache(maxsize=None)
def _ending_maker(boundary, kind, delta):
    def make():
        lay = Layout(500 + delta)
        n = len(literal(ENDINGS[kind]))
        lay.place(boundary + delta, kind, n, ENDINGS[kind])
        assert lay.pos == boundary + delta
        return lay.finish([(kind, n)])
    return functools.lru_cache(maxsize=None)(make)


def ending_cases(level, kind):
    """files that stop one byte before a boundary of `level`, on it and one byte behind it, their last bytes ENDINGS[kind]"""
    boundary, unit, chunk = ENDING_LEVELS[level]
    return [Case(f"end_{level}_{kind}_{d:+d}", _ending_maker(boundary, kind, d), unit, chunk=chunk) for d in (-1, 0, 1)]


# (the 2-block chunks get the two endings whose last bytes carry the most state; their files are 768 KiB each)
ENDING_CASES = {(lv, kind): ending_cases(lv, kind) for lv in ENDING_LEVELS for kind in ENDINGS
                if lv != "chunk2" or kind in ("crlf", "gtname")}


def _all_bytes():
    """sequence lines that hold all 256 byte values: '\\n' only ends a line, '>' only sits inside one; the lines
    cross two tile seams and three records share them"""
    lay = Layout(600)
    rng = np.random.default_rng(601)
    for r in range(3):
        lay.hdr(b"bytes%d" % r, b"\n")
        for _ in range(12):
            line = [b for b in rng.permutation(256).tolist() if b != 10]
            if line[0] == ord(">"):
                line[0], line[1] = line[1], line[0]
            for b in line:
                (lay.ws if b in _WS else lay.seq)(bytes([b]))
            lay.ws(b"\n")
    return lay.finish()


ALL_BYTES = Case("all_bytes", _all_bytes, TILE)

# a 20-state + gap table (amino acids); every other byte is 255
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY-"
PROTEIN_LUT = np.full(256, 255, dtype=np.uint8)
PROTEIN_LUT[np.frombuffer(PROTEIN, dtype=np.uint8)] = np.arange(len(PROTEIN), dtype=np.uint8)
_PROTEIN_ITEMS = [("a", 1), ("d", 4), ("g", 5), ("c", 2), ("b", 1)]
CUSTOM_TABLE = [
    Case("protein_tile", lambda: packed_on(TILE, _PROTEIN_ITEMS, 701, skip=BLOCK, size=40_000, alphabet=PROTEIN), TILE, skip=BLOCK),
    Case("protein_c1", lambda: packed_on(BLOCK, _PROTEIN_ITEMS, 702, tail=1, alphabet=PROTEIN), BLOCK, chunk=1),
]

# the cases that also run with the RNA table (pattern g holds u and U, the filler T)
RNA = [ONE_COPY[2], CHUNK1[3]]
# the seam file the downstream operations (k-mer counts, pack) start from
DOWNSTREAM = CHUNK1[5]

# every case small enough for the oracle's parser (CHUNK1 / CHUNK2 are files of BLOCK_SEAMS under a knob; the
# "chunk1" endings are the "block" files); CUSTOM_TABLE has a yardstick of its own
SMALL_CASES = ONE_COPY + BLOCK_SEAMS + THRESHOLD + [ALL_BYTES] + \
    [c for (lv, _), cs in ENDING_CASES.items() if lv != "chunk1" for c in cs]

SECOND_TRIP = "abde"


@functools.lru_cache(maxsize=None)
def _second_trip_prefix():
    block = Layout(801)
    block.fill(100_002)          # (no multiple of the block: every copy meets the seams elsewhere)
    block.ws(b"\n")
    block.finish()
    lay = Layout(802)
    lay.bulk(block, (TRIP * BLOCK - TILE) // block.raw.size)
    return lay


def second_trip(name, split):
    """257 blocks: np.tile'd filler records up to a tile before block 256, then one placement on block 256's start
    -- the seam between the first and the second trip of the single-block scans -- and 40 bytes behind it.  Every
    call shares the filler's bytes and books; only the last tile differs."""
    lay = _second_trip_prefix().clone()
    lay.place(TRIP * BLOCK, name, split)
    lay.fill(TRIP * BLOCK + 40)
    return lay.finish([(name, split)])


def expected(lay, join, lut):
    """(codes, offsets) the device must give: the layout's texts through a 256-entry lookup"""
    texts, n, sep = lay._texts, lay.common, (b"-" if join else b"")
    if n:  # (the clones of one 33 MiB prefix share the lookup of its records)
        key = (join, lut.tobytes())
        if key not in lay._common_codes:
            lay._common_codes[key] = lut[np.frombuffer(sep.join(texts[:n]) + sep, dtype=np.uint8)]
        codes = np.concatenate([lay._common_codes[key], lut[np.frombuffer(sep.join(texts[n:]), dtype=np.uint8)]])
    else:
        codes = lut[np.frombuffer(sep.join(texts), dtype=np.uint8)]
    sizes = [codes.size] if join else [len(t) for t in texts]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64) if texts else np.zeros(1, np.uint64)
    return codes, offsets
