"""The layouts of tests/test_gpu_far_rows.py, pinned on the CPU before they are used on the device.

Every kernel that touches a count row computes `mat + row * B`.  A matrix of a production size has more than 2^32
elements, and no other test puts a row at an element index of 2^32 or more: a product that lost its 64-bit cast would
wrap, row r* + j would read row j, and nothing would notice.  The layouts here put real rows behind the boundary at
the price of the empty rows in front of them: a selection skips a row without a valid k-mer, such a row costs the
oracle nothing, and a stream of a million of them is an offsets array.

A row is B = 4^k bins wide, r* = 2^32 / B is the first row that starts at element 2^32, h* = 2^31 / B the first at
2^31.  A layout has N = r* + 293 rows.  The REAL rows -- seeded sequences of 600 to 1500 bases, each with a base
composition of its own and a few invalid symbols -- sit at positions 0 .. 7, at h* - 1, h*, h* + 1, in the contiguous
block r* - 2 .. r* + 93 and in the last 16 rows; two rows behind the boundary are exact copies of one another (PAIR).
Every other row has no valid k-mer: length 0, and near h*, r* and the end a mix of length 0, length k - 1 and twenty
invalid symbols.  So a product that wraps at 2^32 reads a front row or an empty row in place of a far one, and one that
goes negative at 2^31 reads outside the matrix.

The TWIN of a layout is the same real sequences alone, in the same order, as a small matrix: twin row i is far row
`real_positions(layout)[i]`.  Whatever is a function of the rows' contents must come out of both with the same bits --
address arithmetic is all that differs.

This module holds the layouts, their arithmetic, the row lists and the long-double truth of the distance checks, and
the conditions under which the cases say something, checked from the oracle alone:

  * at least 90 real rows start at element 2^32 or beyond, row r* - 1 ends exactly at the boundary, N B > 2^32;
  * except for the planted pair no two real rows are equal;
  * `oracle.nmost` over the real rows, n = 40, accepts at least 8 rows beyond the seeds and ends with at least 20
    members at positions >= r*; `oracle.max_divergent(4, 30, "stdev")` keeps at least 4 pushes and ends with at least 3
    members >= r*;
  * the tie case really presents a copy of the set's lowest member as the next candidate.

Which run the nmost conditions describe.  The reference seeds a selection with the first n records OF THE STREAM and drops
those without a valid k-mer (src/records.rs:299-306): nmost(40) over the whole layout is seeded by rows 0 .. 39, of which
only 0 .. 7 are real, and keeps a set of 8.  So "the oracle over the real rows alone, n = 40" is the answer to nmost(40)
with an explicit order that lists the real rows' positions -- the run the two nmost conditions above are about -- and
not to nmost(40) without an order, whose answer is the oracle over the real rows with n = 8 (`oracle_nmost_whole`;
`test_whole_stream_nmost_is_seeded_by_the_front_rows` pins that equivalence on the oracle).  That run is the only form
of nmost the persistent engine takes, so it has a condition of its own: at least MIN_WHOLE_FAR of its accepts take a
row >= r*, and at least MIN_WHOLE_FAR members lie >= r* at the end -- the engine replaces its lowest member by far rows,
fetches them as members and scans on against them.  No more can be asked of rows this short: the reference's score
has no clamp, the first replacements leave the running sum a rounding error below the lowest member's frequency in
some bin, and from then on every candidate that misses such a bin scores NaN and is rejected (the oracle does the
same) -- a set of 8 stops accepting after a handful of accepts (8, 5 and 6 here).  The seeds are searched for all of these conditions together
(about one seed in 1 000 at 4^6 bins, one in 13 000 at 4^7).  max_divergent(4, 30) is
seeded by rows 0 .. 3 either way."""
import functools
from typing import NamedTuple

import numpy as np
import pytest

import oracle
from test_distance_truth_host import truth_euclid_rows, truth_jsd_rows

TAIL = 293                 # rows behind r*
N_SELECT = 40              # nmost(40)
MAX_ARGS = (4, 30, "stdev")
MIN_ACCEPTS, MIN_FAR_MEMBERS = 8, 20
MIN_PUSHES, MIN_FAR_MAX_MEMBERS = 4, 3
MIN_FAR_REAL = 90
MIN_WHOLE_FAR = 2          # whole-stream nmost: accepts of rows >= r*, and members >= r* at the end, at least
INVALID_RUN = 20           # a filler row of twenty invalid symbols
NEAR = 16                  # rows on either side of h* whose fillers are the mix (and every filler from r* - NEAR on)


class Layout(NamedTuple):
    name: str
    k: int
    count_bytes: int   # width of a count on the device
    engine_nmost: int  # summary().engine of nmost(40) over the whole matrix: 1 persistent, 0 multi-launch
    engine_max: int    # ... of max_divergent (the persistent engine takes `max` up to 4096 bins only, csrc/persist.hip)
    seed: int

    @property
    def nbins(self):
        return 4 ** self.k

    @property
    def r_star(self):
        return (1 << 32) // self.nbins

    @property
    def h_star(self):
        return (1 << 31) // self.nbins

    @property
    def nrows(self):
        return self.r_star + TAIL

    @property
    def nbytes(self):
        return self.nrows * self.nbins * self.count_bytes


LAYOUTS = (Layout("u16-k6", 6, 2, 1, 1, 1382), Layout("u32-k7", 7, 4, 1, 0, 36706), Layout("u32-k9", 9, 4, 0, 0, 186))

# twin rows: 0 .. 7 the front, 8 .. 10 the rows at h*, 11 .. 106 the block r* - 2 .. r* + 93, 107 .. 122 the last 16
N_REAL = 8 + 3 + 96 + 16
FIRST_FAR = 13                           # the twin row of r*
PAIR = (FIRST_FAR + 10, FIRST_FAR + 60)  # twin rows of r* + 10 and r* + 60: the second is a copy of the first


@functools.lru_cache(maxsize=None)
def real_positions(layout: Layout) -> np.ndarray:
    """the matrix row of every real sequence, ascending: twin row i is far row real_positions(layout)[i]"""
    r, h, n = layout.r_star, layout.h_star, layout.nrows
    pos = np.concatenate([np.arange(8), [h - 1, h, h + 1], np.arange(r - 2, r + 94), np.arange(n - 16, n)]).astype(np.int64)
    pos.setflags(write=False)
    return pos


@functools.lru_cache(maxsize=None)
def real_seqs(layout: Layout) -> tuple:
    """the real sequences in position order (the twin's input)"""
    rng = np.random.default_rng(layout.seed)
    out = []
    for _ in range(N_REAL):
        n = int(rng.integers(600, 1501))
        s = rng.choice(4, size=n, p=rng.dirichlet((3.0, 3.0, 3.0, 3.0))).astype(np.uint8)
        s[rng.integers(0, n, size=int(rng.integers(1, 4)))] = 4
        out.append(s)
    out[PAIR[1]] = out[PAIR[0]].copy()
    for s in out:
        s.setflags(write=False)
    return tuple(out)


def filler_length(layout: Layout, pos: int) -> int:
    """bases of the filler at row `pos` (a row that is not real): 0 far from the edges; near h*, from r* - NEAR on and
    so up to the end the mix by pos % 3 of length 0, length k - 1 (valid bases) and INVALID_RUN invalid symbols"""
    near = abs(pos - layout.h_star) <= NEAR or pos >= layout.r_star - NEAR
    return (0, layout.k - 1, INVALID_RUN)[pos % 3] if near else 0


@functools.lru_cache(maxsize=None)
def stream(layout: Layout):
    """(data uint8, offsets uint64 [N + 1]) of the whole layout, for Context.build_matrix_concat"""
    pos, seqs = real_positions(layout), real_seqs(layout)
    lengths = np.zeros(layout.nrows, dtype=np.int64)
    near = np.concatenate([np.arange(layout.h_star - NEAR, layout.h_star + NEAR + 1),
                           np.arange(layout.r_star - NEAR, layout.nrows)])
    lengths[near] = [filler_length(layout, int(p)) for p in near]
    lengths[pos] = [s.size for s in seqs]
    offsets = np.zeros(layout.nrows + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lengths)
    data = np.zeros(int(offsets[-1]) + 16, dtype=np.uint8)  # (valid bases 0 in the k - 1 fillers; a readable tail)
    for p in near:
        if lengths[p] == INVALID_RUN:  # (a real row is 600 bases or more)
            data[int(offsets[p]): int(offsets[p + 1])] = 4
    for p, s in zip(pos, seqs):
        data[int(offsets[p]): int(offsets[p + 1])] = s
    data.setflags(write=False)
    offsets.setflags(write=False)
    return data, offsets


def row_seq(layout: Layout, pos: int) -> np.ndarray:
    data, offsets = stream(layout)
    return data[int(offsets[pos]): int(offsets[pos + 1])]


def windows(layout: Layout):
    """(row0, nrows) of the read-back windows: around h*, around r* (the whole block and empty rows on both sides),
    the end"""
    r, h, n = layout.r_star, layout.h_star, layout.nrows
    return ((h - 4, 9), (r - 6, 104), (n - 20, 20))


@functools.lru_cache(maxsize=None)
def real_counts(layout: Layout) -> np.ndarray:
    """oracle.count_kmers of the real rows, uint32 [N_REAL, B]"""
    out = np.stack([oracle.count_kmers(s, 4, layout.k) for s in real_seqs(layout)]).astype(np.uint32)
    out.setflags(write=False)
    return out


def window_counts(layout: Layout, row0: int, nrows: int) -> np.ndarray:
    """oracle.count_kmers of rows row0 .. row0 + nrows - 1 of the layout, fillers included"""
    return np.stack([oracle.count_kmers(row_seq(layout, p), 4, layout.k) for p in range(row0, row0 + nrows)]).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def real_entropies(layout: Layout) -> np.ndarray:
    return np.array([oracle.to_kfreqs(s, 4, layout.k)[1] for s in real_seqs(layout)])


# ------------------------------------------------------------------------------------------- the selections
@functools.lru_cache(maxsize=None)
def oracle_nmost(layout: Layout):
    """(the oracle's nmost(40) over the real rows labelled by their positions, its accept count)"""
    return oracle.nmost_concat(*oracle.concat(real_seqs(layout)), N_SELECT, layout.k, 4, labels=real_positions(layout))


N_FRONT = 8  # real rows among the first N_SELECT positions of the stream: the seeds of a selection without an order


@functools.lru_cache(maxsize=None)
def oracle_nmost_whole(layout: Layout):
    """(the oracle's answer to nmost(N_SELECT) over the whole stream, its accept count): seeded by the real rows among
    the first N_SELECT positions, the N_FRONT front rows"""
    return oracle.nmost_concat(*oracle.concat(real_seqs(layout)), N_FRONT, layout.k, 4, labels=real_positions(layout))


@functools.lru_cache(maxsize=None)
def whole_stream_far_accepts(layout: Layout) -> int:
    """how many of the accepts of `oracle_nmost_whole` take a row at a position >= r* (select_nmost_divergent replayed
    step by step, src/records.rs:311-342): each of them replaces the set's lowest member by a far row, and the
    candidates behind it are scored against a set that holds it"""
    seqs, pos = real_seqs(layout), real_positions(layout)
    oset = oracle.SummedRecords.from_seqs(list(seqs[:N_FRONT]), layout.k, 4, labels=pos[:N_FRONT])
    far = 0
    for i in range(N_FRONT, N_REAL):
        f, h = oracle.to_kfreqs(seqs[i], 4, layout.k)
        if oset.increases_jsd(f, h, int(pos[i])):
            oset.replace_lowest(f, h, int(pos[i]))
            far += bool(pos[i] >= layout.r_star)
    assert oset.members()[0].tolist() == oracle_nmost_whole(layout)[0].members()[0].tolist()  # (the replay is the oracle's run)
    return far


@functools.lru_cache(maxsize=None)
def oracle_max(layout: Layout):
    lo, hi, stat = MAX_ARGS
    return oracle.max_divergent(list(real_seqs(layout)), lo, hi, layout.k, 4, stat, labels=real_positions(layout))


@functools.lru_cache(maxsize=None)
def oracle_nmost_by_order(layout: Layout):
    """the oracle's nmost(40) with its members named by their place in the order `real_positions`"""
    return oracle.nmost(list(real_seqs(layout)), N_SELECT, layout.k, 4)


TIE_N = 3


@functools.lru_cache(maxsize=None)
def tie_case(layout: Layout):
    """(order of matrix rows, the oracle's nmost(TIE_N) over it named by place in the order): the recipe of
    test_gpu_parity.test_degenerate_inputs_take_the_arbiter -- a duplicated row -- over far rows only.  The order
    starts with the first row of the pair and two far rows beside which it is the set's lowest member, then the
    pair's second row: a candidate that scores exactly the threshold, which no float tier may decide.  The rest of
    the far rows follow."""
    seqs, pos = real_seqs(layout), real_positions(layout)
    far = [i for i in range(FIRST_FAR, N_REAL) if i not in PAIR]
    for a in range(len(far)):
        for b in range(a + 1, len(far)):
            head = [PAIR[0], far[a], far[b]]
            if oracle.SummedRecords.from_seqs([seqs[i] for i in head], layout.k, 4).lowest_index == 0:
                twin_order = head + [PAIR[1]] + [i for i in far if i not in head]
                exp = oracle.nmost([seqs[i] for i in twin_order], TIE_N, layout.k, 4)
                return pos[twin_order].astype(np.uint32), exp
    raise AssertionError("no two far rows leave the pair's first row the lowest member")


# ------------------------------------------------------------------------------------------- the row lists
N_Q, N_R = 45, 107  # a ragged last 32-row tile on each side (32 + 13, 96 + 11)


@functools.lru_cache(maxsize=None)
def row_lists(layout: Layout):
    """(q, r) as twin rows, each in a shuffled order: q is two front rows, the three rows at h* and 40 far rows with
    the pair among them; r is q and 62 more far rows.  Far row = real_positions(layout)[twin row]."""
    rng = np.random.default_rng(layout.seed + 1)
    far = [i for i in range(FIRST_FAR, N_REAL) if i not in PAIR]
    far = [far[i] for i in rng.permutation(len(far))]
    q = [0, 5, 8, 9, 10, *PAIR] + far[:38]
    r = q + far[38:100]
    q, r = np.array(q)[rng.permutation(len(q))], np.array(r)[rng.permutation(len(r))]
    assert q.size == N_Q and r.size == N_R
    return q, r


@functools.lru_cache(maxsize=None)
def truth_cells(layout: Layout, mode: str) -> np.ndarray:
    """the long-double truth of every cell q x r (test_distance_truth_host.truth_jsd_rows / truth_euclid_rows).  The
    yardstick is handed each pair restricted to the bins either row fills: a bin empty in both adds an exact zero to
    every sum of either definition, and at 4^9 bins the rows fill under 1 % of them."""
    q, r = row_lists(layout)
    counts = real_counts(layout)
    filled = [np.flatnonzero(row) for row in counts]
    fn = truth_jsd_rows if mode == "jsd" else truth_euclid_rows
    out = np.zeros((q.size, r.size), dtype=np.longdouble)
    for a, i in enumerate(q):
        for b, j in enumerate(r):
            cols = np.union1d(filled[i], filled[j])
            out[a, b] = fn(np.stack([counts[i, cols], counts[j, cols]]), [(0, 1)])[0]
    out.setflags(write=False)
    return out


def square_of(cells: np.ndarray, layout: Layout) -> np.ndarray:
    """the q x q block of a q x r matrix (q is part of r)"""
    q, r = row_lists(layout)
    where = {int(j): b for b, j in enumerate(r)}
    return np.asarray(cells)[:, [where[int(i)] for i in q]]


# ------------------------------------------------------------------------------------------------ the tests
_ids = [x.name for x in LAYOUTS]


@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
def test_position_arithmetic(layout):
    B, r, h, n = layout.nbins, layout.r_star, layout.h_star, layout.nrows
    assert r * B == 1 << 32 and h * B == 1 << 31 and n == r + 293 and n * B > 1 << 32
    assert (r - 1) * B + B == 1 << 32  # row r* - 1 ends exactly at the boundary
    pos = real_positions(layout)
    assert pos.size == N_REAL == 123 and (np.diff(pos) > 0).all() and pos[-1] == n - 1
    assert int((pos * B >= 1 << 32).sum()) >= MIN_FAR_REAL
    assert pos[FIRST_FAR] == r and (pos[:FIRST_FAR] < r).all() and pos[PAIR[0]] == r + 10 and pos[PAIR[1]] == r + 60
    assert {h - 1, h, h + 1, r - 2, r - 1, r + 93, n - 16} <= set(pos.tolist()) and r + 94 not in pos and n - 17 not in pos
    assert (layout.name, r, layout.count_bytes) in {("u16-k6", 1_048_576, 2), ("u32-k7", 262_144, 4), ("u32-k9", 16_384, 4)}
    assert abs(layout.nbytes / {"u16-k6": 8.6e9, "u32-k7": 17.2e9, "u32-k9": 17.5e9}[layout.name] - 1) < 0.01
    assert (B > 16_384) == (layout.name == "u32-k9") and (layout.engine_nmost == 0) == (B > 16_384)  # wide rows: multi-launch only


@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
def test_stream_holds_the_real_rows_and_nothing_else_with_a_kmer(layout):
    data, offsets = stream(layout)
    pos, seqs = real_positions(layout), real_seqs(layout)
    assert offsets.size == layout.nrows + 1 and offsets.dtype == np.uint64 and data.dtype == np.uint8
    lengths = np.diff(offsets.astype(np.int64))
    for p, s in zip(pos, seqs):
        assert 600 <= s.size <= 1500 and 1 <= int((s == 4).sum()) <= 3 and np.array_equal(row_seq(layout, int(p)), s)
    fillers = np.ones(layout.nrows, dtype=bool)
    fillers[pos] = False
    assert set(np.unique(lengths[fillers]).tolist()) == {0, layout.k - 1, INVALID_RUN}
    assert int((lengths[fillers] > 0).sum()) < 300  # most fillers have length 0
    for p in np.flatnonzero(fillers & (lengths > 0)):
        assert oracle.count_kmers(row_seq(layout, int(p)), 4, layout.k).sum() == 0
    for row0, nrows in windows(layout):  # every window holds real rows and fillers of every kind
        inside = np.arange(row0, row0 + nrows)
        kinds = set(lengths[inside][fillers[inside]].tolist())
        assert (~fillers[inside]).any() and kinds == {0, layout.k - 1, INVALID_RUN}, (row0, kinds)
    assert (real_counts(layout).sum(axis=1) > 0).all()


@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
def test_no_two_real_rows_are_equal_but_the_pair(layout):
    seqs, counts = real_seqs(layout), real_counts(layout)
    assert np.array_equal(seqs[PAIR[0]], seqs[PAIR[1]])
    rest = [i for i in range(N_REAL) if i != PAIR[1]]
    assert len({seqs[i].tobytes() for i in rest}) == len(rest)
    assert len({counts[i].tobytes() for i in rest}) == len(rest)  # distinct as count rows too


@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
def test_oracle_nmost_accepts_and_ends_behind_the_boundary(layout):
    exp, acc = oracle_nmost(layout)
    members = exp.members()[0]
    far = int((members >= layout.r_star).sum())
    print(f"{layout.name}: nmost({N_SELECT}) {acc} accepts, {far} members at positions >= r*")
    assert exp.size == N_SELECT and acc >= MIN_ACCEPTS and far >= MIN_FAR_MEMBERS
    by_order = oracle_nmost_by_order(layout)
    assert real_positions(layout)[by_order.members()[0]].tolist() == members.tolist()


@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
def test_whole_stream_nmost_is_seeded_by_the_front_rows(layout):
    """the oracle over a stream with the layout's head -- 8 real rows, 32 rows without a valid k-mer (of the three
    kinds), then the other real rows -- gives nmost(40) the set, and the accept count, it gives nmost(8) over the real
    rows alone; at least one row beyond the seeds is accepted"""
    seqs, pos = real_seqs(layout), real_positions(layout)
    assert int((pos < N_SELECT).sum()) == N_FRONT and (pos[:N_FRONT] == np.arange(N_FRONT)).all()
    empties = [(np.zeros(0, np.uint8), np.zeros(layout.k - 1, np.uint8), np.full(INVALID_RUN, 4, np.uint8))[i % 3]
               for i in range(N_SELECT - N_FRONT)]
    head = list(seqs[:N_FRONT]) + empties + list(seqs[N_FRONT:])
    labels = np.concatenate([pos[:N_FRONT], np.full(len(empties), 0xFFFFFFF0, dtype=np.int64), pos[N_FRONT:]])
    got, got_acc = oracle.nmost_concat(*oracle.concat(head), N_SELECT, layout.k, 4, labels=labels)
    exp, acc = oracle_nmost_whole(layout)
    assert got.size == exp.size == N_FRONT and got_acc == acc
    assert got.members()[0].tolist() == exp.members()[0].tolist() and got.total_jsd == exp.total_jsd
    far_accepts, far_members = whole_stream_far_accepts(layout), int((exp.members()[0] >= layout.r_star).sum())
    print(f"{layout.name}: nmost({N_SELECT}) over the whole stream: a set of {exp.size}, {acc} accepts, {far_accepts} of "
          f"them of rows >= r*, {far_members} members >= r*: {exp.members()[0].tolist()}")
    # the set replaces its lowest member by rows behind r* and ends holding some: the engine fetches members from there
    assert far_accepts >= MIN_WHOLE_FAR and far_members >= MIN_WHOLE_FAR


@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
def test_oracle_max_keeps_pushes_and_ends_behind_the_boundary(layout):
    exp = oracle_max(layout)
    far = int((exp.members()[0] >= layout.r_star).sum())
    print(f"{layout.name}: max{MAX_ARGS} size {exp.size}, {far} members at positions >= r*")
    assert exp.size >= MAX_ARGS[0] + MIN_PUSHES and exp.size <= MAX_ARGS[1] and far >= MIN_FAR_MAX_MEMBERS


@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
def test_tie_case_presents_a_copy_of_the_lowest_member(layout):
    order, exp = tie_case(layout)
    pos = real_positions(layout)
    assert order.dtype == np.uint32 and (order >= layout.r_star).all() and len(set(order.tolist())) == order.size
    assert order[0] == pos[PAIR[0]] and order[TIE_N] == pos[PAIR[1]]
    head = oracle.SummedRecords.from_seqs([row_seq(layout, int(p)) for p in order[:TIE_N]], layout.k, 4)
    assert head.lowest_index == 0  # ... so the candidate behind the seeds is a copy of the lowest member
    assert exp.size == TIE_N


@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
def test_row_lists_and_their_truth(layout):
    q, r = row_lists(layout)
    pos = real_positions(layout)
    assert q.size % 32 and r.size % 32 and q.size > 32 and r.size > 96 and set(q.tolist()) <= set(r.tolist())
    assert len(set(q.tolist())) == q.size and len(set(r.tolist())) == r.size
    for rows in (q, r):
        p = pos[rows]
        assert int((p < 8).sum()) == 2 and int(((p >= layout.h_star - 1) & (p <= layout.h_star + 1)).sum()) == 3
        assert int((p >= layout.r_star).sum()) == rows.size - 5 and not (np.diff(p) > 0).all()
    assert set(PAIR) <= set(q.tolist())
    jsd = truth_cells(layout, "jsd")
    euc = truth_cells(layout, "euclidean")
    zero = np.array([[i == j or {int(i), int(j)} == set(PAIR) for j in r] for i in q])
    assert jsd.shape == euc.shape == (N_Q, N_R) and (jsd[~zero] > 0).all() and (euc[~zero] > 0).all()
    assert (np.abs(jsd[zero]) < 1e-17).all() and (euc[zero] == 0).all() and int(zero.sum()) == N_Q + 2
    # the restriction to the filled bins changes nothing: the dense yardstick on a few cells (k = 9: 4 MB a row)
    counts = real_counts(layout)
    for a, b in ((0, 0), (7, 3), (N_Q - 1, N_R - 1)):
        i, j = int(q[a]), int(r[b])
        dense = truth_jsd_rows(np.stack([counts[i], counts[j]]), [(0, 1)])[0]
        assert abs(dense - jsd[a, b]) <= 1e-15, (a, b)  # (two orders of a long-double sum; tol_derived(4096) is 1e-11)
    sq = square_of(jsd, layout)
    assert sq.shape == (N_Q, N_Q) and (np.abs(np.diag(sq)) < 1e-17).all() and np.abs(sq - sq.T).max() < 1e-17
