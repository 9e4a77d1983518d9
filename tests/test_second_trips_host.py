"""The second regimes of the distance-side kernels, without a GPU: the pinned cases of tests/test_gpu_second_trips.py, the
one new yardstick they need, and CPU tests that tie both to the yardsticks the project already has.

The suites of neighbour joining, cophenet and nearest choose their sizes around the wave (64), the workgroup (256) and the
32-row tile.  Each of these kernels also has a regime that begins at a larger size -- a loop takes its second trip, a row
no longer fits in LDS, a grid is capped and the rows are dealt out in passes -- and the constants below say where.  They
restate the kernels' own (csrc/nj.hip, csrc/cophenet.hip, csrc/nearest.hip, csrc/crossdist.hip, csrc/mash.hip); a case
asserts on the host that it lies beyond the one it is there for.

`restated_prefix(d, steps)` is test_nj_host.restated for the first `steps` records only: `_nj`'s algorithm and order of
operands in float64, but a retired slot stays where it is (its R is -inf, so every Q it takes part in is +inf) and nothing
is compacted -- `_nj` copies the whole matrix twice per step with np.delete, which at n = 8204 is most of a second.  Slots
stay in ascending order either way, so the first of equal Q values is the same pair, and the one sum that is taken afresh
(the new row's R) runs over the same elements in the same order: the records are `_nj`'s bit for bit, on any input."""
import functools

import numpy as np
import pytest

import oracle
from test_cophenet_host import KINDS
from test_nj_host import dyadic_tree, restated, split_lengths, tie_case, truth

# ---- where the second regimes begin
NJ_JOIN_TRIP = 4096      # nj_join_kernel's update loop: NJ_UNROLL x NJ_JOIN_THREADS list positions per trip
NJ_JOIN_CANDS = 1024     # ... and its candidate reduction's stride; a scan leaves min(2048, ceil(r / 4)) candidates
NJ_SCAN_PASS = 8192      # nj_scan_kernel: NJ_MAX_GRID workgroups x 4 waves; more active rows are dealt out in passes
COPH_CHUNK = 1024        # cophenet_kernel: positions of one side of the leaf order per chunk
TOPK_LDS = 2048          # cross_topk_kernel: the cells of a row staged in LDS at most
PAIR_ROW_LDS = 8192      # mash_pairs_kernel: the hashes of the shared row staged in LDS at most
CROSS_STRIP_BYTES = 256 << 20  # the strip buffer's bound; a strip is whole 32-row tile rows

# ---- neighbour joining
NJ_EXACT = ((4100, "random"), (8204, "random"), (8204, "caterpillar"))
NJ_DEVICE_TENSOR = (8204, "caterpillar")  # the one that also runs from a device tensor
PREFIX_KINDS = ("small-integer", "constant", "wide-integer", "far-tail", "far-tail-ties")
# (n, steps): r runs from 4104 to 4093 across the 4096 edge, from 8204 to 8189 across the 8192 edge
PREFIX_CASES = ((4104, 12), (8204, 16))


def tail_start(n: int) -> int:
    """the first slot of the far tail: the list positions beyond the edge n lies above (a scan's second pass, a join's
    second trip); the last twelve slots of a small matrix"""
    return NJ_SCAN_PASS if n > NJ_SCAN_PASS else NJ_JOIN_TRIP if n > NJ_JOIN_TRIP else n - 12


def prefix_case(kind: str, n: int) -> np.ndarray:
    """test_nj_host.tie_case, and three kinds of integers below 2^20.  "wide-integer": uniform, the least Q alone.
    "far-tail": the same, but the slots from tail_start(n) on lie far from every other slot (2^20 - 2^16 at least) and
    close to each other (below 64), so that step after step the least Q is a pair of THEM -- rows that only the second
    pass of a scan reads, list positions that only the second trip of a join's loop reaches.  (In the all-tie kinds the
    winner is always the lowest pair of slots and in "wide-integer" it is somewhere among 33 million pairs: neither
    notices a scan that leaves the last rows out.)  "far-tail-ties": the tail 3 apart from each other and 2^20 - 1 from
    the rest, so that the tie rule decides among pairs of the second pass.

    Exact over a prefix of T <= 16 steps whatever the order of summation: after t joins every entry is a multiple of
    2^-t below 2^21 in magnitude, a row sum lies below 2^34, (r - 2) D - R_i - R_j has at most 14 + 21 + 16 bits; only
    the division of the branch length rounds, alike wherever the operands are alike"""
    if kind not in ("wide-integer", "far-tail", "far-tail-ties"):
        return tie_case(kind, n)
    d = np.random.default_rng([3, n]).integers(0, 1 << 20, size=(n, n)).astype(np.float64)
    if kind != "wide-integer":
        t = tail_start(n)
        rng = np.random.default_rng([7, n])
        far = rng.integers((1 << 20) - (1 << 16), 1 << 20, size=(t, n - t)).astype(np.float64)
        near = rng.integers(0, 64, size=(n - t, n - t)).astype(np.float64)
        d[:t, t:] = far if kind == "far-tail" else float((1 << 20) - 1)
        d[t:, :t] = d[:t, t:].T
        d[t:, t:] = near if kind == "far-tail" else 3.0
    return d


def tail_joins(n: int, children) -> int:
    """how many of the leading records join two nodes of the far tail (its leaves, or nodes made of them)"""
    t, count = tail_start(n), 0
    for a, b, _ in np.asarray(children).tolist():
        if min(a, b) < t:
            break
        count += 1
    return count


def restated_prefix(d, steps: int):
    """-> (children int64 [steps, 3], lengths float64 [steps, 3]): the first `steps` records of restated(d)"""
    d = np.asarray(d, dtype=np.float64)
    n = d.shape[0]
    assert d.shape == (n, n) and 0 <= steps <= n - 3
    D = np.triu(d, 1)
    D = D + D.T
    tri = np.tri(n, dtype=bool)  # on and below the diagonal: never a candidate
    active = np.ones(n, dtype=bool)
    node = np.arange(n, dtype=np.int64)
    R = D.sum(axis=1)
    Q = np.empty_like(D)
    children = np.full((steps, 3), -1, dtype=np.int64)
    lengths = np.zeros((steps, 3))
    r = n
    for t in range(steps):
        rm2 = np.float64(r - 2)
        np.multiply(D, rm2, out=Q)  # (r - 2) D[i][j] - R[i] - R[j], left to right; +inf wherever a slot is retired
        Q -= R[:, None]
        Q -= R[None, :]
        np.putmask(Q, tri, np.inf)
        i, j = divmod(int(np.argmin(Q)), n)  # the first of equal values: the lowest (i, j)
        assert i < j and active[i] and active[j]
        dij = D[i, j]
        li = dij / 2.0 + (R[i] - R[j]) / (2.0 * rm2)
        children[t, 0], children[t, 1] = node[i], node[j]
        lengths[t, 0], lengths[t, 1] = li, dij - li
        di, dj = D[i].copy(), D[j].copy()
        du = (di + dj - dij) / 2.0
        R = R - di - dj + du  # (a retired slot's stays -inf)
        du[i] = 0
        D[i, :] = du
        D[:, i] = du
        active[j] = False
        R[j] = -np.inf
        node[i] = n + t
        R[i] = D[i][active].sum()  # the new row as `_nj` holds it: the active slots in ascending order
        r -= 1
    return children, lengths


@functools.lru_cache(maxsize=None)
def prefix_yardstick(kind: str, n: int, steps: int):
    """-> (d, the first `steps` children, lengths): computed once, shared, left unchanged"""
    d = prefix_case(kind, n)
    c, l = restated_prefix(d, steps)
    for a in (d, c, l):
        a.setflags(write=False)
    return d, c, l


@functools.lru_cache(maxsize=None)
def exact_case(n: int, shape: str):
    """-> (the generating tree's split map, its path lengths): computed once, shared, left unchanged"""
    tree, A = dyadic_tree(n, shape)
    A.setflags(write=False)
    return split_lengths(tree, n), A


# ---- cophenet
# (n, method): single, average and ward where a side has one item in its second chunk (1026) and where the middle leaves
# have two chunks on both sides (2100); average alone where a third chunk writes the buffer the first one used (3000)
COPH_CASES = [(n, method) for n in (1026, 2100) for method in ("single", "average", "ward")] + [(3000, "average")]
COPH_STRIP_SEQS = 1100   # the fused case: rows of k = 3 counts, more than one chunk on a side
COPH_DEFAULT_CUT = 6007  # the driver's own arithmetic cuts this walk in two


def chunks_per_side(n: int):
    """-> (the most chunks any side of any leaf has, the most that BOTH sides of one leaf have).  A leaf order holds
    every position p < n once, whatever the tree, and the leaf at p has n - 1 - p positions to its right and p to its
    left: the counts depend on n alone"""
    chunks = lambda count: -(-count // COPH_CHUNK)  # noqa: E731
    return (max(chunks(max(p, n - 1 - p)) for p in range(n)), max(chunks(min(p, n - 1 - p)) for p in range(n)))


def default_strip_rows(m: int, n: int) -> int:
    """the rows of a strip of an m x n walk where no knob is set: strip_rows of csrc/crossdist.hip"""
    return min(max(CROSS_STRIP_BYTES // (n * 8) // 32 * 32, 32), m)


def random_seqs(rng, count: int, lo: int = 100, hi: int = 1500):
    return [rng.integers(0, 4, size=int(rng.integers(lo, hi)), dtype=np.uint8) for _ in range(count)]


NO_KMER = np.full(40, 4, np.uint8)  # a sequence without a valid k-mer


# ---- nearest
NEAREST_K = 3
NEAREST_QUERIES = 33
NEAREST_REFS = (2048, 2049, 2050, 5000)
NEAREST_KK = (1, 3, 64)
TIE_QUERY = 5  # a copy of reference 2: its nearest are the copies of reference 2, at exactly 0


@functools.lru_cache(maxsize=None)
def nearest_case(n: int):
    """-> (queries, references).  Reference n - 1 and reference 2049 (where it exists) are copies of reference 2, in
    other threads' columns (a thread takes the columns tid, tid + 256, ...); reference 2060 (where it exists) and query 3
    have no valid k-mer; query 5 is reference 2 once more, so that the tie decides the head of a list for certain"""
    rng = np.random.default_rng([4, n])
    q, r = random_seqs(rng, NEAREST_QUERIES), random_seqs(rng, n)
    r[n - 1] = r[2].copy()
    if n > 2049:
        r[2049] = r[2].copy()
    if n > 2060:
        r[2060] = NO_KMER.copy()
    q[3] = NO_KMER.copy()
    q[TIE_QUERY] = r[2].copy()
    return q, r


def copies_of_reference_2(n: int):
    return sorted({2, n - 1} | ({2049} if n > 2049 else set()))


SPARSE_REFS, SPARSE_LIVE = 2100, 10


@functools.lru_cache(maxsize=None)
def sparse_case():
    """-> (queries, references, the ten references with a valid k-mer): fewer finite cells in a row than slots"""
    rng = np.random.default_rng(6)
    q = random_seqs(rng, NEAREST_QUERIES)
    live = np.sort(rng.choice(SPARSE_REFS, SPARSE_LIVE, replace=False))
    r = [NO_KMER.copy() for _ in range(SPARSE_REFS)]
    for j, s in zip(live, random_seqs(rng, SPARSE_LIVE)):
        r[j] = s
    return q, r, live


MASH_NEAREST = dict(k=10, sketch_size=50, n=2100)


@functools.lru_cache(maxsize=None)
def mash_nearest_case():
    """-> (queries, references): query 2 has an empty sketch (every cell of its row is 1.0: one tie over all 2100
    columns), reference n - 1 and 2049 are copies of reference 2 and query 5 is another"""
    rng = np.random.default_rng(8)
    n, k = MASH_NEAREST["n"], MASH_NEAREST["k"]
    q, r = random_seqs(rng, NEAREST_QUERIES, 200, 900), random_seqs(rng, n, 200, 900)
    q[2] = q[2][: k - 1]
    r[n - 1] = r[2].copy()
    r[2049] = r[2].copy()
    q[TIE_QUERY] = r[2].copy()
    return q, r


# ---- cross mash, sketches longer than the staged row
LONG_SKETCH = dict(k=12, sketch_size=9000)
LONG_SHORT_QUERY, LONG_SHORT_REFS, LONG_EMPTY_REF, LONG_RELATED = 3, (7, 40), 20, ((0, 10), (1, 11))


@functools.lru_cache(maxsize=None)
def long_sketch_case():
    """-> (5 queries, 70 references) of 12 000 to 14 000 random bases.  Query 3 and references 7 and 40 are cut to 6 000
    bases: their sketches are shorter than s, so a wave's pairs end at different steps.  Reference 20 has no valid k-mer.
    Two random sequences of this length share a handful of 12-mers, which would leave every intersection at a few
    hashes; references 10 and 11 are queries 0 and 1 with 2 % of their bases replaced, so that some intersections run to
    thousands"""
    rng = np.random.default_rng(9)
    q, r = random_seqs(rng, 5, 12_000, 14_001), random_seqs(rng, 70, 12_000, 14_001)
    for qi, rj in LONG_RELATED:
        s = q[qi].copy()
        at = rng.random(s.size) < 0.02
        s[at] = (s[at] + rng.integers(1, 4, size=int(at.sum()), dtype=np.uint8)) % 4
        r[rj] = s
    q[LONG_SHORT_QUERY] = q[LONG_SHORT_QUERY][:6000]
    for j in LONG_SHORT_REFS:
        r[j] = r[j][:6000]
    r[LONG_EMPTY_REF] = np.full(13_000, 4, np.uint8)
    return q, r


@functools.lru_cache(maxsize=None)
def long_sketch_oracle():
    """-> (the oracle's sketches of the queries, of the references, its distance of every pair)"""
    q, r = long_sketch_case()
    k, s = LONG_SKETCH["k"], LONG_SKETCH["sketch_size"]
    oq, orr = [oracle.mash_sketch(x, k, s, 4, False) for x in q], [oracle.mash_sketch(x, k, s, 4, False) for x in r]
    return oq, orr, np.array([[oracle.mash_distance(a, b, k, s) for b in orr] for a in oq])


# ------------------------------------------------------------------ restated_prefix is restated
@pytest.mark.parametrize("kind", ["small-integer", "constant", "zero", "wide-integer", "far-tail", "far-tail-ties"])
@pytest.mark.parametrize("n", [64, 300])
def test_restated_prefix_is_the_head_of_restated(n, kind):
    d = prefix_case(kind, n)
    before = d.copy()
    want = restated(d)
    for steps in (0, 1, 16, n - 3):
        c, l = restated_prefix(d, steps)
        assert c.shape == l.shape == (steps, 3) and c.dtype == np.int64 and l.dtype == np.float64
        assert np.array_equal(c, want.children[:steps])
        assert np.array_equal(l.view(np.uint64), want.lengths[:steps].view(np.uint64))
    assert np.array_equal(d, before)


def test_restated_prefix_is_the_head_of_restated_on_inexact_input():
    """the same bits where every operation rounds: the two run the same operations on the same operands"""
    for n in (5, 64, 257):
        d = np.random.default_rng([5, n]).random((n, n))
        want = restated(d)
        c, l = restated_prefix(d, n - 3)
        assert np.array_equal(c, want.children[: n - 3])
        assert np.array_equal(l.view(np.uint64), want.lengths[: n - 3].view(np.uint64))


def test_the_prefix_kinds_are_what_they_are_said_to_be():
    assert set(PREFIX_KINDS) == {"small-integer", "constant", "wide-integer", "far-tail", "far-tail-ties"}
    for n in (64, 300):
        d = prefix_case("wide-integer", n)
        assert d.dtype == np.float64 and (d == np.floor(d)).all() and d.min() >= 0 and d.max() < 2.0 ** 20
        assert truth(d)[2] > 0  # the least Q is alone at every step: the minimum itself is held, not the tie rule
        assert np.array_equal(prefix_case("small-integer", n), tie_case("small-integer", n))
        assert np.unique(prefix_case("constant", n)).tolist() == [2.5]
    # the records of the all-tie kinds are the lowest pair of slots, step after step
    c, _ = restated_prefix(prefix_case("constant", 64), 3)
    assert c[:, :2].tolist() == [[0, 1], [64, 2], [65, 3]]
    # those of the far-tail kinds are pairs of the tail until one node is left of it
    assert (tail_start(64), tail_start(300), tail_start(4104), tail_start(8204)) == (52, 288, NJ_JOIN_TRIP, NJ_SCAN_PASS)
    for n in (64, 300):
        t = tail_start(n)
        for kind in ("far-tail", "far-tail-ties"):
            d = prefix_case(kind, n)
            assert np.array_equal(d[:t, :t], prefix_case("wide-integer", n)[:t, :t]) and np.array_equal(d[t:, :t], d[:t, t:].T)
            assert (d == np.floor(d)).all() and d.min() >= 0 and d.max() < 2.0 ** 20 and d[:t, t:].min() >= 2.0 ** 20 - 2.0 ** 16
            c, _ = restated_prefix(d, 16)
            assert tail_joins(n, c) == n - t - 1
        assert c[0, :2].tolist() == [t, t + 1]  # all of the tail ties: its lowest pair of slots
        assert tail_joins(n, restated_prefix(prefix_case("wide-integer", n), 16)[0]) == 0


def test_the_nj_cases_lie_beyond_their_thresholds():
    for n, steps in PREFIX_CASES:
        edge = NJ_JOIN_TRIP if n < NJ_SCAN_PASS else NJ_SCAN_PASS
        assert n > edge and n - steps + 1 <= edge  # r runs n .. n - steps + 1: across the edge
        assert steps <= 16 and n - tail_start(n) - 1 < steps  # the whole tail is joined within the prefix
    assert min(n for n, _ in NJ_EXACT) > NJ_JOIN_TRIP and min(4100 // 4, 2048) > NJ_JOIN_CANDS
    assert sum(n > NJ_SCAN_PASS for n, _ in NJ_EXACT) == 2 and NJ_DEVICE_TENSOR in NJ_EXACT


# ------------------------------------------------------------------ the other cases
def test_the_cophenet_cases_lie_beyond_their_thresholds():
    assert chunks_per_side(300) == (1, 1) and chunks_per_side(1025) == (1, 1)  # what the older files reach
    assert chunks_per_side(1026) == (2, 1)
    assert chunks_per_side(2100) == (3, 2)
    assert chunks_per_side(3000) == (3, 2) and 3000 - 1 > 2 * COPH_CHUNK
    assert chunks_per_side(COPH_STRIP_SEQS)[0] == 2
    assert {n for n, _ in COPH_CASES} == {1026, 2100, 3000} and set(KINDS) == {"random", "tied", "caterpillar", "saturated"}
    # a square walk is cut by the driver's own arithmetic above 5 792 rows
    assert default_strip_rows(5792, 5792) == 5792 and default_strip_rows(5793, 5793) == 5792
    rows = default_strip_rows(COPH_DEFAULT_CUT, COPH_DEFAULT_CUT)
    assert rows % 32 == 0 and rows < COPH_DEFAULT_CUT <= 2 * rows
    assert default_strip_rows(3000, 3000) == 3000 and default_strip_rows(33, 5000) == 33


def test_the_nearest_cases_are_what_they_are_said_to_be():
    k = NEAREST_K
    valid = lambda s: oracle.count_kmers(s, 4, k).sum() > 0  # noqa: E731
    for n in NEAREST_REFS:
        q, r = nearest_case(n)
        assert len(q) == NEAREST_QUERIES and len(r) == n and n >= TOPK_LDS
        copies = copies_of_reference_2(n)
        assert len(copies) == (3 if n > 2050 else 2) and len({c % 256 for c in copies}) == len(copies)
        for c in copies:
            assert np.array_equal(r[c], r[2])
        assert np.array_equal(q[TIE_QUERY], r[2])
        assert not valid(q[3]) and sum(not valid(s) for s in q) == 1
        assert [j for j, s in enumerate(r) if not valid(s)] == ([2060] if n > 2060 else [])
    assert sorted(n > TOPK_LDS for n in NEAREST_REFS) == [False, True, True, True]  # the edge itself, and beyond
    q, r, live = sparse_case()
    assert len(r) == SPARSE_REFS > TOPK_LDS and live.size == SPARSE_LIVE < max(NEAREST_KK)
    assert [j for j, s in enumerate(r) if valid(s)] == live.tolist() and all(valid(s) for s in q)


def test_the_mash_cases_are_what_they_are_said_to_be():
    k, s, n = MASH_NEAREST["k"], MASH_NEAREST["sketch_size"], MASH_NEAREST["n"]
    q, r = mash_nearest_case()
    assert len(r) == n > TOPK_LDS and len(q) == NEAREST_QUERIES
    assert oracle.mash_sketch(q[2], k, s, 4, False).size == 0
    assert all(oracle.mash_sketch(x, k, s, 4, False).size == s for x in r)  # (no two empty sketches meet)
    # the long sketches
    q, r = long_sketch_case()
    k, s = LONG_SKETCH["k"], LONG_SKETCH["sketch_size"]
    assert len(q) == 5 and len(r) == 70 and s > PAIR_ROW_LDS
    oq, orr, exp = long_sketch_oracle()
    for i, sk in enumerate(oq):
        assert (sk.size == s) == (i != LONG_SHORT_QUERY) and 0 < sk.size <= s
    for j, sk in enumerate(orr):
        assert (sk.size == s) == (j not in LONG_SHORT_REFS + (LONG_EMPTY_REF,))
    assert orr[LONG_EMPTY_REF].size == 0 and 5000 < oq[LONG_SHORT_QUERY].size < PAIR_ROW_LDS
    assert (exp[:, LONG_EMPTY_REF] == 1.0).all() and not np.isnan(exp).any()
    for qi, rj in LONG_RELATED:  # thousands of common hashes
        assert 0 < exp[qi, rj] < 0.05
    far = np.delete(exp, [LONG_EMPTY_REF] + [rj for _, rj in LONG_RELATED], axis=1)
    assert np.unique(far).size > 3  # the unrelated pairs: several distinct small intersections
