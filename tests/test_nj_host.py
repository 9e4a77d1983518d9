"""Neighbour joining without a GPU: the yardsticks the GPU tests (test_gpu_nj.py) measure the device tree against, their
own preconditions, and the host-only parts of the feature (`cluster.nj_to_newick`, `cluster.patristic`, the argument
checks, the C boundary).

The yardsticks:
  * `restated(d)`: the algorithm of include/dvs_hip.h "neighbour-joining tree" in numpy float64 -- the same slot
    policy (the new node takes slot i, slot j is retired), the same tie rule (the lowest (i, j) in lexicographic slot
    order among equal Q) and the same order of operands;
  * `truth(d)`: the same in np.longdouble, which also reports the least relative gap between the best and the second
    best Q over the steps with r > 4;
  * `split_lengths(tree, n)`: the unrooted tree as {the smaller side of a split: its branch length}.  This is the only
    form in which two results on general input are compared: at r = 4 the two complementary pairs have exactly equal Q
    in real arithmetic (Q(ab) = -(d_ac + d_ad + d_bc + d_bd) = Q(cd)), rounding decides between them, the records
    differ and the unrooted tree does not.
Bit for bit (`children` and `lengths` with array_equal) is asked only where every decision and every length is exact:
the small-integer, constant and all-zero matrices.

The sequence families of the fused entries (test_gpu_linkage.family_seqs) hold exact duplicates: zero distances, Q ties
between several equally good cherries, and internal edges of length zero whose arrangement rounding decides.  Their
mash distances are not exact, so the bit-for-bit check does not apply; the choice made here is `same_tree(...,
merge_zero=True)`: the split maps are compared after merging zero-length edges -- an edge no longer than the length
tolerance may be missing from the other tree, every longer edge must be there."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from diverseseq_amd import _lib, apps, cluster, distance

EPS = 2.0 ** -52
SIZES_GENERAL = (5, 6, 64, 257, 600)  # the sizes of the GPU test's general cases
KINDS_GENERAL = ("noisy0.1", "noisy0.01", "uniform")


# ---- the yardsticks

def _nj(d, dtype, want_gap: bool):
    """the pinned algorithm in `dtype` -> (children int64 [n - 2, 3], lengths [n - 2, 3], least relative Q gap)"""
    d = np.asarray(d, dtype=np.float64)
    n = d.shape[0]
    assert d.shape == (n, n) and n >= 3
    D = np.triu(d, 1).astype(dtype)
    D = D + D.T  # compact: the active slots only, in ascending slot order
    scale = dtype(np.abs(D).max())
    node = list(range(n))
    R = D.sum(axis=1)
    tri = np.tri(n, dtype=bool)  # on and below the diagonal: never a candidate
    children = np.full((n - 2, 3), -1, dtype=np.int64)
    lengths = np.zeros((n - 2, 3), dtype=dtype)
    two = dtype(2)
    gap = np.inf
    r, t = n, 0
    while r > 3:
        rm2 = dtype(float(r - 2))
        Q = rm2 * D  # (r - 2) D[i][j] - R[i] - R[j], left to right
        Q -= R[:, None]
        Q -= R[None, :]
        np.putmask(Q, tri[:r, :r], np.inf)
        flat = Q.reshape(-1)
        best = int(np.argmin(flat))  # the first of equal values: the lowest (i, j)
        i, j = divmod(best, r)
        if want_gap and r > 4:
            q1 = flat[best]
            flat[best] = np.inf
            q2 = flat.min()
            gap = min(gap, float((q2 - q1) / max(abs(q1), rm2 * scale))) if scale > 0 else 0.0
        dij = D[i, j]
        li = dij / two + (R[i] - R[j]) / (two * rm2)
        children[t, 0], children[t, 1] = node[i], node[j]
        lengths[t, 0], lengths[t, 1] = li, dij - li
        di, dj = D[i].copy(), D[j].copy()
        du = (di + dj - dij) / two
        R = R - di - dj + du
        du[i] = 0
        D[i, :] = du
        D[:, i] = du
        D = np.delete(np.delete(D, j, axis=0), j, axis=1)
        R = np.delete(R, j)
        node[i] = n + t
        del node[j]
        pi = i  # (i < j: its position is unchanged)
        R[pi] = D[pi].sum()
        r -= 1
        t += 1
    dxy, dxz, dyz = D[0, 1], D[0, 2], D[1, 2]
    children[t] = node
    lengths[t] = [(dxy + dxz - dyz) / two, (dxy + dyz - dxz) / two, (dxz + dyz - dxy) / two]
    return children, lengths, gap


def restated(d):
    """-> distance.NJTree, float64"""
    c, l, _ = _nj(d, np.float64, False)
    return distance.NJTree(c, l)


def truth(d):
    """-> (children, lengths longdouble, the least relative gap between the best and second-best Q over r > 4)"""
    return _nj(d, np.longdouble, True)


def split_lengths(tree, n: int) -> dict:
    """the unrooted tree as {smaller side of the split (a bit mask of leaves; of two equal sides the one without leaf
    0): branch length}"""
    children, lengths = np.asarray(tree[0]), np.asarray(tree[1])
    assert children.shape == (n - 2, 3) and lengths.shape == (n - 2, 3)
    full = (1 << n) - 1
    mask = [1 << i for i in range(n)] + [0] * (n - 2)
    out = {}
    for t in range(n - 2):
        for c in range(3):
            v = int(children[t, c])
            if v < 0:
                assert c == 2 and t < n - 3
                continue
            assert v < n + t
            m = mask[v]
            mask[n + t] |= m
            other = full ^ m
            a, b = m.bit_count(), other.bit_count()
            key = m if (a < b or (a == b and not m & 1)) else other
            assert key not in out, "a split twice"
            out[key] = out.get(key, 0) + lengths[t, c]
    assert mask[2 * n - 3] == full
    return out


def same_tree(got: dict, want: dict, tol: float, merge_zero: bool = False) -> float:
    """asserts that two split maps are one tree: the same splits (merge_zero: but for edges no longer than tol), each
    length within tol; -> the worst length difference"""
    worst = 0.0
    for key in set(got) | set(want):
        if key in got and key in want:
            diff = abs(float(got[key] - want[key]))
        else:
            assert merge_zero, f"split {key:#x} is in one tree only"
            diff = abs(float(got.get(key, want.get(key))))
        worst = max(worst, diff)
        assert diff <= tol, (hex(key), diff, tol)
    return worst


# ---- the case generators (seeded)

def dyadic_tree(n: int, shape: str, seed: int = 0):
    """a tree of n leaves with branch lengths integers(1, 1025) / 1024 -> (distance.NJTree, its path lengths float64
    [n, n], exact).  shape: "random" joins two random subtrees at a time, "caterpillar" a leaf to the one growing
    subtree, "balanced" neighbours in rounds; the leaves are numbered at random."""
    rng = np.random.default_rng([seed, n, {"random": 0, "caterpillar": 1, "balanced": 2}[shape]])
    blen = lambda: float(rng.integers(1, 1025)) / 1024.0
    perm = rng.permutation(n)
    # a subtree: (node id, its leaves, their distances to its root)
    subs = [(int(perm[i]), np.array([perm[i]]), np.zeros(1)) for i in range(n)]
    A = np.zeros((n, n))
    children = np.full((n - 2, 3), -1, dtype=np.int64)
    lengths = np.zeros((n - 2, 3))

    def link(x, y, lx, ly):
        A[np.ix_(x[1], y[1])] = (x[2] + lx)[:, None] + (y[2] + ly)[None, :]
        A[np.ix_(y[1], x[1])] = A[np.ix_(x[1], y[1])].T

    t = 0
    while len(subs) > 3:
        if shape == "random":
            a, b = sorted(rng.choice(len(subs), 2, replace=False).tolist())
        elif shape == "caterpillar":
            a, b = 0, 1
        else:
            a, b = 0, 1  # (the joined subtree goes to the back: rounds)
        y, x = subs.pop(b), subs.pop(a)
        lx, ly = blen(), blen()
        link(x, y, lx, ly)
        children[t, :2] = x[0], y[0]
        lengths[t, :2] = lx, ly
        new = (n + t, np.concatenate([x[1], y[1]]), np.concatenate([x[2] + lx, y[2] + ly]))
        if shape == "caterpillar":
            subs.insert(0, new)
        else:
            subs.append(new)
        t += 1
    ls = [blen(), blen(), blen()]
    for a in range(3):
        for b in range(a + 1, 3):
            link(subs[a], subs[b], ls[a], ls[b])
    children[t] = [s[0] for s in subs]
    lengths[t] = ls
    return distance.NJTree(children, lengths), A


def general_case(kind: str, n: int) -> np.ndarray:
    """the pinned general cases: default_rng(0) streams per (kind, n)"""
    rng = np.random.default_rng([0, n, KINDS_GENERAL.index(kind)])
    if kind == "uniform":
        return rng.random((n, n))
    _, A = dyadic_tree(n, "random", seed=1)
    return A * (1.0 + (0.1 if kind == "noisy0.1" else 0.01) * rng.random((n, n)))


def tie_case(kind: str, n: int) -> np.ndarray:
    rng = np.random.default_rng([2, n])
    if kind == "small-integer":
        return rng.integers(0, 4, size=(n, n)).astype(np.float64)
    return np.full((n, n), 2.5 if kind == "constant" else 0.0)


@functools.lru_cache(maxsize=None)
def general_yardstick(kind: str, n: int):
    """-> (d, truth's split map, the least Q gap, restated's worst length error against truth)"""
    d = general_case(kind, n)
    tc, tl, gap = truth(d)
    want = split_lengths((tc, tl), n)
    got = split_lengths(restated(d), n)
    assert set(got) == set(want)
    err = max(abs(float(got[k] - want[k])) for k in want)
    return d, want, gap, err


def length_tolerance(n: int, d: np.ndarray, restated_err: float) -> float:
    """what a device length may differ from truth's: 4 x the restatement's own worst error on the case (the margin
    test_gpu_distance_truth.py gives its kernels), floored where the restatement happens to be exact"""
    return max(4.0 * restated_err, (n + 8) * EPS * float(np.abs(np.triu(d, 1)).max()))


# ---- Newick with branch lengths, read back

def parse_newick(text: str):
    """-> nested (children or leaf name, length or None)"""
    text = text.strip()
    assert text.endswith(";")
    text = text[:-1]
    pos = 0

    def length():
        nonlocal pos
        if pos < len(text) and text[pos] == ":":
            start = pos = pos + 1
            while pos < len(text) and text[pos] not in ",()":
                pos += 1
            return float(text[start:pos])
        return None

    def node():
        nonlocal pos
        while text[pos] == " ":
            pos += 1
        if text[pos] == "(":
            pos += 1
            kids = [node()]
            while text[pos] == ",":
                pos += 1
                kids.append(node())
            assert text[pos] == ")"
            pos += 1
            return tuple(kids), length()
        start = pos
        while pos < len(text) and text[pos] not in ",():":
            pos += 1
        return text[start:pos].strip(), length()

    out = node()
    assert pos == len(text)
    return out


def newick_splits(text: str, names) -> dict:
    """the split map (as split_lengths keys it) of a Newick string whose top level has three children"""
    index = {str(nm): i for i, nm in enumerate(names)}
    n = len(names)
    full = (1 << n) - 1
    out = {}

    def walk(item, top=False):
        body, length = item
        if isinstance(body, str):
            m = 1 << index[body]
        else:
            m = 0
            for kid in body:
                m |= walk(kid)
        if not top:
            other = full ^ m
            a, b = m.bit_count(), other.bit_count()
            key = m if (a < b or (a == b and not m & 1)) else other
            out[key] = out.get(key, 0) + (length if length is not None else 0.0)
        return m

    tree = parse_newick(text)
    assert len(tree[0]) == 3 and tree[1] is None
    assert walk(tree, top=True) == full
    return out


# ---- the yardsticks' own preconditions

@pytest.mark.parametrize("shape", ["random", "caterpillar", "balanced"])
@pytest.mark.parametrize("n", [3, 4, 5, 64, 257])
def test_restated_recovers_dyadic_additive_trees_exactly(n, shape):
    tree, A = dyadic_tree(n, shape)
    assert (A == A.T).all() and (np.diag(A) == 0).all() and (A[~np.eye(n, dtype=bool)] > 0).all()
    got = restated(A)
    assert split_lengths(got, n) == split_lengths(tree, n)  # == on the floats
    p = cluster.patristic(got)
    assert np.array_equal(p, A)
    assert np.array_equal(cluster.patristic(tree), A)


@pytest.mark.parametrize("kind", KINDS_GENERAL)
@pytest.mark.parametrize("n", SIZES_GENERAL)
def test_general_cases_are_well_separated(n, kind):
    """every general case of the GPU test: the least relative gap between the best and second-best Q (r > 4, by truth)
    is 2^16 n 2^-52 at least -- no case left out -- so the f64 decisions are truth's"""
    d, want, gap, err = general_yardstick(kind, n)
    print(f"n={n} {kind}: least Q gap {gap:.3g} (bar {2.0 ** 16 * n * EPS:.3g}); restated's worst length error "
          f"{err / (n * EPS * np.abs(d).max()):.3g} n eps max|D|")
    if n > 4:
        assert gap >= 2.0 ** 16 * n * EPS
    assert len(want) == 2 * n - 3


def test_f64_and_long_double_differ_in_records_not_in_the_tree():
    differ = 0
    for n in (5, 6, 17, 64):
        d = general_case("noisy0.1", n)
        a = restated(d)
        tc, tl, _ = truth(d)
        differ += not np.array_equal(a.children, tc)
        assert set(split_lengths(a, n)) == set(split_lengths((tc, tl), n))
    print("cases whose records differ between f64 and long double:", differ)


@pytest.mark.parametrize("kind", ["small-integer", "constant", "zero"])
def test_tie_cases_are_exact(kind):
    """the heavy-tie matrices: every Q and every matrix update is exact (integers and halves), so f64 and long double
    decide alike, record for record; a length is then one pinned sequence of correctly rounded f64 operations on exact
    operands (its division by 2 (r - 2) rounds, so long double's length differs in the last bits)"""
    for n in (3, 4, 5, 7, 64):
        d = tie_case(kind, n)
        a = restated(d)
        tc, tl, _ = truth(d)
        assert np.array_equal(a.children, tc)
        assert np.abs(a.lengths - tl).max() <= 4 * EPS * max(1.0, float(d.max()))


# ---- nj_to_newick and patristic

def test_newick_round_trip():
    for n, shape in ((3, "random"), (4, "random"), (9, "caterpillar"), (64, "random"), (65, "balanced")):
        tree, A = dyadic_tree(n, shape)
        names = [f"s{i}" for i in range(n)]
        text = cluster.nj_to_newick(names, tree)
        assert text.endswith(");") and text.count("(") == n - 2 and text.count(":") == 2 * n - 3
        assert newick_splits(text, names) == split_lengths(tree, n)
        bare = cluster.nj_to_newick(names, tree, lengths=False)
        assert ":" not in bare and set(newick_splits(bare, names)) == set(split_lengths(tree, n))
    tree = distance.NJTree(np.array([[0, 1, -1], [2, 3, 4]]), np.array([[0.1, 0.2, 0.0], [0.3, 0.4, 0.5]]))
    assert cluster.nj_to_newick("cdab", tree) == "(a:0.3, b:0.4, (c:0.1, d:0.2):0.5);"
    assert cluster.nj_to_newick("cdab", tree, lengths=False) == "(a, b, (c, d));"
    # lengths that need all 17 digits, negative ones, and a caterpillar deeper than the recursion limit
    rng = np.random.default_rng(5)
    for n, shape in ((200, "random"), (3000, "caterpillar")):
        tree, _ = dyadic_tree(n, shape)
        odd = distance.NJTree(tree.children, rng.normal(size=tree.lengths.shape) * (tree.children >= 0))
        text = cluster.nj_to_newick(list(range(n)), odd)
        if n == 200:
            assert newick_splits(text, list(range(n))) == split_lengths(odd, n)
        else:  # (this file's parser recurses; the writer must not)
            read = sorted(float(x) for x in re.findall(r":([^,()]+)", text))
            assert read == sorted(odd.lengths[odd.children >= 0].tolist()) and text.count("(") == n - 2
    with pytest.raises(ValueError):
        cluster.nj_to_newick(["a", "b"], tree)
    with pytest.raises(ValueError):
        cluster.nj_to_newick("abc", (np.zeros((1, 2), dtype=np.int64), np.zeros((1, 2))))


def test_patristic():
    tree = distance.NJTree(np.array([[0, 1, -1], [2, 3, 4]]), np.array([[0.125, 0.25, 0.0], [0.5, 1.0, 2.0]]))
    want = np.array([[0, 0.375, 2.625, 3.125], [0.375, 0, 2.75, 3.25], [2.625, 2.75, 0, 1.5], [3.125, 3.25, 1.5, 0]])
    assert np.array_equal(cluster.patristic(tree), want)
    for n, shape in ((3, "random"), (33, "caterpillar"), (300, "random"), (1025, "balanced")):
        tree, A = dyadic_tree(n, shape, seed=3)
        assert np.array_equal(cluster.patristic(tree), A)
    bad = [
        (np.array([[0, 0, -1], [1, 2, 4]]), "twice"),
        (np.array([[0, 5, -1], [1, 2, 4]]), "a node of the future"),
        (np.array([[0, 1, 2], [3, 4, -1]]), "a third child too early"),
        (np.array([[0, 1, -1], [2, 3, -1]]), "no third child in the last record"),
    ]
    for kids, why in bad:
        with pytest.raises(ValueError):
            cluster.patristic((kids, np.zeros(kids.shape)))
    with pytest.raises(ValueError):
        cluster.patristic((np.zeros((2, 2), dtype=np.int64), np.zeros((2, 2))))
    with pytest.raises(ValueError):
        cluster.patristic((np.array([[0, 1, 2]]), np.zeros((1, 2))))


# ---- argument errors, before any device work (none of these needs a GPU)

def test_argument_errors_need_no_device():
    with pytest.raises(ValueError, match="minimum of 3"):
        cluster.neighbor_joining(np.ones((2, 2)))
    with pytest.raises(ValueError, match="square"):
        cluster.neighbor_joining(np.ones((4, 5)))
    with pytest.raises(ValueError, match="square"):
        cluster.neighbor_joining(np.ones(9))
    seqs = {f"s{i}": np.zeros(30, dtype=np.uint8) for i in range(4)}
    with pytest.raises(ValueError, match="Unexpected distance"):
        cluster.nj_tree(seqs, distance_mode="blah")
    with pytest.raises(ValueError, match="Expected sketch size"):
        cluster.nj_tree(seqs, sketch_size=None)
    with pytest.raises(ValueError, match="Sketch size should only"):
        cluster.nj_tree(seqs, distance_mode="jsd")
    with pytest.raises(ValueError, match="Canonical kmers should only"):
        cluster.nj_tree(seqs, distance_mode="euclidean", sketch_size=None, mash_canonical_kmers=True)
    with pytest.raises(ValueError, match="three sequences"):
        cluster.nj_tree({k: seqs[k] for k in ("s0", "s1")})
    for fn in distance.NJ_MODES.values():
        with pytest.raises(ValueError, match="three sequences"):
            fn([seqs["s0"], seqs["s1"]], 4, 4)
    with pytest.raises(ValueError, match="Unexpected distance"):
        apps.dvs_njtree(distance_mode="blah")
    with pytest.raises(ValueError, match="Expected sketch size"):
        apps.dvs_njtree(sketch_size=None)
    with pytest.raises(ValueError, match="Canonical kmers only"):
        apps.dvs_njtree(moltype="protein", mash_canonical_kmers=True)
    a = apps.dvs_njtree(distance_mode="jsd", k=5)
    assert (a._k, a._sketch_size, a._distance_mode) == (5, None, "jsd") and "dvs_njtree" in apps.__all__
    assert set(distance.NJ_MODES) == set(distance.MODES)
    # neighbour joining is not a linkage method
    assert "nj" not in distance.LINKAGE_METHODS and list(distance.LINKAGE_METHODS) == ["single", "complete", "average",
                                                                                       "weighted", "ward"]


def test_c_boundary_without_a_device():
    L = _lib.load()
    assert L.dvs_abi_version() == 5
    names = ("dvs_nj", "dvs_nj_patristic")  # one entry for the tree: the mode, or the caller's matrix, travels in the dvs_source
    lib = C.CDLL(str(_lib.LIB_PATH))
    for name in names:
        assert name in _lib.EXPORTS and hasattr(lib, name)
    joins = np.array([0, 1, 2], dtype=np.uint32)
    lens = np.array([1.0, 2.0, 4.0])
    out = np.zeros((3, 3))
    u32, f64 = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    assert L.dvs_nj_patristic(None, 3, joins.ctypes.data_as(u32), lens.ctypes.data_as(f64), out.ctypes.data_as(f64)) == _lib.OK
    assert out.tolist() == [[0, 3, 5], [3, 0, 6], [5, 6, 0]]
    assert L.dvs_nj_patristic(None, 2, joins.ctypes.data_as(u32), lens.ctypes.data_as(f64), out.ctypes.data_as(f64)) == _lib.ERR_VALUE
    assert L.dvs_nj_patristic(None, 3, None, lens.ctypes.data_as(f64), out.ctypes.data_as(f64)) == _lib.ERR_VALUE
    # a null context is refused before anything else
    given = distance.make_source(_lib.SRC_GIVEN, out.ctypes.data, 3, keep=out)
    assert L.dvs_nj(None, given, joins.ctypes.data_as(u32), lens.ctypes.data_as(f64)) == _lib.ERR_VALUE
