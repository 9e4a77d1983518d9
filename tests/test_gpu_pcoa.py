"""Principal coordinates on the GPU (csrc/pcoa.hip, the projection kernel included) against the yardstick
and the cases of test_pcoa_host.py.

The bounds.  unit(n) = (n + 8) 2^-52 ||A||_F, A = -1/2 D o D: the rounding of one f64 pass over A.  The Frobenius norm,
because the error of a row's dot product sum_j a_ij x_j is bounded by n eps ||a_i||_2 ||x||_2, and over the rows these add
up to n eps ||A||_F ||x||_2; the spectral norm is smaller (||A||_2 <= ||A||_F), so a bound in it would be tighter than can
be derived entry by entry.
  - every reported residual equals the one numpy computes from the host's B for the returned pair, within unit(n);
  - `converged` implies residual <= tol * lambda_1;
  - |V^T V - I| <= (n + 8) 2^-52 per entry times the basis size (a derived bound: the observed figure is printed in
    units of it);
  - |lambda^_a - lambda_a| <= the reported residual + the yardstick's own (Weyl);
  - on the gapped families a vector equals the yardstick's within 2 (residual + the yardstick's own) / gap (Davis-Kahan
    for each of the two vectors against the eigenvector, gap the distance of its eigenvalue to the nearest other one)
    plus 2^-52, the rounding of the stored components of two unit vectors (half an ulp each).  The yardstick's own
    residual belongs there as it does in Weyl's bound: where the device's residual is below an ulp of lambda_1 (2.4e-16
    lambda_1 at n = 31, exactly 0 at n = 2) the distance between the two vectors is the yardstick's error, 8.3e-16
    against a bound of 7.8e-16 without that term.  This is a deviation from the issue's 2 residual / gap, which cannot be
    met against a computed yardstick: it bounds the distance to the eigenvector, and numpy's vector is itself
    2 (its residual) / gap away from that.  The ratio without the term is printed too.
Every test prints what it observed in units of its bound before it asserts."""
import ctypes as C

import numpy as np
import pytest

from diverseseq_amd import _lib, apps, cluster, distance, engine
from test_gpu_linkage import family_seqs
from test_pcoa_host import (EPS, GAPPED, IDENTITY_ABS, SCALES3, case, cloud_points, distances_between, project, sign_rule,
                            yardstick)

pytestmark = pytest.mark.gpu

POISON = "poison_blocks"


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_fit(a, b) -> bool:
    return all(same_bits(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def check_contract(fit, kind: str, n: int, tol: float = 1e-8, label: str = "", complement: bool = False):
    """what every result owes, whatever the family: shapes, the sign rule, the definitions of coordinates, proportion,
    trace and row means, honest residuals, orthonormal vectors orthogonal to 1, eigenvalues within Weyl's bound"""
    y = yardstick(kind, n)
    m = fit.values.size
    unit = y.unit(n)
    want, want_res = y.complement() if complement else (y.values, y.residuals)
    assert fit.vectors.shape == fit.coordinates.shape == (n, m) and fit.residuals.shape == fit.proportion.shape == (m,)
    assert (np.diff(fit.values) <= 0).all()
    assert same_bits(sign_rule(fit.vectors), fit.vectors)  # on the output alone
    true_res = np.linalg.norm(y.B @ fit.vectors - fit.vectors * fit.values, axis=0)
    honest = np.abs(true_res - fit.residuals).max() / unit
    basis = max(fit.basis, 1)
    orth = np.abs(fit.vectors.T @ fit.vectors - np.eye(m)).max() / ((n + 8) * EPS * basis)
    ones = np.abs(fit.vectors.sum(axis=0)).max() / ((n + 8) * EPS * basis * np.sqrt(n))
    weyl = (np.abs(fit.values - want[:m]) / (fit.residuals + want_res[:m] + np.finfo(float).tiny)).max()
    print(f"{label}{kind} n={n} m={m}: basis {fit.basis}, steps {fit.steps}, residual/lambda_1 {fit.residuals.max() / y.values[0]:.2e}"
          f" = {fit.residuals.max() / unit:.3g} units; |reported - true| {honest:.3g} units; |V^T V - I| {orth:.3g} of its bound,"
          f" |V^T 1| {ones:.3g}; |lambda^ - lambda| {weyl:.3g} of (residual + yardstick's)")
    assert honest <= 1.0
    assert orth <= 1.0 and ones <= 1.0
    assert weyl <= 1.0
    if fit.converged:
        assert (fit.residuals <= tol * fit.values[0]).all()
    # the definitions
    pos = fit.values > 0
    assert same_bits(fit.coordinates, np.where(pos, fit.vectors * np.sqrt(np.where(pos, fit.values, 0.0)), 0.0))
    assert (fit.coordinates[:, ~pos] == 0.0).all()
    assert same_bits(fit.proportion, fit.values / fit.trace)
    assert abs(fit.trace - y.trace) <= 4 * n * EPS * y.trace
    assert np.abs(fit.row_means - y.mu).max() <= 4 * n * EPS * np.abs(y.mu).max()
    return y


# The sizes.  2, 3, 4: the smallest; 9 .. 17: n - 1 <= 16 = b, the start block cannot be filled or is the whole space;
# 31: n < 2 b = 32, the second block cannot be filled; 15 .. 17: the 16 rows a product workgroup carries (4 waves of 4
# rows); 31 .. 33: the prepare pass's 32 x 32 tiles; 63 .. 65: the wave, whose lanes stride a row; 255 .. 257: the 256 threads that stride a column in the Gram,
# mean and norm kernels and the 256 rows per workgroup of the Ritz and update kernels; every n <= 512 has n - 1 < the
# default basis of 512 and may exhaust its space, 1025 may not
SIZES = [2, 3, 4, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1025]


@pytest.mark.parametrize("n", SIZES)
def test_point_clouds(ctx, n):
    for kind, p in GAPPED.items():
        m = min(p, n - 1)
        fit = cluster.pcoa(case(kind, n), m, ctx=ctx)
        assert fit.converged
        y = check_contract(fit, kind, n)
        # Davis-Kahan on the separated pairs
        for a in range(m):
            gap = y.gap(a)
            bound = 2 * (fit.residuals[a] + y.residuals[a]) / gap + EPS
            err = np.linalg.norm(fit.vectors[:, a] - y.vectors[:, a])
            print(f"  axis {a}: |v^ - v| = {err:.2e} = {err / bound:.3g} of 2 (residual + yardstick's) / gap + 2^-52, "
                  f"{err / (2 * fit.residuals[a] / gap + EPS):.3g} of 2 residual / gap + 2^-52")
            assert err <= bound


@pytest.mark.parametrize("kind,n,m", [("jsd", 300, 5), ("random", 300, 5), ("jsd", 1025, 3)])
def test_non_euclidean_families(ctx, kind, n, m):
    fit = cluster.pcoa(case(kind, n), m, ctx=ctx)
    assert fit.converged
    check_contract(fit, kind, n)


def test_negative_axes_give_zero_coordinates(ctx):
    n = 9  # n_axes = n - 1 reaches into the negative end of the jsd family
    fit = cluster.pcoa(case("jsd", n), n - 1, ctx=ctx)
    check_contract(fit, "jsd", n, complement=True)  # (the yardstick's pair of the vector 1 sorts among the negative ones)
    neg = fit.values <= 0
    assert neg.any() and (fit.coordinates[:, neg] == 0.0).all() and (fit.coordinates[:, ~neg] != 0.0).any()


@pytest.mark.parametrize("n", [11, 40, 257])
def test_constant_matrix_more_axes_than_a_block(ctx, n):
    c, m = 3.0, 10 if n == 11 else 20  # (n - 1 = 10 axes at most for n = 11; 20 > b = 16 otherwise)
    fit = cluster.pcoa(case("constant", n) * c, m, ctx=ctx)
    d = np.array(case("constant", n)) * c
    A = -0.5 * d * d
    unit = (n + 8) * EPS * np.linalg.norm(A)
    print(f"constant n={n}: |lambda - c^2/2| = {np.abs(fit.values - c * c / 2).max() / unit:.3g} units, residual "
          f"{fit.residuals.max() / unit:.3g} units, basis {fit.basis}")
    assert fit.converged and np.abs(fit.values - c * c / 2).max() <= unit
    assert np.abs(fit.vectors.T @ fit.vectors - np.eye(m)).max() <= (n + 8) * EPS * fit.basis
    assert np.abs(fit.vectors.sum(axis=0)).max() <= (n + 8) * EPS * fit.basis * np.sqrt(n)
    assert fit.trace == pytest.approx((n - 1) * c * c / 2, rel=1e-14)


def test_many_axes(ctx):
    n = 257  # 64 axes: eight chunks of the Ritz kernel; beyond the cloud's six the eigenvalues are zero to rounding
    fit = cluster.pcoa(case("cloud6", n), 64, ctx=ctx)
    check_contract(fit, "cloud6", n)
    nine = cluster.pcoa(case("cloud6", n), 9, ctx=ctx)  # one past a chunk
    check_contract(nine, "cloud6", n)


def test_crowded_matrix_runs_out_of_basis(ctx):
    n = 2049
    d = case("crowded", n)
    with pytest.raises(RuntimeError, match="worst residual"):
        cluster.pcoa(d, 3, max_basis=64, ctx=ctx)
    fit = cluster.pcoa(d, 3, max_basis=64, strict=False, ctx=ctx)
    assert fit.converged is False and fit.basis == 64 and fit.steps == 4
    y = check_contract(fit, "crowded", n)
    assert (fit.residuals > 1e-8 * fit.values[0]).any()
    print(f"crowded n={n}: residuals / lambda_1 = {fit.residuals / y.values[0]}")


@pytest.mark.parametrize("n", [100, 300])
def test_crowded_matrix_converges_when_the_space_is_exhausted(ctx, n):
    fit = cluster.pcoa(case("crowded", n), 4, ctx=ctx)
    assert fit.converged and fit.basis <= n - 1
    check_contract(fit, "crowded", n)


def test_basis_beyond_the_every_step_solves(ctx):
    """tol = 0 never converges: the basis runs to its limit, past the 256 columns up to which the small problem is solved
    after every step, and ends between two scheduled solves"""
    n = 600
    fit = cluster.pcoa(case("random", n), 3, tol=0.0, max_basis=284, strict=False, ctx=ctx)
    assert fit.basis == 284 and not fit.converged
    check_contract(fit, "random", n, tol=0.0)


@pytest.mark.parametrize("kind,n", [("cloud3", 65), ("cloud6", 257), ("cloud3", 1025), ("jsd", 300)])
def test_residual_floor(ctx, kind, n):
    """tol = 0 and the default basis: what the residual comes down to"""
    fit = cluster.pcoa(case(kind, n), 3, tol=0.0, strict=False, ctx=ctx)
    y = yardstick(kind, n)
    floor = fit.residuals.max()
    print(f"floor {kind} n={n}: residual {floor / y.unit(n):.3g} units = {floor / y.values[0]:.2e} lambda_1; "
          f"||A||_2 / lambda_1 = {np.linalg.norm(y.A, 2) / y.values[0]:.3g}")
    assert floor <= 1e-10 * y.values[0]  # the default tol = 1e-8 sits 100 x above


# ---- the same bits

def test_same_bits_twice_and_from_a_device_tensor(ctx):
    import torch

    n = 513
    d = np.array(case("jsd", n))
    host = cluster.pcoa(d, 4, ctx=ctx)
    assert same_fit(cluster.pcoa(d, 4, ctx=ctx), host)
    t = torch.from_numpy(d).to("cuda:0")
    assert same_fit(cluster.pcoa(t, 4, ctx=ctx), host)
    assert same_bits(t.cpu().numpy(), d)  # only read
    with pytest.raises(ValueError):
        cluster.pcoa(torch.zeros((4, 5), dtype=torch.float64, device="cuda:0"), 2, ctx=ctx)
    with pytest.raises(ValueError):
        cluster.pcoa(torch.zeros((5, 5), dtype=torch.float32, device="cuda:0"), 2, ctx=ctx)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            cluster.pcoa(torch.zeros((5, 5), dtype=torch.float64, device="cuda:1"), 2, ctx=ctx)


def _poison_case(c):
    seqs = family_seqs(5, 8, 1500, seed=21)
    arrays = [seqs[s] for s in seqs]
    out = list(cluster.pcoa(case("jsd", 129), 9, ctx=c))
    out += list(distance.jsd_pcoa(arrays, 4, n_axes=3, ctx=c))
    out += list(distance.mash_pcoa(arrays, 8, 200, n_axes=2, ctx=c))
    with distance.device_side(arrays, "jsd", 4, 4, ctx=c) as dev:
        marks = np.arange(0, 40, 2)
        fit = cluster.pcoa(dev.cross_distances(dev, marks, marks), 3, ctx=c)
        out += [dev.pcoa_project(fit, dev, None, marks)]
    return out


def test_poisoned_blocks_change_no_bit(monkeypatch):
    def fresh(runs):
        c = engine.Context(0)
        try:
            return [_poison_case(c) for _ in range(runs)]
        finally:
            c.close()

    clean, = fresh(1)
    monkeypatch.setenv("DVS_TEST_KNOBS", POISON)
    first, again = fresh(2)
    assert same_fit(first, clean) and same_fit(again, clean)


# ---- the three modes

@pytest.fixture(scope="module")
def family():
    seqs = family_seqs(10, 13, 3000, seed=17)
    return seqs, [seqs[s] for s in seqs]


@pytest.mark.parametrize("mode", ["mash", "euclidean", "jsd"])
def test_fused_modes_equal_the_matrix_route_bit_for_bit(ctx, family, mode):
    seqs, arrays = family
    if mode == "mash":
        fused = distance.mash_pcoa(arrays, 10, 500, n_axes=4, ctx=ctx)
        dist = distance.mash_distances(arrays, 10, 500, ctx=ctx)
        kw = dict(k=10, sketch_size=500)
    else:
        fused = distance.PCOA_MODES[mode](arrays, 5, n_axes=4, ctx=ctx)
        dist = distance.MODES[mode][0](arrays, 5, ctx=ctx)
        kw = dict(k=5, sketch_size=None, distance_mode=mode)
    assert same_fit(cluster.pcoa(dist, 4, ctx=ctx), fused)
    assert same_fit(distance.pcoa(arrays, 4, mode, ctx=ctx, **{k: v for k, v in kw.items() if k != "distance_mode"}), fused)
    names, ordn = cluster.ordinate(seqs, 4, **kw)
    assert names == list(seqs) and same_fit(ordn, fused)


def test_canonical_rows_and_count_matrices(ctx, family):
    _, arrays = family
    fused = distance.jsd_pcoa(arrays, 5, n_axes=3, ctx=ctx, canonical=True)
    assert same_fit(cluster.pcoa(distance.jsd_distances(arrays, 5, ctx=ctx, canonical=True), 3, ctx=ctx), fused)
    m = ctx.build_matrix(arrays, 5, 4)
    try:
        assert same_fit(distance.matrix_pcoa(m, "jsd", 4), distance.jsd_pcoa(arrays, 5, n_axes=4, ctx=ctx))
    finally:
        m.close()


def test_app_against_ordinate(family):
    seqs, _ = family
    kw = dict(k=5, sketch_size=None, distance_mode="jsd")
    got = apps.dvs_pcoa(3, **kw)(seqs)
    names, fit = cluster.ordinate(seqs, 3, **kw)
    assert got["names"] == names and same_bits(got["coordinates"], fit.coordinates)
    assert same_bits(got["proportion"], fit.proportion) and same_bits(got["eigenvalues"], fit.values)


# ---- projection

# the n-term sums of Gower's formula: sum_j (delta_j^2 - mu_j) v_j rounds at n eps sum |delta_j^2 - mu_j| |v_j|, the same
# order as the numpy evaluation behind the host file's measured 3e-14 (IDENTITY_ABS = 1e-13 already holds a margin of 3);
# the device's fit differs from the yardstick's by its residual / gap (1e-15 .. 1e-13 on the clouds, printed above), which
# the margin of 10 covers; the sums at these n are no longer than the host file's n = 200
PROJECT_MARGIN = 10


def cloud_freqs(p: np.ndarray) -> np.ndarray:
    """frequency rows (eight bins, sums of 1) whose euclidean distances are those of the 3-D points p shrunk by 400:
    1/8 + p U / 400 with three orthonormal directions U of zero sum"""
    u = np.zeros((3, 8))
    for a in range(3):
        u[a, 2 * a], u[a, 2 * a + 1] = np.sqrt(0.5), -np.sqrt(0.5)
    f = 0.125 + (p / 400.0) @ u
    assert (f > 0).all()
    return f


@pytest.fixture(scope="module")
def euclid_cloud(ctx):
    """frequency rows whose euclidean distances are those of a 3-D cloud: n fitted rows and 17 held-out ones"""
    n, extra = 257, 17
    p = np.concatenate([cloud_points(n, SCALES3, 1), cloud_points(extra, SCALES3, 11)])
    m = ctx.matrix_from_freqs(cloud_freqs(p))
    yield n, extra, p, m
    m.close()


@pytest.mark.parametrize("strip", [None, 1, 32, 33])
def test_projection_identities_and_strip_heights(ctx, monkeypatch, euclid_cloud, strip):
    n, extra, p, m = euclid_cloud
    side = distance.DeviceSide(m, "euclidean")
    rows = np.arange(n)
    # both identities hold to the fit's residual / sqrt(lambda_a): a fit at its floor (tol = 0: the basis runs to n - 1
    # columns), as the dense solver's of the host file is, not one that stopped anywhere below tol = 1e-8
    fit = cluster.pcoa(side.cross_distances(side, rows, rows), 3, tol=0.0, strict=False, ctx=ctx)
    default = side.pcoa_project(fit, side, None, rows)
    if strip is not None:
        monkeypatch.setenv("DVS_CROSS_STRIP_ROWS", str(strip))
        assert same_bits(side.pcoa_project(fit, side, None, rows), default)
        return
    scale = 400.0  # the frequency rows are the cloud shrunk by 400
    # a fitted row gets its own coordinates back
    own = np.abs(default[:n] - fit.coordinates).max() * scale
    # held-out points keep their distances to the fitted ones (rank 3, three axes)
    held = np.abs(distances_between(default[n:], fit.coordinates) * scale - distances_between(p[n:], p[:n])).max()
    # ... and against the yardstick's formula over the same cells
    cells = side.cross_distances(side, None, rows)
    ref = project(cells, fit.values, fit.vectors, fit.row_means)
    print(f"projection: own coordinates {own:.2e}, held-out distances {held:.2e} (bound {PROJECT_MARGIN * IDENTITY_ABS:.1e}), "
          f"against numpy {np.abs(default - ref).max() * scale:.2e}")
    assert own <= PROJECT_MARGIN * IDENTITY_ABS and held <= PROJECT_MARGIN * IDENTITY_ABS
    assert np.abs(default - ref).max() * scale <= PROJECT_MARGIN * IDENTITY_ABS


def test_projection_row_lists_nan_rows_and_many_axes(ctx):
    rng = np.random.default_rng(23)
    seqs = [rng.integers(0, 4, int(rng.integers(200, 900)), dtype=np.uint8) for _ in range(90)]
    seqs[7] = np.full(300, 4, np.uint8)  # no valid k-mer: NaN cells
    fitted = np.array([r for r in rng.permutation(90) if r != 7][:60])
    with distance.device_side(seqs, "jsd", 3, 4, ctx=ctx) as dev:
        fit = cluster.pcoa(dev.cross_distances(dev, fitted, fitted), 9, ctx=ctx)  # nine axes: one past a chunk of eight
        queries = np.array([5, 7, 80, 7, int(fitted[3])])
        got = dev.pcoa_project(fit, dev, queries, fitted)
        assert got.shape == (5, 9)
        assert np.isnan(got[[1, 3]]).all() and np.isfinite(got[[0, 2, 4]]).all()
        ref = project(dev.cross_distances(dev, queries, fitted), fit.values, fit.vectors, fit.row_means)
        fin = [0, 2, 4]
        unit = 60 * EPS * np.abs(fit.coordinates).max() / np.sqrt(fit.values[fit.values > 0].min() / fit.values[0])
        print(f"row lists: |device - numpy| = {np.abs(got[fin] - ref[fin]).max():.2e} (bound {8 * unit:.2e})")
        assert np.abs(got[fin] - ref[fin]).max() <= 8 * unit
        assert np.abs(got[4] - fit.coordinates[3]).max() <= 1e-9 * np.abs(fit.coordinates).max()  # a fitted row, listed
        assert same_bits(dev.pcoa_project(fit, dev, queries[:0], fitted), np.zeros((0, 9)))
        with pytest.raises(ValueError):
            dev.pcoa_project(fit, dev, queries, fitted[:-1])  # not the fitted rows
        with pytest.raises(ValueError):
            dev.pcoa_project(fit, dev, [90], fitted)


def test_projection_mixed_element_widths(ctx, monkeypatch):
    rng = np.random.default_rng(29)
    q = [rng.integers(0, 4, int(rng.integers(300, 2500)), dtype=np.uint8) for _ in range(20)]
    r = [rng.integers(0, 4, int(rng.integers(300, 2500)), dtype=np.uint8) for _ in range(40)]
    k = 4
    sides = {2: (ctx.build_matrix(q, k, 4), ctx.build_matrix(r, k, 4))}
    monkeypatch.setenv("DVS_COUNTS_U32", "1")
    sides[4] = (ctx.build_matrix(q, k, 4), ctx.build_matrix(r, k, 4))
    monkeypatch.delenv("DVS_COUNTS_U32")
    try:
        for w, (a, b) in sides.items():
            assert a.count_bytes == b.count_bytes == w
        fit = distance.matrix_pcoa(sides[2][1], "jsd", 3)
        want = distance.matrix_pcoa_project(fit, sides[2][0], sides[2][1], "jsd")
        for wq in sides:
            for wr in sides:
                assert same_bits(distance.matrix_pcoa_project(fit, sides[wq][0], sides[wr][1], "jsd"), want)
        assert same_bits(distance.pcoa_project(fit, q, r, "jsd", k=k, ctx=ctx), want)
    finally:
        for a, b in sides.values():
            a.close()
            b.close()


def test_landmark_pcoa_reproduces_the_distances_of_a_rank_3_cloud():
    n, marks = 2049, 64
    p = cloud_points(n, SCALES3, 31)
    # sequences would not give a rank-3 cloud: landmark_pcoa runs over a DeviceSide of frequency rows
    c = engine.Context(0)
    m = c.matrix_from_freqs(cloud_freqs(p))
    try:
        side = distance.DeviceSide(m, "euclidean")
        names, coords, picks, fit = cluster.landmark_pcoa(side, marks, 3)
        full = side.pcoa(3)
        assert names is None and coords.shape == (n, 3) and len(set(picks.tolist())) == marks
        assert same_bits(coords, side.pcoa_project(fit, side, None, picks))
    finally:
        m.close()
        c.close()
    # landmarks of rank-3 data fix the embedding up to a rigid motion: inter-point distances, not coordinates
    some = np.arange(0, n, 16)
    d_land = distances_between(coords[some], coords)
    d_full = distances_between(full.coordinates[some], full.coordinates)
    d_true = distances_between(p[some], p) / 400.0
    # Davis-Kahan over both fits: a coordinate moves by |x| (residual / gap) per axis; the distances by twice that.  The
    # floor is the same bound for the input's own rounding: a frequency 1/8 + x is stored to 2^-52 / 8, a distance over
    # six such bins to 4 sqrt(6) 2^-52 / 8, its square to 2 d times that, and ||delta B||_2 <= n max |delta d^2| moves a
    # vector by ||delta B|| / gap.  It is a worst case (every cell's error aligned); the observed figures, from roundings
    # of random sign, sit some four orders below it
    gap = min(yardstick_gap(fit.values), yardstick_gap(full.values))
    floor = n * 2 * d_true.max() * (4 * np.sqrt(6) * EPS / 8) / (gap * full.values[0])
    bound = 4 * 3 * max(np.abs(coords).max(), np.abs(full.coordinates).max()) * max(
        fit.residuals.max() / (gap * fit.values[0]), full.residuals.max() / (gap * full.values[0]), floor)
    print(f"landmarks: |d_landmark - d_full| = {np.abs(d_land - d_full).max():.2e}, |d_landmark - d_true| = "
          f"{np.abs(d_land - d_true).max():.2e} (bound {bound:.2e}, its floor term {floor:.2e})")
    assert np.abs(d_land - d_full).max() <= bound and np.abs(d_land - d_true).max() <= bound


def yardstick_gap(values) -> float:
    """the least relative gap among the returned eigenvalues and to zero (a rank-3 cloud: the rest are zero)"""
    v = np.append(np.asarray(values), 0.0) / values[0]
    return float(np.abs(np.diff(v)).min())


def test_landmark_pcoa_over_sequences(family):
    seqs, arrays = family
    L = 40
    names, coords, marks, fit = cluster.landmark_pcoa(seqs, L, 3, k=5, sketch_size=None, distance_mode="jsd")
    assert names == list(seqs) and coords.shape == (len(seqs), 3) and marks.shape == (L,) and fit.values.shape == (3,)
    assert len(set(marks.tolist())) == L and (fit.values > 0).all()
    dist = distance.jsd_distances(arrays, 5)
    assert same_fit(cluster.pcoa(dist[np.ix_(marks, marks)], 3), fit)
    # every row, the landmarks or not, is what the projection gives it, bit for bit
    with distance.device_side(arrays, "jsd", 5, 4) as dev:
        assert same_bits(coords, dev.pcoa_project(fit, dev, None, marks))
    # ... which is Gower's formula over the row's cells, to the rounding of an L-term sum
    terms = (np.abs(dist[:, marks] ** 2 - fit.row_means) @ np.abs(fit.vectors)) * 0.5 / np.sqrt(fit.values)
    rounding = (L + 8) * EPS * terms.max()
    ref = project(dist[:, marks], fit.values, fit.vectors, fit.row_means)
    # the landmarks get their own coordinates back: v^T B e_i = lambda v_i + r_i, so to residual / sqrt(lambda) and that rounding
    own = np.abs(coords[marks] - fit.coordinates).max()
    bound = (fit.residuals / np.sqrt(fit.values)).max() + rounding
    print(f"landmarks over sequences: |device - numpy| = {np.abs(coords - ref).max() / rounding:.3g} of the sum's rounding; own "
          f"coordinates {own:.2e} = {own / bound:.3g} of residual / sqrt(lambda) + rounding")
    assert np.abs(coords - ref).max() <= 2 * rounding  # (both sides round)
    assert own <= bound


# ---- errors, at the Python boundary and at the C boundary; the context stays usable after each

def _still_usable(ctx):
    fit = cluster.pcoa(case("cloud3", 33), 2, ctx=ctx)
    assert fit.converged


def test_errors_python_boundary(ctx):
    d = np.array(case("cloud3", 65))
    bad = d.copy()
    bad[3, 40] += 1e-9  # one side only
    with pytest.raises(ValueError, match="not symmetric"):
        cluster.pcoa(bad, 2, ctx=ctx)
    _still_usable(ctx)
    for value in (np.nan, np.inf, -np.inf):
        for where in ((2, 7), (7, 2), (64, 63)):
            bad = d.copy()
            bad[where] = value
            with pytest.raises(ValueError, match="NaN or infinity"):
                cluster.pcoa(bad, 2, ctx=ctx)
    _still_usable(ctx)
    weird = d.copy()
    np.fill_diagonal(weird, np.nan)  # the diagonal counts as 0 and is never read
    assert same_fit(cluster.pcoa(weird, 2, ctx=ctx), cluster.pcoa(d, 2, ctx=ctx))
    no_kmers = [np.full(50, 4, np.uint8), np.arange(50, dtype=np.uint8) % 4, np.ones(50, np.uint8), np.arange(50, dtype=np.uint8) % 3]
    for mode in ("euclidean", "jsd"):
        with pytest.raises(ValueError, match="NaN or infinity"):
            distance.PCOA_MODES[mode](no_kmers, 3, n_axes=2, ctx=ctx)
    empty = [np.zeros(3, np.uint8), np.ones(2, np.uint8), np.arange(40, dtype=np.uint8) % 4]
    with pytest.raises(ZeroDivisionError):
        distance.mash_pcoa(empty, 8, 10, n_axes=2, ctx=ctx)
    _still_usable(ctx)


def test_errors_c_boundary(ctx):
    L = ctx._L
    f64 = C.POINTER(C.c_double)
    n = 9
    d = np.ascontiguousarray(case("cloud3", n))
    values, residuals, mu = np.zeros(64), np.zeros(64), np.zeros(n)
    vectors = np.zeros((n, 64))
    info = _lib.PcoaInfo()

    def given(count=n, on_device=0, handle=d.ctypes.data, rows=None):
        return distance.make_source(_lib.SRC_GIVEN, handle, count, rows, on_device=on_device)

    def call(src, n_axes=2, max_basis=0, tol=1e-8, params=True, out=True):
        p = _lib.PcoaParams(n_axes, max_basis, tol)
        return L.dvs_pcoa(ctx._h, src, C.byref(p) if params else None, values.ctypes.data_as(f64) if out else None,
                          vectors.ctypes.data_as(f64), residuals.ctypes.data_as(f64), mu.ctypes.data_as(f64), C.byref(info))

    assert call(given()) == _lib.OK and info.converged == 2 and info.basis == 8 and info.steps == 1 and info.products == 8
    assert call(given(1)) == _lib.ERR_VALUE                      # n < 2
    assert call(given(), n_axes=0) == _lib.ERR_VALUE
    assert call(given(), n_axes=n) == _lib.ERR_VALUE             # n_axes > n - 1
    assert call(given(), tol=-1.0) == _lib.ERR_VALUE
    assert call(given(), tol=float("nan")) == _lib.ERR_VALUE
    assert call(given(), n_axes=3, max_basis=2) == _lib.ERR_VALUE
    assert call(given(), n_axes=65) == _lib.ERR_UNSUPPORTED      # (before n is looked at)
    assert call(given(), params=False) == _lib.ERR_VALUE
    assert call(given(), out=False) == _lib.ERR_VALUE
    assert call(given(handle=None)) == _lib.ERR_VALUE
    assert call(given(on_device=1)) == _lib.ERR_VALUE            # a host pointer said to be device memory
    rows = np.arange(n, dtype=np.uint32)
    assert call(given(rows=rows)) == _lib.ERR_VALUE              # a caller's matrix takes no row list
    big = 200_000                                                # 320 GB of matrix: more than the device holds
    assert call(given(big)) == _lib.ERR_NOMEM
    m = ctx.build_matrix([np.arange(60, dtype=np.uint8) % 4, np.arange(70, dtype=np.uint8) % 3, np.ones(50, np.uint8)], 2, 4)
    try:
        listed = distance.make_source(_lib.SRC_JSD, m._h, 3, np.arange(3, dtype=np.uint32))
        assert call(listed) == _lib.ERR_UNSUPPORTED              # a row list
        assert b"dvs_pcoa" in L.dvs_last_error(ctx._h)
        assert call(distance.make_source(_lib.SRC_JSD, m._h, 2)) == _lib.ERR_UNSUPPORTED  # some of the rows
        whole = distance.make_source(_lib.SRC_JSD, m._h, 3)
        assert call(whole) == _lib.OK
        # the projection's own
        coords = np.zeros((3, 2))
        table = (values.ctypes.data_as(f64), vectors.ctypes.data_as(f64), mu.ctypes.data_as(f64))
        assert L.dvs_pcoa_project(ctx._h, whole, whole, 2, *table, coords.ctypes.data_as(f64)) == _lib.OK
        assert L.dvs_pcoa_project(ctx._h, whole, whole, 0, *table, coords.ctypes.data_as(f64)) == _lib.ERR_VALUE
        assert L.dvs_pcoa_project(ctx._h, whole, whole, 65, *table, coords.ctypes.data_as(f64)) == _lib.ERR_UNSUPPORTED
        assert L.dvs_pcoa_project(ctx._h, whole, whole, 2, None, table[1], table[2], coords.ctypes.data_as(f64)) == _lib.ERR_VALUE
        assert L.dvs_pcoa_project(ctx._h, whole, whole, 2, *table, None) == _lib.ERR_VALUE
        none = distance.make_source(_lib.SRC_JSD, m._h, 0)
        assert L.dvs_pcoa_project(ctx._h, whole, none, 2, *table, coords.ctypes.data_as(f64)) == _lib.ERR_VALUE  # r->n == 0
        assert L.dvs_pcoa_project(ctx._h, none, whole, 2, *table, coords.ctypes.data_as(f64)) == _lib.OK         # no queries
        assert L.dvs_pcoa_project(ctx._h, given(), given(), 2, *table, coords.ctypes.data_as(f64)) == _lib.ERR_UNSUPPORTED
        euclid = distance.make_source(_lib.SRC_EUCLIDEAN, m._h, 3)
        assert L.dvs_pcoa_project(ctx._h, whole, euclid, 2, *table, coords.ctypes.data_as(f64)) == _lib.ERR_VALUE
    finally:
        m.close()
    _still_usable(ctx)
