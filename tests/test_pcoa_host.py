"""The yardstick and the cases of the principal-coordinates tests (tests/test_gpu_pcoa.py), pinned on the CPU.

Yardstick: B = J (-1/2 D o D) J formed from the definition (include/dvs_hip.h "principal coordinates"), the centring in
np.longdouble and rounded to float64 once, then numpy.linalg.eigh, sorted descending, the sign rule applied.  It is
pinned here against scipy.linalg.eigh and against closed forms; its own relative residual ||B v - lambda v|| / lambda_1
is printed per case.  The cases are seeded and the properties the GPU tests rely on -- the gaps of the point clouds,
the negative end of the non-Euclidean families, the bulk of the crowded matrix -- are asserted here, together with the
two projection identities in numpy and the argument checks of the Python layer that need no device."""
import functools

import numpy as np
import pytest

from diverseseq_amd import cluster, distance

EPS = 2.0 ** -52
SCALES3 = (5.0, 2.0, 1.0)
SCALES6 = (8.0, 5.0, 3.0, 2.0, 1.2, 0.7)
# relative gap between consecutive leading eigenvalues of a cloud, in units of lambda_1: >= 0.009 on these seeds
# (asserted in test_cloud_gaps); the last of them stands (0.7 / 8)^2 ~ 0.0077 lambda_1 above the rest, which are zero to
# rounding.  `Yardstick.gap` is what a Davis-Kahan bound takes: each pair's distance to the nearest other eigenvalue
CLOUD_GAP = 0.009
# the two projection identities on scale-5 clouds, measured at 3e-14 absolute in numpy (asserted below with this bound)
IDENTITY_ABS = 1e-13


# ---- the cases

def cloud_points(n: int, scales=SCALES3, seed: int = 1) -> np.ndarray:
    return np.random.default_rng(seed).normal(size=(n, len(scales))) * np.asarray(scales)


def distances_between(p: np.ndarray, q: np.ndarray) -> np.ndarray:
    return np.sqrt(((p[:, None, :] - q[None, :, :]) ** 2).sum(axis=2))


def cloud(n: int, scales=SCALES3, seed: int = 1) -> np.ndarray:
    """the Euclidean distances of n points of dimension len(scales): B has rank len(scales)"""
    p = cloud_points(n, scales, seed)
    d = distances_between(p, p)
    d = (d + d.T) / 2
    np.fill_diagonal(d, 0.0)
    return d


def constant(n: int, c: float = 1.0) -> np.ndarray:
    """c (11^T - I): lambda = c^2 / 2 with multiplicity n - 1"""
    return c * (np.ones((n, n)) - np.eye(n))


def jsd_dirichlet(n: int, bins: int = 64, seed: int = 2) -> np.ndarray:
    """the Jensen-Shannon divergences (bits) of n Dirichlet(1/2) frequency rows: not Euclidean"""
    f = np.random.default_rng(seed).dirichlet(np.full(bins, 0.5), size=n)

    def h(p):
        with np.errstate(divide="ignore", invalid="ignore"):
            return -np.where(p > 0, p * np.log2(p), 0.0).sum(axis=-1)

    hf = h(f)
    d = np.empty((n, n))
    for i in range(n):
        d[i] = h((f[i] + f) / 2) - (hf[i] + hf) / 2
    d = np.maximum((d + d.T) / 2, 0.0)
    np.fill_diagonal(d, 0.0)
    return d


def random_symmetric(n: int, seed: int = 3) -> np.ndarray:
    u = np.random.default_rng(seed).random((n, n))
    d = (u + u.T) / 2
    np.fill_diagonal(d, 0.0)
    return d


def crowded(n: int, seed: int = 4) -> np.ndarray:
    """0.7 + 0.01 u: a bulk spectrum without gaps, the non-convergence case"""
    u = np.random.default_rng(seed).random((n, n))
    d = 0.7 + 0.01 * (u + u.T) / 2
    np.fill_diagonal(d, 0.0)
    return d


CASES = {"cloud3": cloud, "cloud6": functools.partial(cloud, scales=SCALES6, seed=5), "constant": constant,
         "jsd": jsd_dirichlet, "random": random_symmetric, "crowded": crowded}
GAPPED = {"cloud3": len(SCALES3), "cloud6": len(SCALES6)}  # family -> its leading, separated eigenvalues


@functools.lru_cache(maxsize=None)
def case(kind: str, n: int) -> np.ndarray:
    d = CASES[kind](n)
    d.setflags(write=False)
    return d


# ---- the yardstick

def sign_rule(v: np.ndarray) -> np.ndarray:
    """every column with its component of largest magnitude (the lowest index on a tie) positive"""
    v = np.array(v, dtype=np.float64)
    for a in range(v.shape[1]):
        if v[np.argmax(np.abs(v[:, a])), a] < 0:
            v[:, a] = -v[:, a]
    return v


def centred(d: np.ndarray):
    """-> (A, B, mu, trace) of the definition; the diagonal of d is not read"""
    n = d.shape[0]
    a = -0.5 * np.asarray(d, dtype=np.longdouble) ** 2
    np.fill_diagonal(a, 0.0)
    r = a.mean(axis=1)
    b = a - (r[:, None] + r[None, :]) + a.mean()
    mu = (-2 * r).astype(np.float64)
    return a.astype(np.float64), b.astype(np.float64), mu, float(-a.sum() / n)


class Yardstick:
    def __init__(self, d: np.ndarray):
        self.A, self.B, self.mu, self.trace = centred(d)
        w, v = np.linalg.eigh(self.B)
        order = np.argsort(-w, kind="stable")
        self.values, self.vectors = w[order], sign_rule(v[:, order])
        self.fro = float(np.linalg.norm(self.A))  # ||A||_F
        # its own absolute residuals, ||B v - lambda v||_2 per pair
        self.residuals = np.linalg.norm(self.B @ self.vectors - self.vectors * self.values, axis=0)

    def gap(self, a: int) -> float:
        """the distance of eigenvalue a to the nearest other one"""
        others = np.delete(self.values, a)
        return float(np.abs(others - self.values[a]).min())

    def complement(self):
        """(values, residuals) without the pair of the vector 1, whose eigenvalue 0 sorts among the others once B has
        negative eigenvalues -- the definition's axes are orthogonal to 1.  Only where 0 is a simple eigenvalue."""
        n = self.vectors.shape[0]
        along = np.abs(self.vectors.sum(axis=0)) / np.sqrt(n)
        one = int(np.argmax(along))
        assert along[one] > 1 - 1e-8
        return np.delete(self.values, one), np.delete(self.residuals, one)

    def unit(self, n: int) -> float:
        """(n + 8) 2^-52 ||A||_F: the rounding of one pass over A in f64, the unit of the device tests' bounds"""
        return (n + 8) * EPS * self.fro


@functools.lru_cache(maxsize=None)
def yardstick(kind: str, n: int) -> Yardstick:
    return Yardstick(case(kind, n))


def project(d_query: np.ndarray, values, vectors, mu) -> np.ndarray:
    """Gower's add-a-point formula in numpy: x_a = -1/2 v_a^T (delta o delta - mu) / sqrt(lambda_a), 0 for lambda_a <= 0"""
    values = np.asarray(values, dtype=np.float64)
    pos = values > 0
    scale = np.where(pos, -0.5 / np.sqrt(np.where(pos, values, 1.0)), 0.0)
    return ((d_query * d_query - mu) @ vectors) * scale


# ---- the yardstick pinned

@pytest.mark.parametrize("kind,n", [("cloud3", 65), ("cloud6", 257), ("jsd", 300), ("random", 300), ("crowded", 300)])
def test_yardstick_against_scipy_and_its_own_residual(kind, n):
    scipy_linalg = pytest.importorskip("scipy.linalg")
    y = yardstick(kind, n)
    w = scipy_linalg.eigh(y.B, eigvals_only=True)[::-1]
    top = abs(y.values[0])
    assert np.abs(w - y.values).max() <= 64 * n * EPS * top
    rel = y.residuals.max() / top
    print(f"{kind} n={n}: yardstick's relative residual {rel:.2e}, lambda_min / lambda_1 = {y.values[-1] / top:.3f}")
    assert rel <= 64 * n * EPS
    assert abs(y.values.sum() - y.trace) <= 64 * n * EPS * np.abs(y.values).sum()
    away = np.abs(y.values) > 1e-8 * top  # (1 lies in the null space, where eigh may mix it with others)
    assert np.abs(y.vectors[:, away].T @ np.ones(n)).max() <= 1e-6 * np.sqrt(n)


def test_constant_matrix_closed_form():
    n, c = 9, 3.0
    y = Yardstick(constant(n, c))
    assert np.abs(y.values[: n - 1] - c * c / 2).max() <= 16 * EPS * c * c
    assert abs(y.values[-1]) <= 16 * EPS * c * c
    assert y.trace == pytest.approx((n - 1) * c * c / 2, rel=1e-15)
    assert np.allclose(y.mu, (n - 1) * c * c / n, rtol=1e-15)


def test_two_points_closed_form():
    y = Yardstick(np.array([[0.0, 3.0], [3.0, 0.0]]))
    assert y.values[0] == pytest.approx(4.5, rel=1e-15)  # d^2 / 2
    assert np.allclose(y.vectors[:, 0], [np.sqrt(0.5), -np.sqrt(0.5)])


@pytest.mark.parametrize("kind,n", [(k, n) for k in GAPPED for n in (63, 64, 65, 257, 1025)])
def test_cloud_gaps(kind, n):
    p = GAPPED[kind]
    w = yardstick(kind, n).values
    lead = w[:p] / w[0]
    gaps = lead[:-1] - lead[1:]
    rest = np.abs(w[p:]).max() / w[0]
    print(f"{kind} n={n}: leading {lead[:p].round(4)}, least gap {gaps.min():.4f}, the rest {rest:.1e} lambda_1")
    assert gaps.min() >= CLOUD_GAP
    assert rest <= (n + 8) * EPS
    assert lead[-1] - rest >= 0.005  # ... and the last of them from the rest


def test_the_non_euclidean_families_have_a_negative_end():
    j = yardstick("jsd", 300).values
    assert j[-1] < 0
    r = yardstick("random", 300).values
    assert r[-1] / r[0] < -0.5
    print(f"jsd lambda_min / lambda_1 = {j[-1] / j[0]:.3f}, random {r[-1] / r[0]:.3f}")


def test_complement_drops_the_pair_of_the_vector_one():
    y = yardstick("jsd", 9)
    values, _ = y.complement()
    assert values.size == 8 and values[-1] < 0 and abs(values.sum() - y.trace) <= 64 * EPS * np.abs(values).sum()


def test_the_crowded_matrix_is_a_bulk():
    w = yardstick("crowded", 300).values
    lead = w[:12] / w[0]
    assert (lead[:-1] - lead[1:]).max() < 0.05  # no gap among the leading eigenvalues to converge into


# ---- the identities of the projection, in numpy

@pytest.mark.parametrize("n", [65, 200])
def test_a_training_row_projects_onto_its_own_coordinates(n):
    d = case("cloud3", n)
    y = yardstick("cloud3", n)
    m = 3
    x = y.vectors[:, :m] * np.sqrt(y.values[:m])
    err = np.abs(project(d, y.values[:m], y.vectors[:, :m], y.mu) - x).max()
    print(f"n={n}: self-projection error {err:.2e}")
    assert err <= IDENTITY_ABS


def test_held_out_points_of_a_rank_p_cloud_keep_their_distances():
    n, m = 200, 3
    p, q = cloud_points(n, SCALES3, 1), cloud_points(17, SCALES3, 11)
    y = yardstick("cloud3", n)
    x = y.vectors[:, :m] * np.sqrt(y.values[:m])
    xq = project(distances_between(q, p), y.values[:m], y.vectors[:, :m], y.mu)
    err = np.abs(distances_between(xq, x) - distances_between(q, p)).max()
    print(f"held-out distance error {err:.2e}")
    assert err <= IDENTITY_ABS


# ---- the Python layer's argument checks that need no device

@pytest.mark.parametrize("bad", [0, -1, 1.5, True, "3", 5, 70])
def test_n_axes_is_checked_before_the_handle(bad):
    with pytest.raises((ValueError, NotImplementedError)):
        distance.check_pcoa_args(5, bad, 1e-8, None)


def test_n_axes_beyond_64_is_not_implemented():
    with pytest.raises(NotImplementedError):
        distance.check_pcoa_args(100, 65, 1e-8, None)
    assert distance.check_pcoa_args(100, 64, 1e-8, None) == (64, 1e-8, 0)


@pytest.mark.parametrize("tol", [-1.0, float("nan"), None, "1e-8", True])
def test_tol_is_checked(tol):
    with pytest.raises(ValueError):
        distance.check_pcoa_args(10, 3, tol, None)


@pytest.mark.parametrize("max_basis", [2, 0, -5, 3.5, True])
def test_max_basis_is_checked(max_basis):
    with pytest.raises(ValueError):
        distance.check_pcoa_args(10, 3, 1e-8, max_basis)


def test_too_few_rows_and_bad_shapes_raise_before_any_device_work():
    with pytest.raises(ValueError):
        cluster.pcoa(np.zeros((1, 1)), 1)
    with pytest.raises(ValueError):
        cluster.pcoa(np.zeros((4, 5)), 2)
    with pytest.raises(ValueError):
        cluster.pcoa(np.zeros((4, 4)), 4)  # n - 1 axes at most
    with pytest.raises(ValueError):
        cluster.ordinate({"a": np.zeros(9, np.uint8)}, 1, k=2)
    with pytest.raises(ValueError):
        cluster.ordinate({"a": np.zeros(9, np.uint8), "b": np.zeros(9, np.uint8)}, 1, k=2, distance_mode="nope")
    with pytest.raises(ValueError):
        cluster.landmark_pcoa({c: np.zeros(9, np.uint8) for c in "abcd"}, 3, 3, k=2)  # 3 landmarks hold 2 axes
    with pytest.raises(ValueError):
        distance.pcoa([np.zeros(9, np.uint8)] * 3, 3, "jsd", k=2)


def test_a_fit_is_checked_before_any_device_work():
    fit = distance.PCoA(np.ones(2), np.zeros((5, 2)), None, None, None, np.zeros(5), 1.0, True, 4, 1)
    assert distance.check_pcoa_fit(fit, 5)[1].shape == (5, 2)
    with pytest.raises(ValueError):
        distance.check_pcoa_fit(fit, 6)  # the references are not the fitted rows
    with pytest.raises(ValueError):
        distance.check_pcoa_fit(fit._replace(vectors=np.zeros((5, 3))), 5)
    with pytest.raises(ValueError):
        distance.check_pcoa_fit(object(), 5)
    with pytest.raises(ValueError):
        distance.pcoa_project(fit, [np.zeros(9, np.uint8)], [np.zeros(9, np.uint8)] * 4, "jsd", k=2)


def test_the_app_checks_its_arguments():
    from diverseseq_amd import apps

    with pytest.raises(ValueError):
        apps.dvs_pcoa(0)
    with pytest.raises(ValueError):
        apps.dvs_pcoa(65)
    with pytest.raises(ValueError):
        apps.dvs_pcoa(2, distance_mode="nope")
    with pytest.raises(ValueError):
        apps.dvs_pcoa(2, distance_mode="mash", canonical=True)
    assert "dvs_pcoa" in apps.__all__
