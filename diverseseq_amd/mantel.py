"""The Mantel test on the GPU (csrc/mantel.hip; include/dvs_hip.h "Mantel"): do two distance matrices over the same
items agree beyond what chance gives?  The Pearson correlation r of the cells above the diagonal of the two matrices,
and a p-value from the same correlation after the items of the second matrix are permuted.

Each side is a `distance.DeviceSide` -- the sketches or the count matrix of a collection, whose distances are written
in HBM and never leave it -- or a caller's square matrix, array-like or a contiguous float64 device tensor (waited for
and only read), in any mix: it is the one operation of the package over two sources of different kinds, which is why it
lives here and not on a `DeviceSide`.  `mantel` takes two sides, `of_sequences` builds both from one collection of
sequences by two distance modes, `dvs_mantel` is the app.  The library returns sums and counts (`run_mantel`, the one C
call); r and p are derived here, and the permutations are drawn here (`permutations`, by the rule of
`distance.permuted_labels`).

This module imports downwards only (`distance`, `cluster`, `apps`, `engine`, `_lib`); nothing imports it back."""

from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _lib, apps, cluster, distance, engine

__all__ = ["ALTERNATIVES", "Mantel", "permutations", "mantel_statistics", "run_mantel", "mantel", "of_sequences", "dvs_mantel"]

ALTERNATIVES = ("two-sided", "greater", "less")
_MODE_KEYS = ("distance_mode", "k", "sketch_size", "num_states", "mash_canonical", "canonical")


class Mantel(NamedTuple):
    """A Mantel test of n items.  r: Pearson's correlation of the cells above the diagonal, nan where either matrix
    is constant; p_value: (1 + count) / (1 + permutations), the count of the permutations at least as extreme as the
    observed arrangement in the sense of `alternative` -- "two-sided": n_abs_ge, "greater": n_ge, "less": n_le -- nan
    where r is nan or permutations = 0; z float64 [permutations + 1]: the cross sums Z of the shifted cells, [0] the
    observed; r_permuted float64 [permutations]: r under each permutation, in the order they were drawn; n_ge, n_le,
    n_abs_ge: the counts, taken on z in float64; moments float64 [6]: s_x, s_y, A, B, S_uu, S_vv; passes: the reads of a
    matrix's upper triangle."""
    r: float
    p_value: float
    alternative: str
    n: int
    permutations: int
    z: np.ndarray
    r_permuted: np.ndarray
    n_ge: int
    n_le: int
    n_abs_ge: int
    moments: np.ndarray
    passes: int


def permutations(n: int, permutations: int, seed=None, strata=None) -> np.ndarray:
    """the permutations of a Mantel run: uint32 [permutations, n], row p holding at position i the item of the second
    matrix that stands there.  The draws are those of `distance.permuted_labels`: default_rng(seed), one
    rng.permutation(n) per row, in order; with strata (one hashable per item) the items are re-dealt inside their
    block only.  For any labels, distance.permuted_labels(labels, P, seed, strata) == labels[permutations(n, P, seed,
    strata)] row by row."""
    blocks = None if strata is None else distance.encode_grouping(strata, n, "strata")[0]
    return distance.permuted_labels(np.arange(n, dtype=np.uint32), int(permutations), seed, blocks)


_draw = permutations  # (the functions below have a `permutations` argument of their own)


def mantel_statistics(n: int, moments, z) -> np.ndarray:
    """r of every entry of z from the sums, as include/dvs_hip.h states it, in np.longdouble and rounded once ->
    float64 of z's shape; nan where either variance factor is <= 0"""
    ld = np.longdouble
    m = ld(n * (n - 1) // 2)
    _, _, a, b, suu, svv = (ld(v) for v in moments)
    vx, vy = suu - a * a / m, svv - b * b / m
    zz = np.asarray(z, dtype=np.float64)
    if not (vx > 0 and vy > 0):
        return np.full(zz.shape, np.nan)
    return ((zz.astype(ld) - a * b / m) / np.sqrt(vx * vy)).astype(np.float64)


def _check_alternative(alternative) -> str:
    if alternative not in ALTERNATIVES:
        raise ValueError(f"alternative must be one of {ALTERNATIVES}, not {alternative!r}")
    return alternative


def _check_permutations(count) -> int:
    if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or count < 0:
        raise ValueError(f"permutations must be an integer >= 0, not {count!r}")
    if count >= 2 ** 32 - 1:
        raise ValueError(f"permutations = {count}: fewer than 2^32 - 1")
    return int(count)


def _check_n(n: int) -> None:
    if n < 3:
        raise ValueError("need at least three rows for a Mantel test")


def run_mantel(ctx: engine.Context | None, src_x: _lib.Source, src_y: _lib.Source, perms: np.ndarray,
               alternative: str = "two-sided") -> Mantel:
    """dvs_mantel over the two sources with the checked permutations (uint32 [P, n]) -> Mantel"""
    ctx = ctx or engine.default_context()
    perms = np.ascontiguousarray(perms, dtype=np.uint32)
    n_perm = int(perms.shape[0])
    moments = np.zeros(6, dtype=np.float64)
    z = np.zeros(n_perm + 1, dtype=np.float64)
    info = _lib.MantelInfo()
    ctx.check(ctx._L.dvs_mantel(ctx._h, src_x, src_y, _lib.ptr(perms, C.c_uint32) if n_perm else None, n_perm,
                                _lib.ptr(moments, C.c_double), _lib.ptr(z, C.c_double), C.byref(info)))
    r = mantel_statistics(src_x.n, moments, z)
    count = {"two-sided": info.n_abs_ge, "greater": info.n_ge, "less": info.n_le}[alternative]
    p_value = (1.0 + int(count)) / (1.0 + n_perm) if n_perm and not np.isnan(r[0]) else float("nan")
    return Mantel(float(r[0]), p_value, alternative, int(src_x.n), n_perm, z, r[1:].copy(), int(info.n_ge), int(info.n_le),
                  int(info.n_abs_ge), moments, int(info.passes))


def _side(side):
    """a `distance.DeviceSide` or a caller's matrix -> (source, n, its context or None, wait)"""
    if isinstance(side, distance.DeviceSide):
        return side._source(), side.n, side.ctx, lambda: None
    src, n, wait = cluster._caller_matrix(side)
    return src, n, None, wait


def mantel(x, y, *, permutations: int = 999, seed=None, alternative: str = "two-sided", strata=None,
           ctx: engine.Context | None = None) -> Mantel:
    """The Mantel test (`Mantel`) of two sides over the same n >= 3 items.  x, y: each a `distance.DeviceSide`, or a
    square matrix as `cluster.permanova` takes it -- anything np.asarray(m, float64) takes, or a square, contiguous
    float64 torch tensor on the context's device, which is waited for and only read; only the cells above the diagonal
    count, and each must be finite and >= 0.  permutations: how many are drawn (0: r alone, p_value nan); seed, strata:
    as the module's `permutations`; alternative: "two-sided" (the default, as scikit-bio), "greater" or "less".
    ValueError before any device work for a bad alternative, negative permutations, sides of different n, n < 3,
    strata of the wrong length, or two sides on different contexts (ctx: for two matrices; it must be the sides' own
    otherwise)."""
    alternative = _check_alternative(alternative)
    count = _check_permutations(permutations)
    (sx, nx, cx, wait_x), (sy, ny, cy, wait_y) = _side(x), _side(y)
    if nx != ny:
        raise ValueError(f"a side of {nx} rows against one of {ny} rows")
    _check_n(nx)
    for own in (cx, cy):
        if own is not None and ctx is not None and own is not ctx:
            raise ValueError("the two sides of a Mantel test must be on one context")
        ctx = own if own is not None else ctx
    perms = _draw(nx, count, seed, strata)
    wait_x()
    wait_y()
    return run_mantel(ctx, sx, sy, perms, alternative)


def _check_mode(mode, which: str) -> dict:
    """a mode dictionary -> its six values, the missing ones at their defaults, checked by distance.check_mode_args"""
    if not hasattr(mode, "keys") or "distance_mode" not in mode or "k" not in mode:
        raise ValueError(f"{which}: a dictionary with 'distance_mode' and 'k' (and any of {_MODE_KEYS[2:]})")
    unknown = [key for key in mode if key not in _MODE_KEYS]
    if unknown:
        raise ValueError(f"{which}: unknown key {unknown[0]!r}")
    full = {"sketch_size": None, "num_states": 4, "mash_canonical": False, "canonical": False, **mode}
    distance.check_mode_args(full["distance_mode"], full["sketch_size"], full["mash_canonical"], full["canonical"])
    return full


def _mode_side(seqs, mode: dict, ctx) -> "distance.DeviceSide":
    args = distance.mode_args(mode["distance_mode"], mode["k"], mode["sketch_size"], mode["num_states"], mode["mash_canonical"])
    return distance.device_side(seqs, mode["distance_mode"], *args, ctx=ctx, canonical=mode["canonical"])


def of_sequences(seqs, x_mode: dict, y_mode: dict, *, permutations: int = 999, seed=None, alternative: str = "two-sided",
                 strata=None, ctx: engine.Context | None = None) -> Mantel:
    """The Mantel test between two distances of ONE collection of sequences (uint8 arrays of alphabet indices): do,
    say, the jsd and the mash distances tell the same story?  Each mode is {"distance_mode", "k", "sketch_size",
    "num_states", "mash_canonical", "canonical"} (the last four optional), checked by distance.check_mode_args.  Both
    sides are built in HBM, neither matrix crosses PCIe, the permutations are drawn once; the other arguments and their
    checks, before any device work, as `mantel`."""
    x_mode, y_mode = _check_mode(x_mode, "x_mode"), _check_mode(y_mode, "y_mode")
    alternative = _check_alternative(alternative)
    count = _check_permutations(permutations)
    n = len(seqs)
    _check_n(n)
    perms = _draw(n, count, seed, strata)
    ctx = ctx or engine.default_context()
    with _mode_side(seqs, x_mode, ctx) as side_x:  # (closed if the second fails, and both on the way out)
        with _mode_side(seqs, y_mode, ctx) as side_y:
            return run_mantel(ctx, side_x._source(), side_y._source(), perms, alternative)


@apps._define_app
class dvs_mantel(apps._DistanceApp):
    """Do two k-mer distances of a collection agree (beyond the reference, which has no such app)?  The Mantel test
    between the distances of x_mode and of y_mode, each {"distance_mode", "k", "sketch_size", "mash_canonical_kmers",
    "canonical"} with the checks of `dvs_ctree`; permutations, seed and alternative as `diverseseq_amd.mantel.mantel`.
    `main(seqs)` returns {"r", "p_value", "alternative", "permutations", "n"}.  Not registered as an entry point."""

    def __init__(self, x_mode: dict, y_mode: dict, *, moltype: str = "dna", permutations: int = 999, seed=None,
                 alternative: str = "two-sided") -> None:
        self._modes = []
        for which, mode in (("x_mode", x_mode), ("y_mode", y_mode)):
            if not hasattr(mode, "keys") or "distance_mode" not in mode:
                raise ValueError(f"{which}: a dictionary with 'distance_mode'")
            unknown = [key for key in mode if key not in ("distance_mode", "k", "sketch_size", "mash_canonical_kmers", "canonical")]
            if unknown:
                raise ValueError(f"{which}: unknown key {unknown[0]!r}")
            distance_mode, canonical = mode["distance_mode"], bool(mode.get("canonical", False))
            sketch_size, mash_canonical = self._check_mode(distance_mode, mode.get("sketch_size", 3_000), moltype,
                                                           mode.get("mash_canonical_kmers"), canonical=canonical)
            self._modes.append({"distance_mode": distance_mode, "k": mode.get("k", 12), "sketch_size": sketch_size,
                                "num_states": apps._num_states(moltype), "mash_canonical": mash_canonical,
                                "canonical": canonical})
        self._moltype = moltype
        self._permutations, self._seed = _check_permutations(permutations), seed
        self._alternative = _check_alternative(alternative)

    def main(self, seqs):
        names, arrays = apps._as_arrays(seqs, self._moltype)
        fit = of_sequences(arrays, *self._modes, permutations=self._permutations, seed=self._seed,
                           alternative=self._alternative)
        return {"r": fit.r, "p_value": fit.p_value, "alternative": fit.alternative, "permutations": fit.permutations,
                "n": fit.n}
