"""The reference's app surface over the HIP path: `dvs_nmost`, `dvs_max`, `dvs_delta_jsd`
(diverse_seq/records.py:254-429) and `dvs_ctree` / `dvs_par_ctree` (diverse_seq/cluster.py:98-188,
399-495), the five names its pyproject registers under the `cogent3.app` entry-point group
(pyproject.toml:89-94; `pyproject.toml` here registers the same five); and `dvs_dist`
(diverse_seq/distance.py:21-116), the distance-matrix app the reference defines without registering it.
`dvs_ctree`, `dvs_par_ctree` and `dvs_dist` also take distance_mode="jsd", the pairwise Jensen-Shannon
divergence of k-mer frequencies (diverseseq_amd.distance.jsd_distances).  `dvs_nearest`, beyond the reference: the
nearest of a fixed set of reference sequences for every query (diverseseq_amd.distance.nearest); and `dvs_clusters`:
the tree, its flat clusters at a cut, one representative per cluster and the silhouettes
(diverseseq_amd.cluster.ctree_clusters); and `dvs_njtree`: the neighbour-joining tree of the same distances, with branch
lengths (diverseseq_amd.cluster.nj_tree); and `dvs_maxmin`: farthest-first selection of representatives by distance,
a diverse panel or a dereplication (diverseseq_amd.distance.maxmin); and `dvs_pcoa`: the principal coordinates of the
same distances, the picture that goes with the trees and the clusters (diverseseq_amd.cluster.ordinate); and
`dvs_kmedoids`: the n sequences that represent a collection best, k-medoids over the same distances
(diverseseq_amd.cluster.representatives); and `dvs_permanova`: whether a grouping of the sequences explains those
distances, PERMANOVA (diverseseq_amd.distance.permanova).

Constructor arguments, defaults, seeding (`numpy.random.default_rng(seed).shuffle` of the unique
ids) and error messages are the reference's.  cogent3 is OPTIONAL: when it is importable the classes
are wrapped with its `define_app` and take / return its sequence collections; without it (this
image) they are plain callables over `{name: sequence}` mappings -- str (IUPAC letters), bytes or
uint8 arrays of alphabet indices -- and return the selected mapping, (name, delta) pair or Newick
string.  Everything numeric goes through `diverseseq_amd._dvs`, i.e. the C ABI.
"""

from __future__ import annotations

import numpy as np

from . import _dvs as dvs
from . import cluster as _cluster
from . import distance as _distance

try:  # pragma: no cover - cogent3 is not in this image
    from cogent3.app.composable import define_app as _define_app
    from cogent3 import get_moltype as _get_moltype
    HAVE_COGENT3 = True
except Exception:  # noqa: BLE001
    HAVE_COGENT3 = False

    def _define_app(*a, **kw):
        def wrap(cls):
            cls.__call__ = lambda self, *args, **kwargs: self.main(*args, **kwargs)
            return cls
        return wrap if not (len(a) == 1 and isinstance(a[0], type)) else wrap(a[0])

__all__ = ["dvs_nmost", "dvs_max", "dvs_delta_jsd", "dvs_ctree", "dvs_par_ctree", "dvs_dist", "dvs_nearest",
           "dvs_clusters", "dvs_cophenet", "dvs_njtree", "dvs_maxmin", "dvs_dereplicate", "dvs_pcoa", "dvs_kmedoids", "dvs_mst",
           "dvs_permanova"]

# len(get_moltype(m).alphabet) of the reference (records.py:299, 415-416)
_NUM_STATES = {"dna": 4, "rna": 4, "protein": 20, "text": 26, "bytes": 256}
_ALPHABET = {"dna": "TCAG", "rna": "UCAG", "protein": "ACDEFGHIKLMNPQRSTVWY"}


def _num_states(moltype: str) -> int:
    if HAVE_COGENT3:  # pragma: no cover
        return len(_get_moltype(moltype).alphabet)
    try:
        return _NUM_STATES[moltype.lower()]
    except KeyError:
        raise ValueError(f"unknown moltype {moltype!r}") from None


def _check_canonical(canonical: bool, moltype: str, moltypes: str = "dna") -> None:
    """canonical count rows fold a k-mer with its reverse complement: nucleotides only (the message is the one the
    mash apps give for their canonical k-mers)"""
    if canonical and moltype not in ("dna", "rna"):
        raise ValueError(f"Canonical kmers only supported for {moltypes} sequences.")


def _encode(seq, moltype: str) -> bytes:
    """sequence -> alphabet indices, one byte per symbol (diverse_seq/util.py:32-45 str2arr); gaps and
    ambiguity codes become indices >= num_states and invalidate the k-mers that contain them"""
    if isinstance(seq, (bytes, bytearray, memoryview)):
        return bytes(seq)
    if isinstance(seq, np.ndarray):
        return np.ascontiguousarray(seq, dtype=np.uint8).tobytes()
    text = str(seq).replace("-", "").replace("?", "")  # degap (records.py: seqs.degap())
    canon = _ALPHABET.get(moltype.lower())
    if canon is None:
        raise ValueError(f"cannot encode text for moltype {moltype!r} without cogent3")
    lut = np.full(256, len(canon), dtype=np.uint8)
    for i, ch in enumerate(canon):
        lut[ord(ch)] = lut[ord(ch.lower())] = i
    if moltype.lower() == "dna":
        lut[ord("U")] = lut[ord("u")] = 0
    return lut[np.frombuffer(text.encode("ascii", "replace"), dtype=np.uint8)].tobytes()


def _as_mapping(seqs, moltype: str):
    """(names, {name: index bytes}, taker) for a cogent3 collection or a plain mapping"""
    if HAVE_COGENT3 and hasattr(seqs, "take_seqs"):  # pragma: no cover
        degapped = seqs.degap()
        data = {s.name: np.array(s).tobytes() for s in degapped.seqs}
        return list(data), data, seqs.take_seqs
    data = {str(n): _encode(s, moltype) for n, s in dict(seqs).items()}

    def take(names):  # (the store's names are str(n): compare on those, whatever the mapping's keys are)
        sel = {str(n) for n in names}
        return {n: seqs[n] for n in seqs if str(n) in sel}

    return list(data), data, take


def _populate_inmem_zstore(data: dict):
    """diverse_seq/util.py:176-184"""
    zstore = dvs.make_zarr_store()
    for name, arr in data.items():
        zstore.write(name, arr)
    return zstore


def _as_arrays(seqs, moltype: str):
    """(names, the sequences as uint8 arrays of alphabet indices, in that order) of what `_as_mapping` takes"""
    names, data, _ = _as_mapping(seqs, moltype)
    return names, [np.frombuffer(data[n], dtype=np.uint8) for n in names]


class _DistanceApp:
    """what the apps over a distance mode share: the constructor checks of ClusterTreeBase.__init__
    (cluster.py:36-95) and the attributes they leave"""

    @staticmethod
    def _check_mode(distance_mode, sketch_size, moltype, mash_canonical_kmers, *, moltypes: str = "dna",
                    keep_sketch_size: bool = False, canonical: bool = False):
        """-> (sketch_size, mash_canonical_kmers) as the app keeps them; `moltypes`: how the message names the
        molecule types that have canonical k-mers; the sketch size means nothing to the euclidean and jsd modes
        (cli.py:546-560) and is dropped for them unless keep_sketch_size; canonical: the count rows of the jsd and
        euclidean modes folded onto the canonical k-mer bins (dna / rna only; mash has mash_canonical_kmers)"""
        if mash_canonical_kmers is None:
            mash_canonical_kmers = False
        if distance_mode not in _distance.MODES:
            raise ValueError(f"Unexpected distance {distance_mode!r}.")
        if moltype not in ("dna", "rna") and mash_canonical_kmers:
            raise ValueError(f"Canonical kmers only supported for {moltypes} sequences.")
        _check_canonical(canonical, moltype, moltypes)
        if distance_mode == "mash" and canonical:
            raise ValueError(_distance.CANONICAL_MASH)
        if distance_mode == "mash" and sketch_size is None:
            raise ValueError("Expected sketch size for mash distance measure.")
        if distance_mode != "mash" and not keep_sketch_size:
            sketch_size = None
        return sketch_size, mash_canonical_kmers

    def _keep_mode(self, distance_mode, k, sketch_size, moltype, mash_canonical_kmers, canonical: bool = False) -> None:
        self._moltype = moltype
        self._k = k
        self._num_states = _num_states(moltype)
        self._sketch_size = sketch_size
        self._distance_mode = distance_mode
        self._mash_canonical = mash_canonical_kmers
        self._canonical = bool(canonical)

    def _mode_kwargs(self) -> dict:
        """the keyword arguments of the diverseseq_amd.cluster functions over sequences"""
        return dict(k=self._k, sketch_size=self._sketch_size, distance_mode=self._distance_mode,
                    mash_canonical_kmers=self._mash_canonical, num_states=self._num_states, canonical=self._canonical)


@_define_app
class dvs_max:
    """select the maximally divergent seqs from a sequence collection (records.py:254-321)"""

    def __init__(self, min_size: int = 5, max_size: int = 30, stat: str = "stdev", moltype: str = "dna",
                 include: list[str] | str | None = None, k: int = 6, seed: int | None = None,
                 canonical: bool = False) -> None:
        _check_canonical(canonical, moltype)
        self._canonical = bool(canonical)
        self._k = k
        self._moltype = moltype
        self._num_states = _num_states(moltype)
        self._min_size = min_size
        self._max_size = max_size
        self._stat = stat
        self._rng = np.random.default_rng(seed)
        self._include = [include] if isinstance(include, str) else include

    def main(self, seqs):
        _, data, take = _as_mapping(seqs, self._moltype)
        zstore = _populate_inmem_zstore(data)
        seqids = list(zstore.unique_seqids)
        self._rng.shuffle(seqids)
        result = dvs.max_divergent(zstore, min_size=self._min_size, max_size=self._max_size, k=self._k,
                                   num_states=self._num_states, seqids=seqids, stat=self._stat,
                                   canonical=self._canonical)
        return take(set(result.record_names) | set(self._include or []))


@_define_app
class dvs_nmost:
    """select the n-most diverse seqs from a sequence collection (records.py:324-373)"""

    def __init__(self, n: int = 10, moltype: str = "dna", include: list[str] | str | None = None, k: int = 6,
                 seed: int | None = None, canonical: bool = False) -> None:
        _check_canonical(canonical, moltype)
        self._canonical = bool(canonical)
        self._k = k
        self._n = n
        self._moltype = moltype
        self._rng = np.random.default_rng(seed)
        self._include = [include] if isinstance(include, str) else include

    def main(self, seqs):
        _, data, take = _as_mapping(seqs, self._moltype)
        zstore = _populate_inmem_zstore(data)
        seqids = list(zstore.unique_seqids)
        self._rng.shuffle(seqids)
        result = dvs.nmost_divergent(zstore, n=self._n, k=self._k, seqids=seqids,  # (num_states left at 4, :371)
                                     canonical=self._canonical)
        return take(set(result.record_names) | set(self._include or []))


@_define_app
class dvs_delta_jsd:
    """delta JSD of a sequence against a fixed reference set (records.py:376-429)"""

    def __init__(self, seqs, moltype: str = "dna", k: int = 6, canonical: bool = False) -> None:
        _check_canonical(canonical, moltype)
        _, data, _ = _as_mapping(seqs, moltype)
        zero_len = ", ".join(n for n, s in data.items() if len(s) == 0)
        if zero_len:
            raise ValueError(f"cannot compute delta_jsd with zero-length sequences: {zero_len}")
        self.moltype = moltype
        self._sr = dvs.get_delta_jsd_calculator(list(data.items()), k, _num_states(moltype), canonical=bool(canonical))

    def main(self, seq):
        if HAVE_COGENT3 and hasattr(seq, "moltype"):  # pragma: no cover
            if seq.moltype.name != self.moltype:
                seq = seq.to_moltype(self.moltype)
            seq = seq.degap()
            name, arr = seq.name, np.array(seq).tobytes()
        else:
            name, raw = seq  # (name, sequence)
            arr = _encode(raw, self.moltype)
        if len(arr) == 0:
            return name, float("nan")
        return name, self._sr.delta_jsd(name, arr)


class _ClusterTreeBase(_DistanceApp):
    """argument checks of ClusterTreeBase.__init__ (cluster.py:36-95)"""

    def __init__(self, *, k: int = 12, sketch_size: int | None = 3_000, moltype: str = "dna",
                 distance_mode: str = "mash", mash_canonical_kmers: bool | None = None,
                 show_progress: bool = False, canonical: bool = False) -> None:
        sketch_size, mash_canonical_kmers = self._check_mode(distance_mode, sketch_size, moltype, mash_canonical_kmers,
                                                             moltypes="dna/rna", canonical=canonical)
        self._keep_mode(distance_mode, k, sketch_size, moltype, mash_canonical_kmers, canonical)
        self._progress = show_progress

    def main(self, seqs):
        names, arrays = _as_arrays(seqs, self._moltype)
        newick = _cluster.ctree(dict(zip(names, arrays)), **self._mode_kwargs())
        if HAVE_COGENT3:  # pragma: no cover
            from cogent3 import make_tree

            return make_tree(newick, underscore_unmunge=True)
        return newick


@_define_app
class dvs_ctree(_ClusterTreeBase):
    """Create a cluster tree from kmer distances (cluster.py:98-188)."""

    def __init__(self, *, k: int = 12, sketch_size: int | None = 3_000, moltype: str = "dna",
                 distance_mode: str = "mash", mash_canonical_kmers: bool | None = None,
                 show_progress: bool = False, canonical: bool = False) -> None:
        super().__init__(k=k, sketch_size=sketch_size, moltype=moltype, distance_mode=distance_mode,
                         mash_canonical_kmers=mash_canonical_kmers, show_progress=show_progress, canonical=canonical)


@_define_app
class dvs_njtree(_ClusterTreeBase):
    """Create a neighbour-joining tree from kmer distances (beyond the reference, which has no such app): the tree
    of additive distances -- unrooted, with branch lengths, no molecular clock assumed -- where `dvs_ctree` gives the
    average-linkage tree.  Arguments and their checks as `dvs_ctree`; `main(seqs)` returns the Newick string with
    branch lengths, or cogent3's tree when cogent3 is importable.  Three sequences at least."""

    def __init__(self, *, k: int = 12, sketch_size: int | None = 3_000, moltype: str = "dna",
                 distance_mode: str = "mash", mash_canonical_kmers: bool | None = None,
                 show_progress: bool = False, canonical: bool = False) -> None:
        super().__init__(k=k, sketch_size=sketch_size, moltype=moltype, distance_mode=distance_mode,
                         mash_canonical_kmers=mash_canonical_kmers, show_progress=show_progress, canonical=canonical)

    def main(self, seqs):
        names, arrays = _as_arrays(seqs, self._moltype)
        newick, _ = _cluster.nj_tree(dict(zip(names, arrays)), **self._mode_kwargs())
        if HAVE_COGENT3:  # pragma: no cover
            from cogent3 import make_tree

            return make_tree(newick, underscore_unmunge=True)
        return newick


@_define_app
class dvs_pcoa(_DistanceApp):
    """Principal coordinates (PCoA, classical MDS) of the k-mer distances of a collection (beyond the reference, which has
    no such app): the picture that goes with `dvs_ctree`, `dvs_njtree` and `dvs_clusters`.  The mode arguments and their
    checks as `dvs_ctree`; n_axes: the axes wanted (1 .. 64, and fewer than the sequences).  `main(seqs)` returns
    {"names": [...], "coordinates": float64 [n, n_axes] (row i belongs to names[i]), "proportion": float64 [n_axes], the
    share of the total inertia on each axis, "eigenvalues": float64 [n_axes]}."""

    def __init__(self, n_axes: int = 3, *, k: int = 12, sketch_size: int | None = 3_000, moltype: str = "dna",
                 distance_mode: str = "mash", mash_canonical_kmers: bool | None = None, canonical: bool = False) -> None:
        sketch_size, mash_canonical_kmers = self._check_mode(distance_mode, sketch_size, moltype, mash_canonical_kmers,
                                                             moltypes="dna/rna", canonical=canonical)
        if isinstance(n_axes, bool) or not isinstance(n_axes, (int, np.integer)) or not 1 <= n_axes <= _distance.PCOA_MAX_AXES:
            raise ValueError(f"n_axes must be an integer in 1 .. {_distance.PCOA_MAX_AXES}, not {n_axes!r}")
        self._n_axes = int(n_axes)
        self._keep_mode(distance_mode, k, sketch_size, moltype, mash_canonical_kmers, canonical)

    def main(self, seqs):
        names, arrays = _as_arrays(seqs, self._moltype)
        names, fit = _cluster.ordinate(dict(zip(names, arrays)), self._n_axes, **self._mode_kwargs())
        return {"names": names, "coordinates": fit.coordinates, "proportion": fit.proportion, "eigenvalues": fit.values}


@_define_app
class dvs_kmedoids(_DistanceApp):
    """The n sequences that represent a collection best (beyond the reference, which has no such app): k-medoids, the
    set whose members lie closest, in total, to everything else, by any distance of `dvs_dist`.  The mode arguments and
    their checks as `dvs_maxmin`; init: "build" (PAM's BUILD) or "maxmin" (farthest-first picks as the start);
    max_swaps: the most exchanges made (0: the initial set as it is).  `main(seqs)` returns {"representatives": [names,
    slot order], "sizes": [the size of each one's cluster], "representative": {name: its representative's name},
    "distance": {name: float}, "total_distance": float, "converged": bool}."""

    def __init__(self, n: int, distance_mode: str = "mash", *, k: int = 12, sketch_size: int | None = 3_000,
                 moltype: str = "dna", mash_canonical_kmers: bool | None = None, init: str = "build", max_swaps: int = 300,
                 canonical: bool = False) -> None:
        sketch_size, mash_canonical_kmers = self._check_mode(distance_mode, sketch_size, moltype, mash_canonical_kmers,
                                                             canonical=canonical)
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= _distance.KMEDOIDS_MAX_K:
            raise ValueError(f"n must be an integer in 1 .. {_distance.KMEDOIDS_MAX_K}, not {n!r}")
        if init not in ("build", "maxmin"):
            raise ValueError(f"init must be 'build' or 'maxmin', not {init!r}")
        if (isinstance(max_swaps, bool) or not isinstance(max_swaps, (int, np.integer))
                or not 0 <= max_swaps <= _distance.KMEDOIDS_MAX_SWAPS):
            raise ValueError(f"max_swaps must be an integer in 0 .. {_distance.KMEDOIDS_MAX_SWAPS}, not {max_swaps!r}")
        self._n, self._init, self._max_swaps = int(n), init, int(max_swaps)
        self._keep_mode(distance_mode, k, sketch_size, moltype, mash_canonical_kmers, canonical)

    def main(self, seqs):
        names, arrays = _as_arrays(seqs, self._moltype)
        if not names:
            raise ValueError("no sequences")
        reps, sizes, labels, fit = _cluster.representatives(dict(zip(names, arrays)), self._n, init=self._init,
                                                            max_swaps=self._max_swaps, **self._mode_kwargs())
        return {"representatives": reps, "sizes": [int(v) for v in sizes],
                "representative": {name: reps[l] for name, l in zip(names, labels.tolist())},
                "distance": {name: float(d) for name, d in zip(names, fit.dist)},
                "total_distance": float(fit.td[-1]), "converged": bool(fit.stop)}


@_define_app
class dvs_permanova(_DistanceApp):
    """Does a grouping of the sequences explain their distances (beyond the reference, which has no such app)?
    PERMANOVA, the test that goes with `dvs_pcoa`, by any distance of `dvs_dist`.  grouping: {name: group}, any
    hashables, with an entry for every sequence the app is given; permutations, seed and strata ({name: block}) as
    `diverseseq_amd.distance.permanova`; the mode arguments and their checks as `dvs_maxmin`.  `main(seqs)` returns {"f",
    "p_value", "r2", "ss_total", "ss_within", "ss_among": floats, "groups": [the groups in the order of their first
    sequence], "group_sizes": {group: int}, "group_ss": {group: float}, "permutations": int}."""

    def __init__(self, grouping: dict, distance_mode: str = "mash", *, k: int = 12, sketch_size: int | None = 3_000,
                 moltype: str = "dna", mash_canonical_kmers: bool | None = None, permutations: int = 999, seed=None,
                 strata: dict | None = None, canonical: bool = False) -> None:
        sketch_size, mash_canonical_kmers = self._check_mode(distance_mode, sketch_size, moltype, mash_canonical_kmers,
                                                             canonical=canonical)
        if not hasattr(grouping, "keys") or (strata is not None and not hasattr(strata, "keys")):
            raise ValueError("grouping (and strata) must map the names of the sequences to their groups")
        if isinstance(permutations, bool) or not isinstance(permutations, (int, np.integer)) or permutations < 0:
            raise ValueError(f"permutations must be an integer >= 0, not {permutations!r}")
        self._grouping = {str(n): g for n, g in grouping.items()}
        self._strata = None if strata is None else {str(n): g for n, g in strata.items()}
        self._permutations, self._seed = int(permutations), seed
        self._keep_mode(distance_mode, k, sketch_size, moltype, mash_canonical_kmers, canonical)

    def main(self, seqs):
        names, arrays = _as_arrays(seqs, self._moltype)
        missing = [n for n in names if n not in self._grouping or (self._strata is not None and n not in self._strata)]
        if missing:
            raise ValueError(f"no group for sequence {missing[0]!r}")
        groups = [self._grouping[n] for n in names]
        strata = None if self._strata is None else [self._strata[n] for n in names]
        fit = _distance.permanova(arrays, groups, self._distance_mode, k=self._k, sketch_size=self._sketch_size,
                                  num_states=self._num_states, mash_canonical=self._mash_canonical,
                                  permutations=self._permutations, seed=self._seed, strata=strata,
                                  canonical=self._canonical)
        order = list(dict.fromkeys(groups))
        return {"f": fit.f, "p_value": fit.p_value, "r2": fit.r2, "ss_total": fit.ss_total, "ss_within": fit.ss_within,
                "ss_among": fit.ss_among, "groups": order,
                "group_sizes": {g: int(v) for g, v in zip(order, fit.group_sizes)},
                "group_ss": {g: float(v) for g, v in zip(order, fit.group_ss)}, "permutations": fit.permutations}


@_define_app
class dvs_par_ctree(_ClusterTreeBase):
    """The same tree with the reference's worker-process knobs accepted (cluster.py:399-495).  The
    reference spreads sketches and strided distance rows over `max_workers` processes; here one GPU does
    both stages (several GPUs: diverseseq_amd.parallel.mash_distances_sharded), so `max_workers` and
    `parallel` only keep the signature."""

    def __init__(self, *, k: int = 12, sketch_size: int | None = 3_000, moltype: str = "dna",
                 distance_mode: str = "mash", mash_canonical_kmers: bool | None = None,
                 show_progress: bool = False, max_workers: int | None = None, parallel: bool = True,
                 canonical: bool = False) -> None:
        super().__init__(k=k, sketch_size=sketch_size, moltype=moltype, distance_mode=distance_mode,
                         mash_canonical_kmers=mash_canonical_kmers, show_progress=show_progress, canonical=canonical)
        self._max_workers = max_workers
        self._parallel = parallel


@_define_app
class dvs_dist(_DistanceApp):
    """Calculate pairwise kmer-based distances between sequences (diverse_seq/distance.py:21-116): the mash
    distance, the euclidean distance between k-mer frequencies or, beyond the reference, their Jensen-Shannon
    divergence ("jsd").  Returns cogent3's DistanceMatrix when cogent3 is importable, else (names, float64 [n, n])
    with the names in input order."""

    def __init__(self, distance_mode: str = "mash", *, k: int = 12, sketch_size: int | None = 3_000,
                 moltype: str = "dna", mash_canonical_kmers: bool | None = None, show_progress: bool = False,
                 canonical: bool = False) -> None:
        sketch_size, mash_canonical_kmers = self._check_mode(distance_mode, sketch_size, moltype, mash_canonical_kmers,
                                                             keep_sketch_size=True, canonical=canonical)
        self._keep_mode(distance_mode, k, sketch_size, moltype, mash_canonical_kmers, canonical)
        self._show_progress = show_progress

    def main(self, seqs):
        names, arrays = _as_arrays(seqs, self._moltype)
        dists = _distance.MODES[self._distance_mode][0](arrays, *_distance.mode_args(
            self._distance_mode, self._k, self._sketch_size, self._num_states, self._mash_canonical),
            **({"canonical": True} if self._canonical else {}))
        if HAVE_COGENT3:  # pragma: no cover
            from cogent3.evolve.fast_distance import DistanceMatrix

            return DistanceMatrix.from_array_names(matrix=dists, names=names)
        return names, dists


@_define_app
class dvs_nearest(_DistanceApp):
    """The nearest of a fixed set of reference sequences for every query, by any distance of `dvs_dist` (beyond the
    reference, which has no such app).  The references are taken, encoded and sketched (mash) or counted (euclidean,
    jsd) once, here; `main(seqs)` returns {query name: [(reference name, distance), ...]}, nearest first, a tie to the
    reference that came first; a reference at NaN distance (jsd, euclidean: no valid k-mer on either side) is not
    listed, so a list may be shorter than n_nearest."""

    def __init__(self, refs, n_nearest: int = 1, distance_mode: str = "mash", *, k: int = 12,
                 sketch_size: int | None = 3_000, moltype: str = "dna", mash_canonical_kmers: bool | None = None,
                 canonical: bool = False) -> None:
        sketch_size, mash_canonical_kmers = self._check_mode(distance_mode, sketch_size, moltype, mash_canonical_kmers,
                                                             keep_sketch_size=True, canonical=canonical)
        names, arrays = _as_arrays(refs, moltype)
        self._n_nearest = _distance.check_n_nearest(n_nearest, len(names))
        self._keep_mode(distance_mode, k, sketch_size, moltype, mash_canonical_kmers, canonical)
        self._ref_names = names
        self._mode_args = _distance.mode_args(distance_mode, k, sketch_size, self._num_states, mash_canonical_kmers)
        # (kept for the life of the app: the handle's finaliser frees it)
        self._refs = _distance.device_side(arrays, distance_mode, *self._mode_args, canonical=self._canonical)

    def main(self, seqs):
        names, arrays = _as_arrays(seqs, self._moltype)
        if not names:
            return {}
        with _distance.device_side(arrays, self._distance_mode, *self._mode_args, canonical=self._canonical) as q:
            idx, dist = q.nearest(self._refs, self._n_nearest)
        return {name: [(self._ref_names[j], float(d)) for j, d in zip(idx[i], dist[i]) if j >= 0]
                for i, name in enumerate(names)}


@_define_app
class dvs_clusters(_DistanceApp):
    """The flat clusters of the `dvs_ctree` tree at a cut, with one representative per cluster (beyond the reference,
    which has no such app): exactly one of n_clusters (scipy's fcluster "maxclust" partition: a cut never separates
    merges of equal height, so fewer clusters may come back) and height (its "distance" partition).  `main(seqs)`
    returns {"tree": Newick string, "clusters": {label: [names]}, "medoids": {label: name}, "silhouette": {name: float},
    "mean_silhouette": float}; labels count from 0 in the order the clusters first appear among the names; a medoid is
    the member with the least summed distance to the rest of its cluster (a cluster none of whose members has a
    number for that sum has no entry)."""

    def __init__(self, n_clusters: int | None = None, height: float | None = None, distance_mode: str = "mash", *,
                 k: int = 12, sketch_size: int | None = 3_000, moltype: str = "dna",
                 mash_canonical_kmers: bool | None = None, linkage: str = "average", canonical: bool = False) -> None:
        sketch_size, mash_canonical_kmers = self._check_mode(distance_mode, sketch_size, moltype, mash_canonical_kmers,
                                                             canonical=canonical)
        if (n_clusters is None) == (height is None):
            raise ValueError("dvs_clusters takes exactly one of n_clusters and height")
        if n_clusters is not None and (isinstance(n_clusters, bool) or not isinstance(n_clusters, (int, np.integer))
                                       or n_clusters < 1):
            raise ValueError(f"n_clusters must be an integer of 1 or more, not {n_clusters!r}")
        if height is not None and np.isnan(float(height)):
            raise ValueError("the height of a cut cannot be NaN")
        _distance.linkage_method_code(linkage)
        self._n_clusters, self._height = n_clusters, height
        self._keep_mode(distance_mode, k, sketch_size, moltype, mash_canonical_kmers, canonical)
        self._linkage = linkage

    def main(self, seqs):
        names, arrays = _as_arrays(seqs, self._moltype)
        newick, _, sc = _cluster.ctree_clusters(dict(zip(names, arrays)), n_clusters=self._n_clusters, height=self._height,
                                                linkage=self._linkage, **self._mode_kwargs())
        clusters: dict = {c: [] for c in range(sc.sizes.size)}
        for name, c in zip(names, sc.labels.tolist()):
            clusters[c].append(name)
        return {"tree": newick, "clusters": clusters,
                "medoids": {c: names[i] for c, i in enumerate(sc.medoids.tolist()) if i >= 0},
                "silhouette": {name: float(v) for name, v in zip(names, sc.silhouette)},
                "mean_silhouette": sc.mean_silhouette}


@_define_app
class dvs_dereplicate(_DistanceApp):
    """The groups of sequences joined by distances of `radius` or less, with one representative per group (beyond the
    reference, which has no such app): the connected components of "distance <= radius" -- the clusters `dvs_clusters`
    gives for single linkage and height=radius -- found without the N x N matrix and without a tree.  `main(seqs)`
    returns what `dvs_clusters` returns, {"tree": None, "clusters": {label: [names]}, "medoids": {label: name},
    "silhouette": {name: float}, "mean_silhouette": float}: labels count from 0 in the order the groups first appear
    among the names; a medoid, the group's representative, is the member with the least summed distance to the rest."""

    def __init__(self, radius: float, distance_mode: str = "mash", *, k: int = 12, sketch_size: int | None = 3_000,
                 moltype: str = "dna", mash_canonical_kmers: bool | None = None, canonical: bool = False) -> None:
        sketch_size, mash_canonical_kmers = self._check_mode(distance_mode, sketch_size, moltype, mash_canonical_kmers,
                                                             canonical=canonical)
        self._radius = _distance.check_radius(radius)
        self._keep_mode(distance_mode, k, sketch_size, moltype, mash_canonical_kmers, canonical)

    def main(self, seqs):
        names, arrays = _as_arrays(seqs, self._moltype)
        _, _, sc = _cluster.dereplicate(dict(zip(names, arrays)), self._radius, **self._mode_kwargs())
        clusters: dict = {c: [] for c in range(sc.sizes.size)}
        for name, c in zip(names, sc.labels.tolist()):
            clusters[c].append(name)
        return {"tree": None, "clusters": clusters,
                "medoids": {c: names[i] for c, i in enumerate(sc.medoids.tolist()) if i >= 0},
                "silhouette": {name: float(v) for name, v in zip(names, sc.silhouette)},
                "mean_silhouette": sc.mean_silhouette}


@_define_app
class dvs_cophenet(_DistanceApp):
    """How well the `dvs_ctree` tree of each linkage method represents the distances it was built from (beyond the
    reference, which has no such app): the cophenetic correlation, scipy's cophenet(Z, Y)[0].  `main(seqs)` returns
    {"best": method, "correlation": {method: float}, "tree": Newick string of the best method}; the best is the method
    of the largest correlation, a tie to the one named first, a NaN correlation (two sequences, equal distances) never
    taken -- with none to take, the first method."""

    def __init__(self, methods=("single", "complete", "average", "weighted", "ward"), distance_mode: str = "mash", *,
                 k: int = 12, sketch_size: int | None = 3_000, moltype: str = "dna",
                 mash_canonical_kmers: bool | None = None, canonical: bool = False) -> None:
        sketch_size, mash_canonical_kmers = self._check_mode(distance_mode, sketch_size, moltype, mash_canonical_kmers,
                                                             canonical=canonical)
        methods = [methods] if isinstance(methods, str) else list(methods)
        if not methods:
            raise ValueError("dvs_cophenet takes one linkage method at least")
        for method in methods:
            _distance.linkage_method_code(method)
        self._methods = methods
        self._keep_mode(distance_mode, k, sketch_size, moltype, mash_canonical_kmers, canonical)

    def main(self, seqs):
        names, arrays = _as_arrays(seqs, self._moltype)
        trees = _cluster.compare_linkages(dict(zip(names, arrays)), self._methods, **self._mode_kwargs())
        corr = {method: float(r) for method, (_, r) in trees.items()}
        best = self._methods[0]
        for method in self._methods:
            if corr[method] == corr[method] and not corr[best] >= corr[method]:
                best = method
        return {"best": best, "correlation": corr, "tree": _cluster.linkage_to_newick(names, trees[best][0])}


@_define_app
class dvs_maxmin(_DistanceApp):
    """Farthest-first (max-min) selection of representatives by any distance of `dvs_dist` (beyond the reference, whose
    selections are by delta-JSD): from the seeds on, the sequence farthest from those already taken, until `n` are
    taken or every sequence lies within `min_distance` of one -- a diverse panel, or one representative per group
    within min_distance.  At least one of n and min_distance; seeds: names taken first, in that order (None: the first
    sequence).  `main(seqs)` returns {"picks": [names in pick order], "radius": [a pick's distance to the nearest
    earlier pick, NaN for a seed], "representative": {name: the nearest pick's name, None for a sequence at NaN
    distance from the picks}, "distance": {name: float}, "cover": the largest distance of a sequence to its
    representative}."""

    def __init__(self, n: int | None = None, min_distance: float | None = None, distance_mode: str = "mash", *,
                 k: int = 12, sketch_size: int | None = 3_000, moltype: str = "dna",
                 mash_canonical_kmers: bool | None = None, seeds: list[str] | str | None = None,
                 canonical: bool = False) -> None:
        sketch_size, mash_canonical_kmers = self._check_mode(distance_mode, sketch_size, moltype, mash_canonical_kmers,
                                                             canonical=canonical)
        if n is None and min_distance is None:
            raise ValueError("dvs_maxmin takes n, min_distance or both")
        if n is not None and (isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1):
            raise ValueError(f"n must be an integer of 1 or more, not {n!r}")
        if min_distance is not None and np.isnan(float(min_distance)):
            raise ValueError("min_distance cannot be NaN")
        self._n, self._min_distance = n, min_distance
        self._seeds = [seeds] if isinstance(seeds, str) else None if seeds is None else [str(s) for s in seeds]
        if self._seeds is not None and not self._seeds:
            raise ValueError("dvs_maxmin takes one seed at least")
        self._keep_mode(distance_mode, k, sketch_size, moltype, mash_canonical_kmers, canonical)

    def main(self, seqs):
        names, arrays = _as_arrays(seqs, self._moltype)
        if not names:
            raise ValueError("no sequences")
        at = {name: i for i, name in enumerate(names)}
        missing = [s for s in self._seeds or [] if s not in at]
        if missing:
            raise ValueError(f"seed names not among the sequences: {missing}")
        seeds = [at[s] for s in self._seeds] if self._seeds else [0]
        r = _distance.maxmin(arrays, self._n, self._distance_mode, k=self._k, sketch_size=self._sketch_size,
                             num_states=self._num_states, mash_canonical=self._mash_canonical, seeds=seeds,
                             min_distance=self._min_distance, canonical=self._canonical)
        picked = [names[i] for i in r.picks.tolist()]
        return {"picks": picked, "radius": [float(v) for v in r.radius],
                "representative": {name: picked[o] if o >= 0 else None for name, o in zip(names, r.owner.tolist())},
                "distance": {name: float(d) for name, d in zip(names, r.dist)}, "cover": r.cover}


@_define_app
class dvs_mst(_DistanceApp):
    """The minimum spanning tree of the sequences by any distance of `dvs_dist` (beyond the reference, which has no
    such app): single linkage for collections whose N x N matrix could never exist -- the distances are recomputed strip
    by strip, once per Boruvka round.  `main(seqs)` returns the edges, [(name, name, distance)] in ascending (distance,
    position of the first name, position of the second) -- a minimum spanning network to draw --, or with tree=True the
    Newick string of the single-linkage tree, the merge heights of `dvs_ctree(linkage="single")`.  min_samples: the
    tree of the mutual-reachability distance max(d(a, b), core(a), core(b)) instead, core(a) the min_samples-th smallest
    distance from a, its own included: robust single linkage, the first half of HDBSCAN.  A sequence without a valid
    k-mer (jsd, euclidean) is joined by no edge; tree=True then raises ValueError."""

    def __init__(self, distance_mode: str = "mash", *, tree: bool = False, min_samples: int | None = None, k: int = 12,
                 sketch_size: int | None = 3_000, moltype: str = "dna", mash_canonical_kmers: bool | None = None,
                 canonical: bool = False) -> None:
        sketch_size, mash_canonical_kmers = self._check_mode(distance_mode, sketch_size, moltype, mash_canonical_kmers,
                                                             canonical=canonical)
        if not isinstance(tree, (bool, np.bool_)):
            raise ValueError(f"tree must be True or False, not {tree!r}")
        if min_samples is not None and (isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer))
                                        or not 1 <= min_samples <= _distance.MIN_SAMPLES_MAX):
            raise ValueError(f"min_samples must be an integer between 1 and {_distance.MIN_SAMPLES_MAX}, not {min_samples!r}")
        self._tree, self._min_samples = bool(tree), min_samples
        self._keep_mode(distance_mode, k, sketch_size, moltype, mash_canonical_kmers, canonical)

    def main(self, seqs):
        names, arrays = _as_arrays(seqs, self._moltype)
        if self._tree:
            return _cluster.mst_ctree(dict(zip(names, arrays)), min_samples=self._min_samples, **self._mode_kwargs())
        tree = _distance.mst(arrays, self._distance_mode, k=self._k, sketch_size=self._sketch_size,
                             num_states=self._num_states, mash_canonical=self._mash_canonical, canonical=self._canonical,
                             min_samples=self._min_samples)
        return _cluster.mst_to_edges(names, tree)
