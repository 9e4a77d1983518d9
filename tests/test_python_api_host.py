"""The public surface of the Python layer -- every public name of diverseseq_amd.distance, .cluster, .apps and .engine
with its signature or fields, and the public attributes of distance.DeviceSide and distance.Sketches -- held to
tests/golden/python_api.json, which tests/golden/gen_python_api.py recorded from the commit before distance.py became
a package.  What that change meant to alter is written here, name by name; nothing else may differ.  No GPU."""
import json
import pathlib
import runpy

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"

# the four base classes that each held the operations of one feature: `DeviceSide` defines every operation itself
REMOVED = ("distance.GroupOps", "distance.MedoidOps", "distance.OrdinationOps", "distance.SpanningOps")

# the one property through which `Sketches` forwards, and the operations whose C call had no function of its own name:
# every operation has one `run_<op>` now
ADDED = {
    "distance.Sketches.side": {"kind": "property"},
    **{f"distance.run_{op}": "callable" for op in ("distances", "cross_distances", "nearest", "cluster_scores", "cophenet",
                                                    "maxmin", "within", "threshold_clusters", "pcoa_project")},
}

# one convention for the C-call layer, run_<op>(ctx, src, the checked arguments...): the six that were public lose
# their separate `n`, which is the source's own
RESIGNED = {
    "distance.run_linkage": ("(ctx: 'engine.Context | None', n: 'int', src: '_lib.Source', code: 'int', too_few: 'str' = "
                             "'need at least two sequences to build a tree') -> 'np.ndarray'",
                             "(ctx: 'engine.Context | None', src: '_lib.Source', code: 'int', too_few: 'str' = "
                             "'need at least two sequences to build a tree') -> 'np.ndarray'"),
    "distance.run_nj": ("(ctx: 'engine.Context | None', n: 'int', src: '_lib.Source') -> 'NJTree'",
                        "(ctx: 'engine.Context | None', src: '_lib.Source') -> 'NJTree'"),
    "distance.run_pcoa": ("(ctx: 'engine.Context | None', n: 'int', src: '_lib.Source', n_axes: 'int', tol: 'float', "
                          "max_basis: 'int', strict: 'bool' = True) -> 'PCoA'",
                          "(ctx: 'engine.Context | None', src: '_lib.Source', n_axes: 'int', tol: 'float', "
                          "max_basis: 'int', strict: 'bool' = True) -> 'PCoA'"),
    "distance.run_kmedoids": ("(ctx: 'engine.Context | None', n: 'int', src: '_lib.Source', k: 'int', rows: 'np.ndarray | None', "
                              "max_swaps: 'int') -> 'KMedoids'",
                              "(ctx: 'engine.Context | None', src: '_lib.Source', k: 'int', rows: 'np.ndarray | None', "
                              "max_swaps: 'int') -> 'KMedoids'"),
    "distance.run_mst": ("(ctx: 'engine.Context | None', n: 'int', src: '_lib.Source | None', core: 'np.ndarray | None' = None) "
                         "-> 'MST'",
                         "(ctx: 'engine.Context | None', src: '_lib.Source', core: 'np.ndarray | None' = None) -> 'MST'"),
    "distance.run_permanova": ("(ctx: 'engine.Context | None', n: 'int', src: '_lib.Source', labels: 'np.ndarray', "
                               "n_groups: 'int', perms: 'np.ndarray') -> 'PERMANOVA'",
                               "(ctx: 'engine.Context | None', src: '_lib.Source', labels: 'np.ndarray', n_groups: 'int', "
                               "perms: 'np.ndarray') -> 'PERMANOVA'"),
}


def current_inventory() -> dict:
    return runpy.run_path(str(GOLDEN / "gen_python_api.py"))["inventory"]()  # (the generator's own inventory)


def test_the_public_surface_is_the_recorded_one_but_for_the_written_differences():
    recorded = json.loads((GOLDEN / "python_api.json").read_text())["names"]
    got = current_inventory()
    assert set(REMOVED) <= set(recorded) and not set(REMOVED) & set(got)
    assert not set(ADDED) & set(recorded)
    for name, want in ADDED.items():
        assert name in got, name
        assert got[name] == want if isinstance(want, dict) else got[name]["kind"] == want, (name, got[name])
        assert name.count(".") == 2 or got[name]["signature"].startswith("(ctx: 'engine.Context | None', "), (name, got[name])
    for name, (before, after) in RESIGNED.items():
        assert recorded[name] == {"kind": "callable", "signature": before}, (name, recorded[name])
        assert got[name] == {"kind": "callable", "signature": after}, (name, got[name])
    rest = lambda names: {k: v for k, v in names.items() if k not in REMOVED and k not in ADDED and k not in RESIGNED}  # noqa: E731
    want, have = rest(recorded), rest(got)
    assert sorted(have) == sorted(want), sorted(set(have) ^ set(want))
    differing = {k: (want[k], have[k]) for k in want if want[k] != have[k]}
    assert not differing, differing


def test_the_packages_public_names_are_counted():
    """dir() of the package: the recorded names, less the four classes, plus the nine `run_` functions"""
    from diverseseq_amd import distance

    recorded = json.loads((GOLDEN / "python_api.json").read_text())["names"]
    before = {k.split(".")[1] for k in recorded if k.startswith("distance.") and k.count(".") == 1}
    now = {n for n in dir(distance) if not n.startswith("_")}
    assert len(now) == len(before) - 4 + 9
    assert before - now == {k.split(".")[1] for k in REMOVED}
    assert now - before == {k.split(".")[1] for k in ADDED if k.count(".") == 1}


def test_the_layers_depend_downwards_only():
    """_results <- _calls <- _sides <- _sequences: a module imports only from those before it, and ctypes stays out of
    the first and the last"""
    import ast

    pkg = pathlib.Path(__file__).resolve().parent.parent / "diverseseq_amd" / "distance"
    order = ["_results", "_calls", "_sides", "_sequences"]
    for i, name in enumerate(order):
        tree = ast.parse((pkg / f"{name}.py").read_text())
        siblings = {node.module for node in ast.walk(tree)
                    if isinstance(node, ast.ImportFrom) and node.level == 1 and node.module}
        assert siblings <= set(order[:i]), (name, siblings)
        imported = {a.name for node in ast.walk(tree) if isinstance(node, ast.Import) for a in node.names}
        assert ("ctypes" in imported) == (name in ("_calls", "_sides")), (name, imported)
