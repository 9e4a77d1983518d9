"""bench.py's own launch logic, end to end on a box without a GPU: `python bench.py --gpus 2` with no launcher
around it must start two ranks itself (a parent that never touches the GPU -> `python -m
torch.distributed.run` as a child), run BOTH multi-GPU schemes and print ONE line with n_gpus == 2.  The
compute is the oracle-backed stand-in of tests/bench_cpu_engine.py under gloo (DVS_BENCH_TEST_ENGINE, a hook
that exists for this test only); what is under test is bench.py: self-launch, rank plumbing, the exchange
steps of diverseseq_amd.parallel, the max-over-ranks timing, the line's fields and the exit codes."""
import json
import os
import pathlib
import subprocess
import sys

import numpy as np

from conftest import ROOT

ARGS = ["--steps", "1", "--warmup", "0", "--nseq", "240", "--length", "200", "-k", "3", "-n", "5", "--no-cpu-baseline"]


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["DVS_BENCH_TEST_ENGINE"] = "bench_cpu_engine"
    env["PYTHONPATH"] = os.pathsep.join([str(ROOT), str(pathlib.Path(__file__).resolve().parent),
                                         env.get("PYTHONPATH", "")])
    return env


def test_bench_gpus_2_launches_two_ranks_itself():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--full", *ARGS], env=_env(),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2
    assert out["config"]["launched_by"].startswith("bench.py itself")
    assert out["engine_module"] == "bench_cpu_engine"
    # both schemes in one line, each with its exchange step's time
    assert out["value"] > 0 and out["value_exact"] > 0
    assert out["config"]["chunk_mode_collective"]["samples"] >= 1
    assert out["config"]["exact_mode"]["collective"] is None or out["config"]["exact_mode"]["collective"]["samples"] >= 1
    assert out["config"]["exact_mode"]["accepts_per_step"] > 0
    assert out["scaling"] == "weak" and out["unit"] == "sequences/s"


def test_bench_refuses_a_world_that_is_not_gpus():
    """under a launcher (WORLD_SIZE set) the line must not claim another n_gpus: exit non-zero"""
    env = _env()
    env.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29611")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", *ARGS], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_exact_scheme_of_the_stand_in_gives_the_one_process_answer():
    """the stand-in's exact mode at world 1 (no launcher, --gpus 1 --mode exact) selects what the oracle selects
    from the same stream: the hook is a faithful stand-in, not a stub"""
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--mode", "exact", *ARGS], env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert out["n_gpus"] == 1 and out["config"]["accepts_per_step"] > 0


def _line(r):
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_times_the_headline_only_and_full_adds_the_rest():
    """without --full: the headline fields and nothing measured beside them; with --full: the offsets-cache
    timing and the CPU baseline with its oracle check of the last timed step"""
    args = [a for a in ARGS if a != "--no-cpu-baseline"]
    plain = _line(subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", *args], env=_env(),
                                 capture_output=True, text=True, timeout=300))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in plain
    assert plain["steps"] == 1 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert "cpu_baseline" not in plain and "verified_vs_oracle" not in plain
    assert "value_with_offsets_cache" not in plain["config"]
    full = _line(subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--full", *args], env=_env(),
                                capture_output=True, text=True, timeout=300))
    assert full["verified_vs_oracle"] is True
    assert full["cpu_baseline"]["value"] > 0
    assert full["config"]["value_with_offsets_cache"] > 0


def test_plain_run_with_two_gpus_times_the_chunk_scheme_alone():
    out = _line(subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", *ARGS], env=_env(),
                               capture_output=True, text=True, timeout=600))
    assert out["n_gpus"] == 2 and out["value"] > 0
    assert "value_exact" not in out and "exact_mode" not in out["config"]


def test_dump_outputs_writes_the_last_step_and_repeats_itself(tmp_path):
    """--dump-outputs DIR: float32 / float64 arrays of what the last timed step computed, the same from run to run,
    and the members are the oracle's members of the same sequences"""
    import oracle

    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        _line(subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", *ARGS, "--dump-outputs", str(d)],
                             env=_env(), capture_output=True, text=True, timeout=300))
        dumps.append({p.stem: np.load(p) for p in sorted(d.glob("*.npy"))})
    a, b = dumps
    assert set(a) >= {"members_positions", "members_delta_jsd", "total_jsd", "row_totals", "row_entropy",
                      "count_sample", "count_sample_rows"}
    assert a.keys() == b.keys()
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert np.array_equal(a[name], b[name]), name
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    nseq, k, n = 240, 3, 5
    assert a["row_totals"].shape == (nseq,) and a["members_positions"].shape == (n,)
    assert a["count_sample"].shape == (a["count_sample_rows"].size, 4 ** k)
    assert np.all(a["row_totals"] == 200 - k + 1)
    # the stand-in's inputs are torch.randint(0, 4) with bench.py's seed; the oracle on the same sequences
    import torch

    g = torch.Generator(device="cpu")
    g.manual_seed(20260421)
    host = torch.randint(0, 4, (nseq * 200,), dtype=torch.uint8, generator=g).numpy()
    offsets = np.arange(nseq + 1, dtype=np.uint64) * np.uint64(200)
    oset, _ = oracle.nmost_concat(host, offsets, n, k, 4)
    elab, edelta, _, _ = oset.members()
    assert a["members_positions"].tolist() == elab.tolist()
    assert np.allclose(a["members_delta_jsd"], edelta, rtol=1e-12, atol=0)
    assert a["total_jsd"][0] == oset.total_jsd
    for j, r in enumerate(a["count_sample_rows"].astype(int)):
        assert np.array_equal(a["count_sample"][j], oracle.count_kmers(host[r * 200:(r + 1) * 200], 4, k))
