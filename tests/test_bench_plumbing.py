"""bench.py's multi-rank control flow on CPU: tests/bench_cpu_harness.py swaps bench.py's GPU hooks for stand-ins and runs bench.main():
`--gpus 2` re-launches itself under torch.distributed.run exactly as on a GPU node (self-spawn, 127.0.0.1 rendezvous, one process per
rank), shards the cfg5 sweep weak and strong, runs the product's PlannerSweep.step() with the stand-in back-end of
test_distributed_gloo.py over gloo, goes through measure()'s barriers / max-over-ranks reductions / collective timing, and rank 0 prints
ONE short JSON line with the fields the driver parses and writes the full record to a file.  Also: the line stays SHORT at full size
(the 24 KB line of round 3 could not be parsed)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np

import conftest


def _run(gpus, tmp_path, extra=(), full_mode=True):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(conftest.ROOT, "tests"), conftest.ROOT, conftest.PKG, env.get("PYTHONPATH", "")])
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    full = str(tmp_path / "full.json")
    cmd = [sys.executable, os.path.join(conftest.ROOT, "tests", "bench_cpu_harness.py"), "--gpus", str(gpus), "--steps", "3", "--warmup", "1",
           "--sweep-per-gpu", "6", "--sweep-total", "13", "--no-cpu-baseline", "--full-out", full] + (["--full"] if full_mode else []) + list(extra)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[-1]), lines[-1], (json.load(open(full)) if os.path.exists(full) else None)


def test_bench_two_ranks_self_spawn(tmp_path):
    out, line, full = _run(2, tmp_path)
    assert len(line) < 6000
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1 and out["higher_is_better"] is True
    for k in ("metric", "value", "value_launched", "unit", "ms_per_step", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "summary"):
        assert k in out, k
    assert "configs" not in out                                  # the stdout line is the SHORT one
    weak, strong = full["configs"]
    assert weak["scaling"] == "weak" and strong["scaling"] == "strong"
    assert weak["world_size"] == 2 and "allgather_ms" in weak and "allgather_ms" in strong
    assert weak["config"]["scenarios_total"] == 12 and strong["config"]["scenarios_total"] == 13      # ragged strong shards: 7 + 6
    # whole-job units: both ranks' region QPs per step
    assert abs(weak["value_launched"] * weak["ms_per_step"] * 1e-3 - 12 * 4) < 1e-6
    assert abs(strong["value_launched"] * strong["ms_per_step"] * 1e-3 - 13 * 4) < 1e-6
    # the scaling line itself shows that a collective over N ranks ran (the headline has none): VERDICT r4 item 7
    assert out["world_size"] == 2 and out["allgather_ms"] == out["summary"]["cfg5_weak"]["allgather_ms"] and "int32 status" in out["collective"]
    assert weak["config"]["winner_record_bytes"] == 632
    assert set(out["summary"]) == {"stand_in", "cfg5_weak", "cfg5_strong"}
    assert all(len(v) <= 9 for v in out["summary"].values())     # eight numbers per sub-config (+ allgather_ms for the sweeps)


def test_bench_one_rank_no_process_group(tmp_path):
    out, line, full = _run(1, tmp_path)
    assert out["n_gpus"] == 1 and full["configs"][1]["config"]["scenarios_this_rank"] == 13
    assert "collective" not in out                                # one rank: nothing is gathered, nothing is claimed


def test_bench_plain_run_is_the_headline_alone(tmp_path):
    """Without --full: the headline's timed steps and its line, nothing else -- no other configs, no CPU baseline, no latency or
    kernel-train runs, no full-record file; --dump-outputs writes the last timed step's outputs as float64 arrays."""
    dump = tmp_path / "out"
    out, line, full = _run(1, tmp_path, extra=["--dump-outputs", str(dump)], full_mode=False)
    assert full is None and out["full_record"] is None
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "solves/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert set(out["summary"]) == {"stand_in"} and "cpu_baseline" not in out and "collective" not in out
    assert "p50_step_latency_ms" not in out["config"]
    files = sorted(os.listdir(dump))
    assert files == ["iters.npy", "kkt.npy", "status.npy"], files
    for f in files:
        a = np.load(os.path.join(dump, f))
        assert a.dtype == np.float64 and a.shape == (256,)


def test_dump_outputs_sample_above_the_limit(tmp_path):
    """bench.write_outputs keeps a fixed, seeded sample of the rows of every array once the outputs exceed 64 MB in all."""
    sys.path.insert(0, conftest.ROOT)
    import bench

    big = {"X": np.arange(9 * 2 ** 20, dtype=np.float64).reshape(-1, 8), "status": np.zeros(9 * 2 ** 20 // 8)}
    for d in ("a", "b"):
        bench.write_outputs(dict(big), str(tmp_path / d))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 10 ** 6
    for f in ("X.npy", "X.rows.npy", "status.npy", "status.rows.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    rows = np.load(tmp_path / "a" / "X.rows.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "X.npy"), big["X"][rows])


def test_stdout_line_stays_short_at_full_size():
    """stdout_line() on the FULL records of real default runs kept from the GPU box (profiles/bench_full_*.json: headline + nine
    sub-configs + cpu_baseline): under 6 KB, with the objects the driver needs."""
    sys.path.insert(0, conftest.ROOT)
    import bench

    kept = sorted(glob.glob(os.path.join(conftest.ROOT, "profiles", "bench_full_*.json")))
    assert kept, "no kept full bench record under profiles/"
    for path in kept:
        full = json.load(open(path))
        line = json.dumps(bench.stdout_line(full))
        assert len(line) < 6000, (path, len(line))
        out = json.loads(line)
        assert out["roofline"]["frac"] > 0 and out["cpu_baseline"]["value"] > 0 and len(out["summary"]) >= 10
        assert out["value"] <= out["value_launched"]
