"""bench.py's lines on the device: a plain run carries the contract's keys and nothing it had to measure beside the headline; a
`--full` run adds the instrumented roofline pass and the HBM table, which must come out (a change in an op's calling convention that
the accounting hooks do not follow would otherwise only show at round end)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_full_line_has_roofline_and_hbm_table():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--full"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["value"] > 0 and d["config"]["workload"].startswith("fsf_nuscenes_10sweep")
    roof = d["roofline"]
    assert roof["bound"] == "mfma" and 0 < roof["frac"] < 1 and roof["peak"] > roof["achieved"] > 0
    # the in-situ table (what is quoted) and, under `debug`, the cache-warm isolated replay it replaced as the headline of this block
    replay = roof["debug"]["hbm_isolated_replay"]
    for k in ("linear_norm_act", "seg_reduce", "sir_input", "rows_to_planes"):
        assert replay[k]["ms_per_step"] > 0 and 0 < replay[k]["frac_of_hbm_peak"] < 1
    assert "hbm" not in roof and "frac_of_fp32_pipe_peak" not in json.dumps(roof)
    for k in ("linear_norm_act", "seg_reduce", "sir_input"):
        assert 0 < roof["hbm_in_situ"][k]["frac_of_hbm_peak"] < 1


@pytest.mark.gpu
def test_bench_plain_line_measures_nothing_beside_the_headline():
    """Without `--full` the line holds the contract's keys and the workload's description, and none of the blocks that take passes
    of their own (extra loops, the instrumented pass, the side workloads, the CPU oracle)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config"):
        assert key in d, key
    assert d["metric"] == "frames/sec fwd nuScenes 10-sweep FSF" and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    for key in ("frame_front", "launches", "roofline", "stages", "h2d", "trained_like", "train", "allreduce", "cpu_baseline"):
        assert key not in d, key
    cfg = d["config"]
    assert cfg["workload"].startswith("fsf_nuscenes_10sweep") and cfg["boxes_out"] > 0 and "camera_queries" not in cfg


@pytest.mark.gpu
def test_bench_dump_outputs_holds_the_last_timed_steps_results(tmp_path):
    """`--dump-outputs DIR`: the results the timed path returned in its last step (FSF.simple_test: boxes, scores, labels of the frame)
    as DIR/<name>.npy, and `--steps` sets the number of timed steps."""
    import numpy as np

    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-roofline",
                        "--no-trained-like", "--no-h2d", "--no-train-block", "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    files = sorted(f for f in os.listdir(dump) if f.endswith(".npy"))
    assert files == ["0.boxes_3d.npy", "0.labels_3d.npy", "0.scores_3d.npy"] and d["dump_outputs"]["arrays"] == 3
    boxes, scores, labels = (np.load(dump / f) for f in ("0.boxes_3d.npy", "0.scores_3d.npy", "0.labels_3d.npy"))
    assert boxes.dtype == scores.dtype == np.float32 and labels.dtype == np.float64
    assert boxes.shape == (d["config"]["boxes_out"], 9) and scores.shape == labels.shape == (boxes.shape[0],) and boxes.shape[0] > 0
    assert np.isfinite(boxes).all() and (labels == np.round(labels)).all()
