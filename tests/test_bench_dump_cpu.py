"""CPU: bench.py's `--dump-outputs` writer — what becomes an array, the dtypes, the 64 MB budget and its seeded row sample."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
from fullysparsefusion_amd.mmdet3d_plugin.core.bbox import LiDARInstance3DBoxes  # noqa: E402


def test_collect_outputs_names_and_dtypes():
    g = torch.Generator().manual_seed(0)
    out = [dict(boxes_3d=LiDARInstance3DBoxes(torch.randn(7, 9, generator=g), box_dim=9), scores_3d=torch.rand(7, generator=g),
                labels_3d=torch.arange(7), extra=dict(n=3, half=torch.ones(2, dtype=torch.float16), f64=torch.zeros(2, dtype=torch.float64),
                                                     flag=torch.tensor([True, False]), note="text"))]
    arrays, skipped = bench.collect_outputs(out)
    got = {name: a for name, a in arrays}
    assert list(got) == ["0.boxes_3d", "0.scores_3d", "0.labels_3d", "0.extra.n", "0.extra.half", "0.extra.f64", "0.extra.flag"]
    assert skipped == ["0.extra.note"]
    np.testing.assert_array_equal(got["0.boxes_3d"], out[0]["boxes_3d"].tensor.numpy())
    assert got["0.boxes_3d"].dtype == got["0.scores_3d"].dtype == got["0.extra.half"].dtype == np.float32
    assert got["0.labels_3d"].dtype == got["0.extra.f64"].dtype == got["0.extra.flag"].dtype == got["0.extra.n"].dtype == np.float64
    np.testing.assert_array_equal(got["0.labels_3d"], np.arange(7))


def test_dump_outputs_keeps_the_budget_with_a_fixed_row_sample(tmp_path):
    rng = np.random.default_rng(0)
    arrays = [("big", rng.standard_normal((200000, 16)).astype(np.float32)),  # 12.8 MB
              ("wide", rng.standard_normal((1, 50000, 8)).astype(np.float32)),  # 1.6 MB, leading axis of length 1
              ("small", rng.standard_normal((1000, 4)).astype(np.float32)), ("scalar", np.asarray(3.0))]
    budget = 4 << 20
    info = bench.dump_outputs(arrays, [], str(tmp_path / "a"), budget=budget)
    again = bench.dump_outputs(arrays, [], str(tmp_path / "b"), budget=budget)
    assert info["sampled"] == again["sampled"] and set(info["sampled"]) == {"big", "wide"}
    assert info["bytes"] <= budget and sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= budget
    for name, a in arrays:
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        np.testing.assert_array_equal(x, y)
        if name in info["sampled"]:  # rows of the original, in order
            rows = a.reshape(-1, a.shape[-1])
            idx = [int(np.flatnonzero((rows == r).all(1))[0]) for r in x[:50]]
            assert idx == sorted(idx) and len(x) == info["sampled"][name]["rows"] < len(rows)
        else:
            np.testing.assert_array_equal(x, a)
    assert (tmp_path / "a" / ".gitignore").read_text() == "*\n"  # a directory the dump made keeps itself out of version control
    whole = bench.dump_outputs(arrays, [], str(tmp_path / "c"))
    assert whole["sampled"] == {} and whole["bytes"] == sum(a.nbytes for _, a in arrays)
