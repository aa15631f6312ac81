"""CPU: what a plain bench.py run spends beside its timed steps — `--full` is off unless asked for, and the line's query / box counts
then take no extra pass of the detector."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_full_is_off_unless_asked_for(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--full"])
    assert bench.parse().full is True


def test_plain_description_runs_no_extra_pass(monkeypatch):
    def no_pass(*a, **k):
        raise AssertionError("a plain run ran an extra pass of the detector")

    monkeypatch.setattr(bench, "step", no_pass)
    out = [dict(boxes_3d=torch.zeros(5, 9))]
    args = argparse.Namespace(no_describe=False, train=False, hot_path_only=False, full=False)
    assert bench.describe_output(None, None, out, args) == {"boxes_out": 5}
    # --full: the query counts from one untimed pass of the query-generation stages
    hot = dict(frustum_obj_feats=torch.zeros(7, 4), fsd_obj_feats=torch.zeros(3, 4))
    monkeypatch.setattr(bench, "step", lambda model, inp, hot_path_only=False, nxt=None: hot if hot_path_only else no_pass())
    args.full = True
    assert bench.describe_output(None, None, out, args) == dict(camera_queries=7, lidar_queries=3, boxes_out=5)
    # the training / query-stage outputs carry their counts: no pass either way
    monkeypatch.setattr(bench, "step", no_pass)
    for full in (False, True):
        args = argparse.Namespace(no_describe=False, train=False, hot_path_only=True, full=full)
        assert bench.describe_output(None, None, hot, args) == dict(camera_queries=7, lidar_queries=3)
