"""Which forward kernel a sparse convolution layer gets (ops/spconv.py `choose_kernel`), without a GPU: the decision over a grid of
layers recorded from the code before the five places that answered the question were brought together, one rule per kernel written
out by hand, the layer's single prepared-weight cache, and the plane-kernel branch leaving a lazy `.features` unformed."""
import types

import pytest
import torch

from fullysparsefusion_amd import hip_ops, switches
from fullysparsefusion_amd.mmdet3d_plugin.ops import spconv as sp

ROWS = (0, 1, 4095, 4096, 10000, 10001)
SOURCES = ("none", "match", "mismatch")  # plane sources at hand: none / widths that sum to cin / one 32-channel source (no cin here is 32)
LETTER = {"P": sp.PLANES, "H": sp.SPLIT_F16, "S": sp.SPLIT, "F": sp.FP32}

# (kind, cin, cout, mode) -> one group per entry of ROWS (table rows = operand rows), in each group one letter per
# (source in SOURCES) x (PLANES on, off) x (TRAIN_PLANES on, off), the last fastest.  Kernel volume 27.  Recorded from the predicates
# of SparseConvolution.forward (inference) and the branches of _SparseConvFn.forward / .backward fed the flags the layer passed
# (training; "train_dgrad" = the data gradient, which asks with cin / cout swapped), before `choose_kernel` replaced them.
RECORDED = {
    ("subm", 64, 64, "infer"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PPSSPPSSSSSS PPSSPPSSSSSS PPSSPPSSSSSS",
    ("subm", 64, 64, "train_fwd"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PSSSPSSSPSSS PSSSPSSSPSSS PSSSPSSSPSSS",
    ("subm", 64, 64, "train_dgrad"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PSSSPSSSPSSS PSSSPSSSPSSS PSSSPSSSPSSS",
    ("subm", 64, 128, "infer"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PPSSPPSSSSSS PPSSPPSSSSSS PPSSPPSSSSSS",
    ("subm", 64, 128, "train_fwd"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PSSSPSSSPSSS PSSSPSSSPSSS PSSSPSSSPSSS",
    ("subm", 64, 128, "train_dgrad"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PSSSPSSSPSSS PSSSPSSSPSSS PSSSPSSSPSSS",
    ("subm", 128, 128, "infer"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PPSSPPSSSSSS PPSSPPSSSSSS PPSSPPSSSSSS",
    ("subm", 128, 128, "train_fwd"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PSSSPSSSPSSS PSSSPSSSPSSS PSSSPSSSPSSS",
    ("subm", 128, 128, "train_dgrad"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PSSSPSSSPSSS PSSSPSSSPSSS PSSSPSSSPSSS",
    ("subm", 128, 256, "infer"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PPSSPPSSSSSS PPSSPPSSSSSS PPSSPPSSSSSS",
    ("subm", 128, 256, "train_fwd"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PSSSPSSSPSSS PSSSPSSSPSSS PSSSPSSSPSSS",
    ("subm", 128, 256, "train_dgrad"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PSSSPSSSPSSS PSSSPSSSPSSS PSSSPSSSPSSS",
    ("subm", 256, 256, "infer"): "FFFFFFFFFFFF HHHHHHHHHHHH HHHHHHHHHHHH PPHHPPHHHHHH PPHHPPHHHHHH PPHHPPHHHHHH",
    ("subm", 256, 256, "train_fwd"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PSSSPSSSPSSS PSSSPSSSPSSS PSSSPSSSPSSS",
    ("subm", 256, 256, "train_dgrad"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PSSSPSSSPSSS PSSSPSSSPSSS PSSSPSSSPSSS",
    ("subm", 256, 512, "infer"): "FFFFFFFFFFFF HHHHHHHHHHHH HHHHHHHHHHHH PPHHPPHHHHHH PPHHPPHHHHHH PPHHPPHHHHHH",
    ("subm", 256, 512, "train_fwd"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PSSSPSSSPSSS PSSSPSSSPSSS PSSSPSSSPSSS",
    ("subm", 256, 512, "train_dgrad"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS",
    ("subm", 512, 512, "infer"): "FFFFFFFFFFFF HHHHHHHHHHHH HHHHHHHHHHHH HHHHHHHHHHHH HHHHHHHHHHHH HHHHHHHHHHHH",
    ("subm", 512, 512, "train_fwd"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS",
    ("subm", 512, 512, "train_dgrad"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS",
    ("subm", 1024, 512, "infer"): "FFFFFFFFFFFF HHHHHHHHHHHH HHHHHHHHHHHH HHHHHHHHHHHH HHHHHHHHHHHH HHHHHHHHHHHH",
    ("subm", 1024, 512, "train_fwd"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS",
    ("subm", 1024, 512, "train_dgrad"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS",
    ("subm", 512, 256, "infer"): "FFFFFFFFFFFF HHHHHHHHHHHH HHHHHHHHHHHH HHHHHHHHHHHH HHHHHHHHHHHH HHHHHHHHHHHH",
    ("subm", 512, 256, "train_fwd"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS",
    ("subm", 512, 256, "train_dgrad"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PSSSPSSSPSSS PSSSPSSSPSSS PSSSPSSSPSSS",
    ("subm", 256, 128, "infer"): "FFFFFFFFFFFF HHHHHHHHHHHH HHHHHHHHHHHH PPHHPPHHHHHH PPHHPPHHHHHH PPHHPPHHHHHH",
    ("subm", 256, 128, "train_fwd"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PSSSPSSSPSSS PSSSPSSSPSSS PSSSPSSSPSSS",
    ("subm", 256, 128, "train_dgrad"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PSSSPSSSPSSS PSSSPSSSPSSS PSSSPSSSPSSS",
    ("subm", 6, 64, "infer"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("subm", 6, 64, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("subm", 6, 64, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("subm", 48, 64, "infer"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS",
    ("subm", 48, 64, "train_fwd"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS",
    ("subm", 48, 64, "train_dgrad"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS",
    ("subm", 96, 64, "infer"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PPSSPPSSSSSS PPSSPPSSSSSS PPSSPPSSSSSS",
    ("subm", 96, 64, "train_fwd"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PSSSPSSSPSSS PSSSPSSSPSSS PSSSPSSSPSSS",
    ("subm", 96, 64, "train_dgrad"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS",
    ("strided", 64, 64, "infer"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PPSSPPSSSSSS PPSSPPSSSSSS PPFFPPFFFFFF",
    ("strided", 64, 64, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("strided", 64, 64, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("strided", 64, 128, "infer"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PPSSPPSSSSSS PPSSPPSSSSSS PPFFPPFFFFFF",
    ("strided", 64, 128, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("strided", 64, 128, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("strided", 128, 128, "infer"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PPSSPPSSSSSS PPSSPPSSSSSS PPFFPPFFFFFF",
    ("strided", 128, 128, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("strided", 128, 128, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("strided", 128, 256, "infer"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PPSSPPSSSSSS PPSSPPSSSSSS PPFFPPFFFFFF",
    ("strided", 128, 256, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("strided", 128, 256, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("strided", 256, 256, "infer"): "FFFFFFFFFFFF HHHHHHHHHHHH HHHHHHHHHHHH PPHHPPHHHHHH PPHHPPHHHHHH PPFFPPFFFFFF",
    ("strided", 256, 256, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("strided", 256, 256, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("strided", 256, 512, "infer"): "FFFFFFFFFFFF HHHHHHHHHHHH HHHHHHHHHHHH PPHHPPHHHHHH PPHHPPHHHHHH PPFFPPFFFFFF",
    ("strided", 256, 512, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("strided", 256, 512, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("strided", 512, 512, "infer"): "FFFFFFFFFFFF HHHHHHHHHHHH HHHHHHHHHHHH HHHHHHHHHHHH HHHHHHHHHHHH FFFFFFFFFFFF",
    ("strided", 512, 512, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("strided", 512, 512, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("strided", 1024, 512, "infer"): "FFFFFFFFFFFF HHHHHHHHHHHH HHHHHHHHHHHH HHHHHHHHHHHH HHHHHHHHHHHH FFFFFFFFFFFF",
    ("strided", 1024, 512, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("strided", 1024, 512, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("strided", 512, 256, "infer"): "FFFFFFFFFFFF HHHHHHHHHHHH HHHHHHHHHHHH HHHHHHHHHHHH HHHHHHHHHHHH FFFFFFFFFFFF",
    ("strided", 512, 256, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("strided", 512, 256, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("strided", 256, 128, "infer"): "FFFFFFFFFFFF HHHHHHHHHHHH HHHHHHHHHHHH PPHHPPHHHHHH PPHHPPHHHHHH PPFFPPFFFFFF",
    ("strided", 256, 128, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("strided", 256, 128, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("strided", 6, 64, "infer"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("strided", 6, 64, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("strided", 6, 64, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("strided", 48, 64, "infer"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS SSSSSSSSSSSS FFFFFFFFFFFF",
    ("strided", 48, 64, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("strided", 48, 64, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("strided", 96, 64, "infer"): "FFFFFFFFFFFF SSSSSSSSSSSS SSSSSSSSSSSS PPSSPPSSSSSS PPSSPPSSSSSS PPFFPPFFFFFF",
    ("strided", 96, 64, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("strided", 96, 64, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("inverse", 64, 64, "infer"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PPFFPPFFFFFF PPFFPPFFFFFF PPFFPPFFFFFF",
    ("inverse", 64, 64, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("inverse", 64, 64, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("inverse", 64, 128, "infer"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PPFFPPFFFFFF PPFFPPFFFFFF PPFFPPFFFFFF",
    ("inverse", 64, 128, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("inverse", 64, 128, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("inverse", 128, 128, "infer"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PPFFPPFFFFFF PPFFPPFFFFFF PPFFPPFFFFFF",
    ("inverse", 128, 128, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("inverse", 128, 128, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("inverse", 128, 256, "infer"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PPFFPPFFFFFF PPFFPPFFFFFF PPFFPPFFFFFF",
    ("inverse", 128, 256, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("inverse", 128, 256, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("inverse", 256, 256, "infer"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PPFFPPFFFFFF PPFFPPFFFFFF PPFFPPFFFFFF",
    ("inverse", 256, 256, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("inverse", 256, 256, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("inverse", 256, 512, "infer"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PPFFPPFFFFFF PPFFPPFFFFFF PPFFPPFFFFFF",
    ("inverse", 256, 512, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("inverse", 256, 512, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("inverse", 512, 512, "infer"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("inverse", 512, 512, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("inverse", 512, 512, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("inverse", 1024, 512, "infer"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("inverse", 1024, 512, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("inverse", 1024, 512, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("inverse", 512, 256, "infer"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("inverse", 512, 256, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("inverse", 512, 256, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("inverse", 256, 128, "infer"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PPFFPPFFFFFF PPFFPPFFFFFF PPFFPPFFFFFF",
    ("inverse", 256, 128, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("inverse", 256, 128, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("inverse", 6, 64, "infer"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("inverse", 6, 64, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("inverse", 6, 64, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("inverse", 48, 64, "infer"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("inverse", 48, 64, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("inverse", 48, 64, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
    ("inverse", 96, 64, "infer"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PPFFPPFFFFFF PPFFPPFFFFFF PPFFPPFFFFFF",
    ("inverse", 96, 64, "train_fwd"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF PFFFPFFFPFFF PFFFPFFFPFFF PFFFPFFFPFFF",
    ("inverse", 96, 64, "train_dgrad"): "FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF FFFFFFFFFFFF",
}


def _widths(source, cin):
    return {"none": None, "match": sp.source_widths(cin), "mismatch": [32]}[source]


def test_choose_kernel_reproduces_the_recorded_decisions():
    assert len(RECORDED) == 3 * 13 * 3
    checked = 0
    for (kind, cin, cout, mode), groups in RECORDED.items():
        groups = groups.split(" ")
        assert len(groups) == len(ROWS) and all(len(g) == 12 for g in groups)
        a, b = (cout, cin) if mode == "train_dgrad" else (cin, cout)
        for rows, group in zip(ROWS, groups):
            letters = iter(group)
            for source in SOURCES:
                for planes_on in (True, False):
                    for train_planes_on in (True, False):
                        got = sp.choose_kernel(kind, a, b, 27, rows, rows, _widths(source, cin), mode != "infer", planes_on, train_planes_on)
                        assert got == LETTER[next(letters)], (kind, cin, cout, mode, rows, source, planes_on, train_planes_on, got)
                        checked += 1
    assert checked == 8424


def test_one_rule_per_kernel_written_out():
    assert sp.choose_kernel("subm", 64, 64, 27, 4096, 4096) == "planes"
    assert sp.choose_kernel("subm", 64, 64, 27, 4095, 4095) == "split"
    assert sp.choose_kernel("inverse", 256, 128, 27, 20000, 5000, planes_on=False) == "fp32"
    assert sp.choose_kernel("inverse", 256, 128, 27, 20000, 5000, [256]) == "fp32"  # (one 256-channel source: no shape of the plane kernel)
    assert sp.choose_kernel("inverse", 256, 128, 27, 20000, 5000) == "planes"
    assert sp.choose_kernel("subm", 512, 512, 27, 3000, 3000) == "split_f16"
    # no rows on either side: nothing to launch
    assert sp.choose_kernel("subm", 64, 64, 27, 0, 5000) == "fp32" and sp.choose_kernel("strided", 64, 64, 27, 5000, 0) == "fp32"
    # the autograd path: planes need both switches, split is submanifold-only and never the f16 variant, `split_on` is a veto
    assert sp.choose_kernel("subm", 64, 64, 27, 4096, 4096, train=True) == "planes"
    assert sp.choose_kernel("subm", 64, 64, 27, 4096, 4096, train=True, train_planes_on=False) == "split"
    assert sp.choose_kernel("strided", 128, 128, 27, 3000, 9000, train=True) == "fp32"
    assert sp.choose_kernel("subm", 512, 512, 27, 3000, 3000, train=True) == "split"
    assert sp.choose_kernel("subm", 512, 512, 27, 3000, 3000, train=True, split_on=False) == "fp32"


def test_the_layer_asks_with_its_own_shape_the_switches_and_the_threshold_of_the_moment(monkeypatch):
    subm, strided = sp.SubMConv3d(64, 64, 3, bias=False), sp.SparseConv3d(64, 128, 3, stride=2, bias=False)
    inverse = sp.SparseInverseConv3d(256, 128, 3, indice_key="k", bias=False)
    assert subm.kernel_for(5000, 5000) == "planes" and subm.takes_planes([64], 5000) and not subm.takes_planes([32], 5000)
    assert strided.kernel_for(10000, 30000, [64]) == "planes" and strided.kernel_for(4000, 30000) == "split"
    assert inverse.kernel_for(20000, 5000) == "planes" and inverse.kernel_for(4000, 1000) == "fp32"
    assert subm.kernel_for(100, 100) == "split" and not subm.takes_planes([64], 100)
    monkeypatch.setattr(sp.SparseConvolution, "PLANES_MIN_ROWS", 64)
    assert subm.kernel_for(100, 100) == "planes" and subm.takes_planes([64], 100)
    monkeypatch.setattr(sp.SparseConvolution, "SPLIT_STRIDED_MAX_ROWS", 50)
    assert strided.kernel_for(60, 100) == "fp32" and strided.kernel_for(50, 100) == "split"
    monkeypatch.setattr(switches, "PLANES", False)
    assert subm.kernel_for(5000, 5000) == "split" and not subm.takes_planes([64], 5000)
    monkeypatch.setattr(switches, "PLANES", True)
    monkeypatch.setattr(switches, "TRAIN_PLANES", False)
    assert subm.kernel_for(5000, 5000) == "planes" and subm.kernel_for(5000, 5000, train=True) == "split"


def test_source_widths_and_the_splitter_agree(monkeypatch):
    assert [sp.source_widths(c) for c in (32, 128, 136, 256)] == [[32], [128], [68, 68], [128, 128]]
    monkeypatch.setattr(hip_ops, "to_planes", lambda f: f)
    for c in (64, 128, 256):
        feat = torch.arange(3 * c, dtype=torch.float32).reshape(3, c)
        parts = sp._plane_srcs(feat)
        assert [p.size(1) for p in parts] == sp.source_widths(c) and torch.equal(torch.cat(parts, 1), feat)


def test_plane_kernel_layer_under_no_grad_leaves_lazy_features_unformed(monkeypatch):
    m, calls = 5000, []
    conv = sp.SubMConv3d(128, 64, 3, bias=False, indice_key="subm")
    idx = torch.zeros((m, 4), dtype=torch.int32)
    x = sp.SparseConvTensor((torch.zeros(m, 64), torch.zeros(m, 64)), idx, [8, 8, 8], 1)
    x.plane_sources = [types.SimpleNamespace(c=64, m=m), types.SimpleNamespace(c=64, m=m)]
    x.indice_dict["subm"] = sp.Rulebook("subm", torch.zeros((m, 27), dtype=torch.int32), idx, [8, 8, 8], idx, [8, 8, 8])

    def forward_planes(sources, wplanes, kvol, cout, nbr, **kw):
        calls.append((sources, wplanes, kvol, cout, kw))
        return torch.zeros(nbr.size(0), cout), "planes of the output"

    monkeypatch.setattr(hip_ops, "spconv_forward_planes", forward_planes)
    monkeypatch.setattr(hip_ops, "spconv_prepare_weight_planes", lambda w: "prepared")
    with torch.no_grad():
        y = conv(x, relu=True)
    assert x._features is None, "the plane-kernel branch read x.features: the lazy concatenation was written"
    (sources, wplanes, kvol, cout, kw), = calls
    assert sources is x.plane_sources and wplanes == "prepared" and (kvol, cout) == (27, 64)
    assert kw == dict(scale=None, shift=None, residual=None, relu=True, want_planes=True)
    assert y.features.shape == (m, 64) and y.plane_sources == ["planes of the output"]


def test_one_prepared_weight_cache_per_layer(monkeypatch):
    conv, made = sp.SubMConv3d(8, 8, 3), []

    def prepare(name):
        def f(w):
            made.append((name, tuple(w.shape)))
            return (name, len(made))
        return f

    for kernel, name in sp.SparseConvolution._PREPARE.items():
        monkeypatch.setattr(hip_ops, name, prepare(kernel))
    keys = sorted(conv.state_dict())
    for kernel in (sp.FP32, sp.SPLIT, sp.SPLIT_F16, sp.PLANES):
        assert conv._prepared(kernel) is conv._prepared(kernel)
    assert made == [(k, (27, 8, 8)) for k in (sp.FP32, sp.SPLIT, sp.SPLIT_F16, sp.PLANES)]  # two calls, prepared once, per kernel
    first = conv._prepared(sp.SPLIT)
    with torch.no_grad():
        conv.weight.add_(1.0)  # an optimizer step: same storage, new version
    assert conv._prepared(sp.SPLIT) != first and conv._prepared(sp.SPLIT) is conv._prepared(sp.SPLIT) and len(made) == 5
    assert conv._prepared(sp.PLANES) == (sp.PLANES, 6)  # every kernel's entry goes stale on its own
    conv.weight.data = conv.weight.data.clone()  # a re-assigned parameter: new storage
    conv._prepared(sp.SPLIT)
    assert len(made) == 7
    # the cache is no parameter, buffer or state_dict entry
    assert sorted(conv.state_dict()) == keys == ["bias", "weight"] and sorted(sp.SubMConv3d(8, 8, 3, bias=False).state_dict()) == ["weight"]
    assert [n for n, _ in conv.named_parameters()] == ["weight", "bias"] and list(conv.buffers()) == []
