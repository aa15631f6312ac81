"""GPU: the sparse-convolution weight gradient (K10 on the fp32 matrix pipe, K10p on the bf16 matrix cores, the fold kernel behind both;
fullysparsefusion_amd/csrc/spconv_bwd.hip) on the crafted pair lists of tests/wgrad_cases.py, every result compared bit for bit with
the int64 / float64 referee — tests/test_wgrad_cases_cpu.py shows which decisions of the kernels each case reaches and that a model of
the two launches with any of nine defects fails one of them.  Every case: the result, the same call again (bitwise determinism), and,
where an offset's pair range is split and some splits are dead, a call of the same plan with every list full and other values first, so
that the dead splits' workspace slices hold non-zero sums when the case runs."""
import numpy as np
import pytest
import torch

import wgrad_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops

    return hip_ops


@pytest.mark.parametrize("name", W.NAMES)
def test_weight_gradient_equals_the_referee_bit_for_bit(ops, device, name):
    d = W.case(name)
    c = d["case"]
    feat, gout = torch.tensor(d["feat"], device=device), torch.tensor(d["gout"], device=device)  # (the case's arrays are read-only)
    if c.num is None:
        run = lambda: ops.linear_backward_weight(feat, gout)[None]
    else:
        assert d["pairs"].min() >= 0 and d["pairs"][:, 0].max() < c.m_in and d["pairs"][:, 1].max() < c.m_out and max(c.num) <= c.cap
        pairs, num = torch.tensor(d["pairs"], device=device), torch.tensor(d["num"], device=device)
        run = lambda: ops.spconv_backward_weight(feat, gout, pairs, num)
        if W.needs_stale_workspace(c):
            f2, g2 = (torch.from_numpy(x).to(device) for x in W.operands(c, key=7))
            full = torch.full((c.kvol,), c.cap, dtype=torch.int32, device=device)
            filled = ops.spconv_backward_weight(f2, g2, pairs, full)
            assert int(torch.count_nonzero(filled)) > 0.9 * filled.numel()  # (every slice of the workspace was summed into this)
    got = run()
    assert got.shape == (c.kvol, c.cin, c.cout)
    W.check_exact(name, got.cpu().numpy(), d["want"])
    assert torch.equal(got, run())
