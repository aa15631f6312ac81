"""GPU: the rulebook kernels (K7/K8, csrc/rulebook.hip) on the cases of tests/rulebook_cases.py — every case through
fsf_rulebook_subm, fsf_rulebook_strided (with and without the inverse table), fsf_rulebook_to_pairs on every table,
fsf_order_by_neighbor_mask and fsf_remap_indices — against the dense referee (the oracle on the grids of more than 2^32 cells).

Everything is integer and compared whole with assert_array_equal: no tolerance, no sampling.  The wrappers allocate their outputs
themselves (torch.empty), so an entry a kernel leaves unwritten is made visible two ways: the whole returned tensor is compared, and
before each call blocks of exactly the outputs' sizes are filled with 0x5A5A5A5A and freed, which torch's caching allocator then
hands to the wrapper (best effort: the comparison does not depend on it).  tests/test_rulebook_cases_cpu.py shows, without a GPU,
that these cases tell eight planted defects from the correct algorithm and which decisions of the kernels each case reaches."""
import numpy as np
import pytest
import torch

import rulebook_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops

    return hip_ops


def _poison(device, *shapes):
    blocks = [torch.full(s, R.POISON, dtype=torch.int32, device=device) for s in shapes if int(np.prod(s)) > 0]
    torch.cuda.synchronize()
    del blocks


def _check_pairs(ops, table_dev, want_table):
    """fsf_rulebook_to_pairs as tests/test_hip_ops.py::test_rulebook_subm_bit_exact judges it: num[k] and both pair lists per offset,
    in ascending output row — and nothing written behind them (the wrapper pre-fills the lists with -1)."""
    ip, num = ops.rulebook_to_pairs(table_dev)
    ip, num = ip.cpu().numpy(), num.cpu().numpy()
    m_out, kvol = want_table.shape
    assert ip.shape == (kvol, 2, max(m_out, 1)) and num.shape == (kvol,)
    want = R.table_pairs(want_table)
    np.testing.assert_array_equal(num, [len(i_r) for i_r, _ in want])
    for k, (i_r, o_r) in enumerate(want):
        np.testing.assert_array_equal(ip[k, 0, :num[k]], i_r)
        np.testing.assert_array_equal(ip[k, 1, :num[k]], o_r)
    tail = np.arange(ip.shape[2])[None, :] >= num[:, None]
    assert (ip[:, 0][tail] == -1).all() and (ip[:, 1][tail] == -1).all()


@pytest.mark.parametrize("name", R.ALL)
def test_rulebook_subm_and_its_pairs(ops, device, name):
    c, e = R.case(name), R.expected(name)
    idx = torch.from_numpy(np.array(c["idx"])).to(device)
    _poison(device, e["subm"].shape)
    nbr = ops.rulebook_subm(idx, c["batch"], c["shape"], c["subm_ksize"], c["subm_dilation"])
    got = nbr.cpu().numpy()
    assert got.shape == e["subm"].shape and got.dtype == np.int32
    np.testing.assert_array_equal(got, e["subm"])
    _check_pairs(ops, nbr, e["subm"])


@pytest.mark.parametrize("name", R.ALL)
def test_rulebook_strided_both_tables_and_their_pairs(ops, device, name):
    c, e = R.case(name), R.expected(name)
    idx = torch.from_numpy(np.array(c["idx"])).to(device)
    m, kvol = c["idx"].shape[0], int(np.prod(c["ksize"]))
    cap = max(1, min(m * kvol, c["batch"] * int(np.prod(e["out_shape"]))))
    geom = (c["ksize"], c["stride"], c["padding"], c["dilation"])
    for want_inverse in (True, False):
        _poison(device, (cap, 4), (cap, kvol), (m, kvol))
        o, nbr, nbr_inv, oshape = ops.rulebook_strided(idx, c["batch"], c["shape"], *geom, want_inverse=want_inverse)
        assert list(oshape) == list(e["out_shape"])
        assert tuple(o.shape) == (e["nbr"].shape[0], 4) and tuple(nbr.shape) == e["nbr"].shape
        np.testing.assert_array_equal(o.cpu().numpy(), e["out_indices"].reshape(-1, 4))  # ascending linear (b, z, y, x)
        np.testing.assert_array_equal(nbr.cpu().numpy(), e["nbr"])
        if want_inverse:
            assert tuple(nbr_inv.shape) == (m, kvol)
            np.testing.assert_array_equal(nbr_inv.cpu().numpy(), e["nbr_inv"])
            _check_pairs(ops, nbr.contiguous(), e["nbr"])
            _check_pairs(ops, nbr_inv, e["nbr_inv"])
        else:
            assert nbr_inv is None


@pytest.mark.parametrize("name", R.ALL)
def test_order_by_neighbor_mask_and_remap(ops, device, name):
    c, e = R.case(name), R.expected(name)
    idx = torch.from_numpy(np.array(c["idx"])).to(device)
    m = c["idx"].shape[0]
    _poison(device, (m,), (m,))
    perm, inv = ops.order_by_neighbor_mask(idx, c["batch"], c["shape"])
    perm_h, inv_h = perm.cpu().numpy(), inv.cpu().numpy()
    np.testing.assert_array_equal(perm_h, e["perm"])
    np.testing.assert_array_equal(inv_h[e["perm"]], np.arange(m))
    for table in (e["subm"], e["nbr"]):  # tables of input rows (values < m, -1 entries, possibly no row at all) into the new order
        _poison(device, table.shape)
        got = ops.remap_indices(torch.from_numpy(np.array(table)).to(device), inv).cpu().numpy()
        assert got.shape == table.shape
        np.testing.assert_array_equal(got, np.where(table >= 0, inv_h[np.clip(table, 0, None)], -1))


@pytest.mark.parametrize("name", ["no_output-all", "no_output-half"])
def test_conv_modules_survive_an_empty_coarse_level(ops, device, name):
    """SparseConv3d -> SparseInverseConv3d on one indice_key (inference) where no input, or only half of them, reaches an output
    site: the coarse level has no row (nothing is launched for it), and an input row without an output row gets the inverse
    layer's bias and nothing else — exactly, since its table row is all -1."""
    from fullysparsefusion_amd.mmdet3d_plugin.ops import spconv as sp
    from oracle import spconv as osp

    c, e = R.case(name), R.expected(name)
    m, m_out = c["idx"].shape[0], e["nbr"].shape[0]
    torch.manual_seed(3)
    down = sp.SparseConv3d(64, 64, c["ksize"], stride=c["stride"], padding=c["padding"], indice_key="down").to(device).eval()
    up = sp.SparseInverseConv3d(64, 64, c["ksize"], indice_key="down").to(device).eval()
    feat = torch.randn(m, 64)
    with torch.no_grad():
        x = sp.SparseConvTensor(feat.to(device), torch.from_numpy(np.array(c["idx"])).to(device), list(c["shape"]), c["batch"])
        coarse = down(x)
        fine = up(coarse)
    assert tuple(coarse.features.shape) == (m_out, 64) and list(coarse.spatial_shape) == list(e["out_shape"])
    np.testing.assert_array_equal(coarse.indices.cpu().numpy(), e["out_indices"].reshape(-1, 4))
    np.testing.assert_array_equal(fine.indices.cpu().numpy(), c["idx"])
    pairs = [(torch.from_numpy(i_r.astype(np.int64)), torch.from_numpy(o_r.astype(np.int64))) for i_r, o_r in R.table_pairs(e["nbr"])]
    w_down, w_up = (mod.weight.detach().cpu().reshape(27, 64, 64) for mod in (down, up))
    y = osp.indice_conv(feat, w_down, pairs, m_out) + down.bias.detach().cpu()
    want = osp.indice_conv(y, w_up, pairs, m, inverse=True) + up.bias.detach().cpu()
    got = fine.features.cpu()
    assert tuple(got.shape) == (m, 64)
    np.testing.assert_allclose(coarse.features.cpu().numpy(), y.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-4, atol=1e-4)  # (the bound of test_spconv_forward_subm_vs_oracle)
    dead = (e["nbr_inv"] < 0).all(1)
    assert dead.all() if name == "no_output-all" else (dead.any() and not dead.all())
    assert torch.equal(got[torch.from_numpy(dead)], up.bias.detach().cpu().expand(int(dead.sum()), 64))


def test_refused_geometries_raise(ops, device):
    """Both refusals are return codes before any launch: an even kernel size of a submanifold convolution (FSF_ERR_UNSUPPORTED), and
    a kernel extent larger than the padded input, O < 1 (FSF_ERR_INVALID_ARG) — also where C's division towards zero would turn
    floor(-1 / 2) + 1 = 0 into 1 (Z = 2, kernel 3, stride 2, padding 0)."""
    from fullysparsefusion_amd._lib import FsfHipError

    idx = torch.tensor([[0, 0, 0, 0], [0, 1, 2, 3], [1, 0, 1, 1]], dtype=torch.int32, device=device)
    for ksize in ((2, 2, 2), (3, 3, 2), (4, 3, 3)):
        with pytest.raises(FsfHipError):
            ops.rulebook_subm(idx, 2, (4, 6, 6), ksize)
    for shape, ksize, stride, dilation in (((1, 6, 6), (3, 3, 3), (2, 2, 2), (1, 1, 1)), ((2, 6, 6), (3, 3, 3), (2, 2, 2), (1, 1, 1)),
                                           ((4, 6, 6), (3, 3, 3), (1, 1, 1), (2, 1, 1)), ((4, 6, 4), (3, 3, 5), (3, 3, 3), (1, 1, 1))):
        assert min(R.out_shape(shape, ksize, stride, (0, 0, 0), dilation)) < 1
        for want_inverse in (True, False):
            with pytest.raises(FsfHipError):
                ops.rulebook_strided(idx[:1], 2, shape, ksize, stride, (0, 0, 0), dilation, want_inverse=want_inverse)
