"""GPU: what the producers of the two matrix-core operand formats WRITE, bit for bit against the numpy model of tests/product_budget.py
(`pick_scale`, `split_f16`, `split_bf16`) — the expected halfwords, scales and header words come from the model, never from the library.

* Row planes: `to_planes` (one scale per (row, 128-channel chunk)) and `rows_to_planes` (one scale per row) on rows from 2^-40 to 2^40,
  a zero row, a row whose maximum is exactly 2^13 (scale 1) and one whose maximum, 2^-120, lies below the scale pick's clamp.
  (`to_planes(row_index=...)` and `channel_pair_sum_add2_planes` are held bitwise to `to_planes` by tests/test_hip_ops.py.)
* Weight planes: every producer writes fixed records behind its header — f16 forms 2048 bytes (1024 of hi, 1024 of lo), bf16 forms
  3072 bytes (hi, mid, lo) — in which halfword i of each plane belongs to one element.  So, whatever the fragment order, the multiset of
  (hi, lo) / (hi, mid, lo) tuples over the buffer is the model's over all weight elements plus all-zero tuples for the padding.  The f16
  forms carry a 256-byte header: 1 / s, s, bits(max |w|) with s = pick_scale(max |w|) (+ the K22f tag for the Linear entry)."""
import numpy as np
import pytest
import torch

import product_budget as P

pytestmark = pytest.mark.gpu

HDR_BYTES = 256
K22F_TAG = 0x4B323266  # "K22f"


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops

    return hip_ops


def _f16_bits(x, s):
    """The model's (hi, lo) halfwords u16 of x at the scales s (s broadcasts against x)."""
    s = np.broadcast_to(np.asarray(s, dtype=np.float64), x.shape)
    hi, lo = P.split_f16(x, s)  # in x's unit: times s they are the f16 values again, exactly
    return (hi * s).astype(np.float16).view(np.uint16), (lo * s).astype(np.float16).view(np.uint16)


def _bf16_bits(x):
    """The model's (hi, mid, lo) halfwords u16 of x: the top 16 bits of each fp32 piece."""
    return [(p.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16) for p in P.split_bf16(x, 3)]


def _spread_rows(n, c, seed):
    """f32 [n, c]: row i at 2^e_i, e from -40 to 40, every element within 2^-6 of its row's level (log-uniform, either sign); then row 1
    zeros, row 2 with the maximum of its first chunk exactly 2^13, row 3 with its maximum at 2^-120 and nothing below 2^-123."""
    rng = np.random.default_rng(seed)
    e = np.round(np.linspace(-40, 40, n))
    x = np.exp2(rng.uniform(-6.0, 0.0, (n, c)) + e[:, None]) * rng.choice([-1.0, 1.0], (n, c))
    x[1] = 0.0
    x[2] = rng.uniform(0.25, 1.0, c) * 2.0 ** 12 * rng.choice([-1.0, 1.0], c)
    x[2, 3] = -2.0 ** 13
    x[3] = rng.uniform(0.25, 1.0, c) * 2.0 ** -121 * rng.choice([-1.0, 1.0], c)
    x[3, min(10, c - 1)] = 2.0 ** -120
    x = x.astype(np.float32)
    assert (np.abs(x[x != 0]) >= np.finfo(np.float32).tiny).all()
    return x


def _row_plane_halfwords(data, rows, c):
    """u8 plane buffer [rows][c / 8][2][8] f16 -> (hi, lo) u16 [rows, c]."""
    raw = data.cpu().numpy()[: rows * c * 4].view(np.uint16).reshape(rows, c // 8, 2, 8)
    return raw[:, :, 0, :].reshape(rows, c), raw[:, :, 1, :].reshape(rows, c)


def test_to_planes_writes_the_models_halfwords_and_scales(ops, device):
    m, c = 37, 136  # a full 128-channel chunk + a ragged one of 8 channels; 76 teams of 16 threads: five workgroups
    x = _spread_rows(m, c, 11)
    pl = ops.to_planes(torch.from_numpy(x).to(device))
    s = P.x_scales(x, "row_chunk")
    assert float(s[2, 0]) == 1.0 and float(s[3, 0]) == 2.0 ** 126 and float(s[1, 0]) == 1.0  # the cases this test is about
    want_hi, want_lo = _f16_bits(x, s)
    hi, lo = _row_plane_halfwords(pl.data, m + 1, c)
    assert np.array_equal(hi[:m], want_hi) and np.array_equal(lo[:m], want_lo)
    assert not hi[m].any() and not lo[m].any()  # the zero row
    want_inv = np.concatenate([(1.0 / s[:, [0, 128]]).astype(np.float32), np.ones((1, 2), np.float32)], 0)
    got_inv = pl.scales.cpu().numpy()
    assert got_inv.shape == (m + 1, 2) and np.array_equal(got_inv.view(np.uint32), want_inv.view(np.uint32))


def test_rows_to_planes_writes_the_models_halfwords_and_scales(ops, device):
    n, c = 9, 72
    x = _spread_rows(n, c, 12)
    rp = ops.rows_to_planes(torch.from_numpy(x).to(device))
    s = P.x_scales(x, "row")
    assert float(s[2, 0]) == 1.0 and float(s[3, 0]) == 2.0 ** 126 and float(s[1, 0]) == 1.0
    want_hi, want_lo = _f16_bits(x, s)
    hi, lo = _row_plane_halfwords(rp.data, n, c)
    assert np.array_equal(hi, want_hi) and np.array_equal(lo, want_lo)
    want_inv = (1.0 / s[:, 0]).astype(np.float32)
    assert np.array_equal(rp.inv_scales.cpu().numpy()[:n].view(np.uint32), want_inv.view(np.uint32))


# ---- weight planes ---------------------------------------------------------------------------------------------------------------
def _weight(shape, seed, device, unaligned=None):
    """(w f32 numpy, the device tensor).  Seeded normal: no exact zeros.  `unaligned` = 'head' | 'tail': the device tensor is a view one
    float into its allocation (the absmax kernel's 16-byte body then starts 3 elements in and ends before the last one) and the layer's
    maximum sits in the first / the last element — outside the aligned body."""
    w = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    assert (w != 0).all() and np.abs(w).max() < 7.0
    if unaligned:
        w.reshape(-1)[0 if unaligned == "head" else -1] = 7.5 if unaligned == "head" else -7.5
        buf = torch.zeros(w.size + 1, dtype=torch.float32, device=device)
        t = buf[1:].view(*shape)
        t.copy_(torch.from_numpy(w))
        assert t.is_contiguous() and t.data_ptr() % 16 == 4 and (w.size - 3) % 4 != 0
        return w, t
    return w, torch.from_numpy(w).to(device)


def _tuples(body, planes):
    """u8 records of `planes` x 1024 bytes -> sorted u64 keys, one per element slot: halfword i of every plane of a record."""
    rec = body.view(np.uint16).reshape(-1, planes, 512).astype(np.uint64)
    key = rec[:, 0, :]
    for p in range(1, planes):
        key = (key << np.uint64(16)) | rec[:, p, :]
    return np.sort(key.reshape(-1))


def _model_tuples(parts, slots):
    key = parts[0].reshape(-1).astype(np.uint64)
    for p in parts[1:]:
        key = (key << np.uint64(16)) | p.reshape(-1).astype(np.uint64)
    assert (key != 0).all() and slots >= key.size  # (a weight element is never the all-zero tuple: the padding count is unambiguous)
    return np.sort(np.concatenate([key, np.zeros(slots - key.size, np.uint64)]))


F16_ENTRIES = {
    "linear_prepare_weight_f16": ((68, 32), None, lambda ops, t: ops.linear_prepare_weight_f16(t, 68), True),
    "linear_prepare_weight-f16x3": ((68, 40), "head", lambda ops, t: ops.linear_prepare_weight(t, fmt="f16x3"), True),
    "spconv_prepare_weight_split_f16": ((2, 32, 68), None, lambda ops, t: ops.spconv_prepare_weight_split_f16(t), False),
    "spconv_prepare_weight_planes": ((2, 32, 64), "tail", lambda ops, t: ops.spconv_prepare_weight_planes(t), False),
}
BF16_ENTRIES = {
    "linear_prepare_weight-bf16x6": ((20, 40), lambda ops, t: ops.linear_prepare_weight(t, fmt="bf16x6")),
    "linear_prepare_weight_sliced": ((2 * 20, 33), lambda ops, t: ops.linear_prepare_weight_sliced(t, 2, 20)),
    "spconv_prepare_weight_split": ((2, 16, 16), lambda ops, t: ops.spconv_prepare_weight_split(t)),
}


@pytest.mark.parametrize("entry", list(F16_ENTRIES))
def test_f16_weight_planes_hold_the_models_tuples_behind_the_models_header(ops, device, entry):
    shape, unaligned, prepare, tagged = F16_ENTRIES[entry]
    w, t = _weight(shape, 100 + list(F16_ENTRIES).index(entry), device, unaligned)
    buf = prepare(ops, t).cpu().numpy()
    assert buf.dtype == np.uint8 and (buf.size - HDR_BYTES) % 2048 == 0 and buf.size > HDR_BYTES
    amax = np.float32(np.abs(w).max())
    s = float(P.pick_scale(amax))
    hdr = buf[:HDR_BYTES].view(np.uint32)
    want = np.array([1.0 / s, s, amax], np.float32).view(np.uint32)
    assert hdr[:3].tolist() == want.tolist()
    assert not tagged or int(hdr[3]) == K22F_TAG
    body = buf[HDR_BYTES:]
    assert np.array_equal(_tuples(body, 2), _model_tuples(_f16_bits(w, s), body.size // 4))


@pytest.mark.parametrize("entry", list(BF16_ENTRIES))
def test_bf16_weight_planes_hold_the_models_tuples(ops, device, entry):
    shape, prepare = BF16_ENTRIES[entry]
    w, t = _weight(shape, 200 + list(BF16_ENTRIES).index(entry), device)
    buf = prepare(ops, t).cpu().numpy()
    assert buf.dtype == np.uint8 and buf.size % 3072 == 0 and buf.size > 0
    assert np.array_equal(_tuples(buf, 3), _model_tuples(_bf16_bits(w), buf.size // 6))
