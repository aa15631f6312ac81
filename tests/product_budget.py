"""Per-element error budgets for the kernels that reproduce an fp32 product on the f16 / bf16 matrix cores (K9 / K9b / K9c / K9b-XP
sparse convolutions, K22 / K22f / K22h Linear layers, the K10 / K10p weight gradient): seeded input families whose rows, input columns and
output channels differ by 2^12 .. 2^30 in magnitude, the budget each output ELEMENT is held to, numpy emulations of the documented
operand formats and planted defects of the kinds these kernels have had.  A plain module (no fixtures, nothing collected);
tests/test_product_budget_cpu.py shows what the budgets stand on, tests/test_product_budget_gpu.py holds the kernels to them.

Every product is brought to one form, out[o, d] = sum_j X[o, j] W[j, d]:
  Linear            X = x [n, k],                           W = w^T [k, c]
  sparse conv       X = gathered rows [m_out, kvol * cin],  W = weight [kvol * cin, cout]   (a missing neighbour is a row of zeros)
  weight gradient   per offset: X = feat[in_k]^T [cin, P],  W = grad_out[out_k] [P, cout]

The budget of element (o, d), in float64:
  A     = sum_j |X[o, j]| |W[j, d]|
  floor = sum_j eps_x[o, j] |W[j, d]| + |X[o, j]| eps_w[j, d]
  rho32 = max |ref32 - want| / A             ref32: torch's fp32 product of the same operands on the host
  B     = (g + m * max(rho32, 2^-23)) * A + floor
eps is the absolute floor of the f16 hi | lo format, |x s - hi - lo| <= max(2^-22 |x s|, 2^-25): eps = 2^-25 / s with s the power of two
the kernel's header documents (see `SCALE_RULES`); 0 for the exact 3-way bf16 split, for fp32 operands, for an all-zero row (its
planes are exact zeros) and for a missing neighbour.  g = 3 * 2^-22 for the f16-plane kernels (the relative 2^-22 of both operands
and the lo * lo term the header of csrc/spconv_planes.hip says it drops), 0 otherwise.  m is the factor over fp32's own error that
kernel's test in tests/test_hip_ops.py already grants (`SCALE_RULES`).  2^-23 = one rounding of the accumulation + the result's.
B = 0 (the zero row, an output without a neighbour) asks for the exact value."""
import functools

import numpy as np
import torch

MAGS = (2.0 ** -12, 1.0, 2.0 ** 12)  # the three row magnitude classes
ZERO_ROW = 5
K = 64                      # Linear family: input width
LINEAR_N = (96, 129)        # six 16-row groups; a one-row tail after a 128-row block
G_F16 = 3 * 2.0 ** -22
U32 = 2.0 ** -23
EPS_F16 = 2.0 ** -25        # absolute floor of hi + lo in the scaled unit (half the spacing of f16 subnormals)
TOP_EXP = 13                # s * amax in [2^13, 2^14): fmt_pick_scale (csrc/operand_formats.h)
MIN_AMAX_EXP = -113         # ... with amax's exponent clamped from below: s <= 2^126, so that s and 1 / s stay normal fp32 numbers
LNA_KC = 32                 # K22f: the row scale follows the running maximum over 32-column chunks
PLANE_CHUNK = 128           # fsf_to_planes: one scale per (row, 128-channel chunk)
K22F_ADDEND_CAP_EXP = 40    # K22f with a row addend: s_x * s_w <= 2^40
K9BXP_UNIT_CAP_EXP = 60     # K9b-XP: a row's unit s_row <= 2^60
BW_RT = 32                  # K10 / K10p: pairs per stage; the pair range is split when cap > 8 * BW_RT
WGRAD_SPLIT_N = 8 * BW_RT + 1  # smallest pair count of a dense layer (kvol = 1) with nsplit > 1: 257

# kernel -> (x scale rule, weight scale rule, g, m)
SCALE_RULES = {
    "K9": ("fp32", "fp32", 0.0, 2.0),           # fp32 matrix pipe; its test grants no factor: 2
    "K9b": ("bf16x3", "bf16x3", 0.0, 2.0),
    "K9c": ("row_chunk", "layer", G_F16, 4.0),
    "K9b-XP": ("row", "layer", G_F16, 2.0),     # its test grants no factor: 2
    "K22": ("bf16x3", "bf16x3", 0.0, 2.0),
    "K22-grouped": ("bf16x3", "bf16x3", 0.0, 3.0),
    "K22f": ("row_running", "layer", G_F16, 2.0),
    "K22f-grouped": ("row_running", "layer", G_F16, 3.0),
    "K22h": ("row", "layer", G_F16, 8.0),
    "K10": ("fp32", "fp32", 0.0, 2.0),          # fp32 matrix pipe (cin <= 64 or cout <= 64); no test grants it a factor: 2
    "K10p": ("bf16x3", "bf16x3", 0.0, 2.0),     # bf16 matrix cores (cin > 64 and cout > 64): the six terms of K9b / K22, their factor
}


# ------------------------------------------------------------------------------------------------------------------ input families
def _channel_treatment(w_out_last):
    """Output channels ::5 at 2^-10 and 1::7 at 2^-20 of the layer (last axis = output channel), in place."""
    w_out_last[..., ::5] *= 2.0 ** -10
    w_out_last[..., 1::7] *= 2.0 ** -20


def linear_family(n, c, k=K, seed=0):
    """x f32 [n, k], w f32 [c, k], cls i64 [n] (index into MAGS).  Row i at MAGS[i % 3] — every 16-row MFMA group mixes all three —, row 5
    zeros, input columns ::4 at 2^-12 with the matching weight columns at 2^12 (small elements carry as much of the result as large
    ones), output channels ::5 at 2^-10 and 1::7 at 2^-20."""
    rng = np.random.default_rng(1000 * n + c + seed)
    cls = np.arange(n) % 3
    x = rng.standard_normal((n, k)) * np.asarray(MAGS)[cls][:, None]
    if n > ZERO_ROW:
        x[ZERO_ROW] = 0.0
    x[:, ::4] *= 2.0 ** -12
    w = rng.standard_normal((c, k)) / np.sqrt(k)
    w[:, ::4] *= 2.0 ** 12
    wt = w.T  # a view: [k, c]
    _channel_treatment(wt)
    return x.astype(np.float32), w.astype(np.float32), cls


GRID = (8, 24, 24)
ISLAND = (1, 2, 3)
PITCH = 5
Z_LAYERS = (1, 5)
ISLANDS_PER_LAYER = (15, 11)   # y starts 0, 5, ..., x starts 0, 5, 10: x <= 12
PATCH = (5, 9, 16, 6)          # z, y0, x0, side: three empty cells away from every island


def sparse_sites():
    """idx i32 [m, 4] (b, z, y, x) sorted by (z, y, x), island i64 [m] (-1 = the dense patch), cls i64 [m]: 26 islands of 1 x 2 x 3 sites
    on a pitch of 5 (two z layers four cells apart: with a 3 x 3 x 3 kernel an island's outputs depend on that island alone), one
    magnitude class per island cycling island to island, and a 6 x 6 patch whose sites cycle through the classes: 192 rows."""
    rows = []
    isl = 0
    for z, count in zip(Z_LAYERS, ISLANDS_PER_LAYER):
        for i in range(count):
            y0, x0 = PITCH * (i // 3), PITCH * (i % 3)
            for dy in range(ISLAND[1]):
                for dx in range(ISLAND[2]):
                    rows.append((0, z, y0 + dy, x0 + dx, isl, isl % 3))
            isl += 1
    pz, py, px, side = PATCH
    for dy in range(side):
        for dx in range(side):
            rows.append((0, pz, py + dy, px + dx, -1, (dy * side + dx + dy) % 3))
    a = np.array(sorted(rows, key=lambda r: (r[1], r[2], r[3])), dtype=np.int64)
    return a[:, :4].astype(np.int32), a[:, 4], a[:, 5]


def conv_tables():
    """{name: (nbr i32 [m_out, 27], m_in)} from the host rulebook (tests/test_hip_ops.py holds the device rulebooks bit-equal to it):
    submanifold 3 x 3 x 3, the stride-2 convolution and its inverse (m_in != m_out)."""
    from oracle import spconv as osp

    idx, _, _ = sparse_sites()
    m = idx.shape[0]
    _, pairs, _ = osp.build_rulebook(idx, 1, GRID, (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), True)
    out_idx, spairs, _ = osp.build_rulebook(idx, 1, GRID, (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1), False)
    mo = out_idx.shape[0]
    return {"subm": (osp.pairs_to_nbr(pairs, m), m), "strided": (osp.pairs_to_nbr(spairs, mo), m),
            "inverse": (osp.pairs_inverse_nbr(spairs, m), mo)}


def conv_family(table, cin, cout, seed=0):
    """feat f32 [m_in, cin], w f32 [27, cin, cout], cls i64 [m_in] for a table of `conv_tables()`.  The rows of the fine level carry their
    island's class; the coarse rows the inverse table reads cycle through the classes row by row.  Input columns ::4 at 2^-12 against
    weight rows at 2^12, output channels as in the Linear family."""
    _, m_in = conv_tables()[table]
    rng = np.random.default_rng(77 + cin * 1000 + cout + seed + {"subm": 0, "strided": 1, "inverse": 2}[table] * 100000)
    cls = sparse_sites()[2] if table != "inverse" else np.arange(m_in) % 3
    feat = rng.standard_normal((m_in, cin)) * np.asarray(MAGS)[cls][:, None]
    feat[ZERO_ROW] = 0.0
    feat[:, ::4] *= 2.0 ** -12
    w = rng.standard_normal((27, cin, cout)) / np.sqrt(cin * 6)
    w[:, ::4, :] *= 2.0 ** 12
    _channel_treatment(w)
    return feat.astype(np.float32), w.astype(np.float32), cls


def wgrad_family(m_in, m_out, cin, cout, cls_in, seed=0):
    """feat f32 [m_in, cin], gout f32 [m_out, cout]: rows at their class's magnitude, input columns ::4 and grad-out columns ::5 at 2^-12 —
    the small entries of grad_W are whole rows and columns of it."""
    rng = np.random.default_rng(555 + m_in * 7 + m_out + cin + cout + seed)
    feat = rng.standard_normal((m_in, cin)) * np.asarray(MAGS)[cls_in][:, None]
    feat[ZERO_ROW] = 0.0
    feat[:, ::4] *= 2.0 ** -12
    gout = rng.standard_normal((m_out, cout)) * np.asarray(MAGS)[(np.arange(m_out) // 6 + 1) % 3][:, None]
    gout[:, ::5] *= 2.0 ** -12
    return feat.astype(np.float32), gout.astype(np.float32)


def dense_rows_classes(n):
    """Classes of n rows laid out like the sparse family's islands: six consecutive rows share one."""
    return (np.arange(n) // 6) % 3


# ------------------------------------------------------------------------------------------------------------------ the formats
def pick_scale(amax):
    """The power of two s with s * amax in [2^13, 2^14) (s = 1 for amax = 0; s = 2^126 for amax < 2^-113: the kernel's clamp), float64,
    elementwise."""
    amax = np.asarray(amax, dtype=np.float64)
    _, ex = np.frexp(np.where(amax > 0, amax, 1.0))  # amax = f * 2^ex, f in [0.5, 1): floor(log2) = ex - 1
    return np.where(amax > 0, np.exp2(TOP_EXP - np.maximum(ex - 1, MIN_AMAX_EXP).astype(np.float64)), 1.0)


def x_scales(x, rule, group=16):
    """s [n, c] float64 for the rows of x under a scale rule: 'row' (fsf_rows_to_planes: K22h, K9b-XP), 'row_chunk' (fsf_to_planes: per
    128-channel chunk, K9c), 'row_running' (K22f: the running maximum over 32-column chunks; the scale may only fall), and the planted
    defect 'group' (one scale per 16-row group)."""
    a = np.abs(x.astype(np.float64))
    n, c = a.shape
    if rule == "row":
        amax = np.broadcast_to(a.max(1, keepdims=True), a.shape)
    elif rule == "row_chunk":
        amax = np.concatenate([np.broadcast_to(a[:, s:s + PLANE_CHUNK].max(1, keepdims=True), a[:, s:s + PLANE_CHUNK].shape)
                               for s in range(0, c, PLANE_CHUNK)], 1)
    elif rule == "row_running":
        run = np.maximum.accumulate(np.stack([a[:, s:s + LNA_KC].max(1) for s in range(0, c, LNA_KC)], 1), 1)
        amax = np.repeat(run, LNA_KC, 1)[:, :c]
    elif isinstance(rule, tuple):  # ("sources", cins): K9c's channel concatenation, every source converted by fsf_to_planes on its own
        return np.concatenate([x_scales(x[:, o:o + w], "row_chunk") for o, w in zip(np.cumsum((0,) + rule[1][:-1]), rule[1])], 1)
    elif rule == "group":
        rmax = a.max(1)
        gmax = np.concatenate([np.full(min(group, n - s), rmax[s:s + group].max()) for s in range(0, n, group)])
        amax = np.broadcast_to(gmax[:, None], a.shape)
    else:
        raise ValueError(rule)
    return pick_scale(amax)


def split_f16(x, s):
    """(hi, lo) float64 in x's own unit: hi = rn_f16(x s), lo = rn_f16(x s - hi), the products and the difference formed in fp32."""
    xs = (x.astype(np.float64) * s).astype(np.float32)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64) / s, lo.astype(np.float64) / s


def split_bf16(x, parts=3):
    """The truncating bf16 split of fp32 values: [hi, mid, lo] float64 (3 parts: exact), or [hi, mid] (the planted 2-way split)."""
    out = []
    r = np.ascontiguousarray(x, dtype=np.float32)
    for _ in range(parts):
        p = (r.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
        out.append(p.astype(np.float64))
        r = (r - p).astype(np.float32)
    return out


def eps_of(x, rule, s=None):
    """The absolute floor of each element of x under a rule (float64, x's shape): 2^-25 / s for the f16 formats — 0 on an all-zero row,
    whose planes are exact zeros —, 0 for 'bf16x3' and 'fp32'."""
    if rule in ("bf16x3", "fp32"):
        return np.zeros(x.shape, dtype=np.float64)
    if rule == "layer":
        return np.full(x.shape, EPS_F16 / float(pick_scale(np.abs(x).max())), dtype=np.float64)
    s = x_scales(x, rule) if s is None else s
    return np.where(np.abs(x).max(-1, keepdims=True) > 0, EPS_F16 / s, 0.0)


# ------------------------------------------------------------------------------------------------------------------ products
class Product:
    """One product in the common form: X float64 [o, j], W float64 [j, d], with the gather that made X (for emulations that split the
    rows before they are gathered).  `rows(p)` maps a per-input-row array p [m_in, cin] to X's layout."""

    def __init__(self, x, w2d, rows, addend=None):
        self.x, self.w, self.rows, self.addend = x, w2d.astype(np.float64), rows, addend
        self.X = rows(x.astype(np.float64))

    def want(self):
        y = self.X @ self.w
        return y if self.addend is None else y + self.addend.astype(np.float64)

    def ref32(self):
        """torch's fp32 product of the same operands on the host."""
        y = torch.from_numpy(self.rows(x_as32(self.x)).astype(np.float32)) @ torch.from_numpy(self.w.astype(np.float32))
        if self.addend is not None:
            y = y + torch.from_numpy(self.addend)
        return y.numpy().astype(np.float64)


def x_as32(x):
    return np.asarray(x, dtype=np.float32)


def linear_product(x, w, addend=None):
    return Product(x, w.astype(np.float64).T, lambda p: p, addend)


def conv_product(feat, w, nbr):
    kvol, cin, cout = w.shape
    nb = np.asarray(nbr).astype(np.int64)

    def rows(p):
        g = np.where((nb >= 0)[:, :, None], p[np.clip(nb, 0, None)], np.zeros((), dtype=p.dtype))
        return g.reshape(nb.shape[0], kvol * p.shape[1])

    # (two-source K9c: `feat` is the channel concatenation; the weight rows follow the same (offset, channel) order)
    return Product(feat, w.astype(np.float64).reshape(kvol * cin, cout), rows)


def wgrad_product(feat, gout, in_rows, out_rows):
    """grad_W[k] = feat[in_rows]^T gout[out_rows] for the pairs of one offset."""
    return Product(feat, gout.astype(np.float64)[out_rows], lambda p: p[in_rows].T)


class Budget:
    def __init__(self, prod, kernel, x_rule=None, eps_x_rows=None):
        xr, wr, self.g, self.m = SCALE_RULES[kernel]
        xr = x_rule or xr
        self.kernel, self.prod = kernel, prod
        self.want = prod.want()
        self.A = np.abs(prod.X) @ np.abs(prod.w)
        if prod.addend is not None:
            self.A = self.A + np.abs(prod.addend.astype(np.float64))
        ex = prod.rows(eps_of(prod.x, xr) if eps_x_rows is None else eps_x_rows)
        self.floor = ex @ np.abs(prod.w) + np.abs(prod.X) @ eps_of(prod.w, wr)
        self.err32 = np.abs(prod.ref32() - self.want)
        self.rho32 = float((self.err32[self.A > 0] / self.A[self.A > 0]).max()) if (self.A > 0).any() else 0.0
        self.rel = self.g + self.m * max(self.rho32, U32)
        self.B = self.rel * self.A + self.floor

    def floor_dominated(self):
        """The outputs whose floor exceeds (g + m 2^-23) A: where the format's floor, not the arithmetic, sets the budget."""
        return self.floor > (self.g + self.m * U32) * self.A

    def floor_share(self):
        return float(self.floor_dominated().mean())

    def with_epilogue(self, scale, shift, res):
        """(want, B) of scale * y + shift + res, per output channel scale / shift f64 [d], res f64 [o, d] or None."""
        r = 0.0 if res is None else res
        want = self.want * scale + shift + r
        return want, np.abs(scale) * self.B + U32 * (np.abs(scale * self.want) + np.abs(shift) + np.abs(r))

    def worst(self, got, want=None, B=None):
        """(max err / B, (row, channel)) — inf where B = 0 and the value is not exact."""
        want = self.want if want is None else want
        B = self.B if B is None else B
        err = np.abs(np.asarray(got, dtype=np.float64) - want)
        ratio = np.where(B > 0, err / np.where(B > 0, B, 1.0), np.where(err > 0, np.inf, 0.0))
        at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        return float(ratio[at]), (int(at[0]), int(at[1]))

    def today(self, got, factor=None):
        """The batch-maximum criterion of tests/test_hip_ops.py on the same data: err <= max(m * err32, 2e-6 * scale)."""
        err = float(np.abs(np.asarray(got, dtype=np.float64) - self.want).max())
        scale = max(1.0, float(np.abs(self.want).max()))
        return err <= max((factor or self.m) * float(self.err32.max()), 2e-6 * scale), err / scale


# ------------------------------------------------------------------------------------------------------------------ emulations
def emulate_f16(prod, x_rule="row", defect=None):
    """The documented f16 hi | lo arithmetic in float64: rows split under `x_rule` before the gather, the weights with the layer's scale,
    hi hi + hi lo + lo hi.  Planted defects: 'group_scale' (one x scale per 16-row group), 'drop_lo' (the lo plane of x dropped on the
    rows more than 2^6 below their 16-row group's maximum: the small rows)."""
    x = prod.x
    s = x_scales(x, "group" if defect == "group_scale" else x_rule)
    xh, xl = split_f16(x, s)
    if defect == "drop_lo":
        rmax = np.abs(x).max(1)
        gmax = np.concatenate([np.full(min(16, len(rmax) - i), rmax[i:i + 16].max()) for i in range(0, len(rmax), 16)])
        xl = np.where((rmax < gmax * 2.0 ** -6)[:, None], 0.0, xl)
    wh, wl = split_f16(prod.w, pick_scale(np.abs(prod.w).max()))
    y = prod.rows(xh) @ wh + prod.rows(xh) @ wl + prod.rows(xl) @ wh
    return y if prod.addend is None else y + prod.addend.astype(np.float64)


BF16_TERMS = ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))  # (piece of X, piece of W): 0 = hi, 1 = mid, 2 = lo


def emulate_bf16(prod, parts=3, drop=None):
    """The bf16 split in float64: the six leading cross terms of the exact 3-way split, or every term of a 2-way split (planted).
    `drop=(i, j)`: the planted defect of one cross term left out."""
    xs = [prod.rows(p) for p in split_bf16(prod.x, parts)]
    ws = split_bf16(prod.w, parts)
    terms = list(BF16_TERMS) if parts == 3 else [(0, 0), (0, 1), (1, 0), (1, 1)]
    if drop is not None:
        terms.remove(tuple(drop))
    y = sum(xs[i] @ ws[j] for i, j in terms)
    return y if prod.addend is None else y + prod.addend.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ the cases
# name -> (kernel, c, slice_c, addend).  c: the smallest width the kernel's gate admits (K22: c % 4 == 0; K22f: c > 32; K22h: a slice of more
# than 64 channels), 68, the width with enough plain, 2^-10 and 2^-20 channels side by side, and 256 = two 128-channel slices.
LINEAR_CASES = {
    "K22-c4": ("K22", 4, None, False), "K22-c68": ("K22", 68, None, False), "K22-c256": ("K22", 256, None, False),
    "K22-add-c68": ("K22-grouped", 68, None, True),
    "K22f-c36": ("K22f", 36, None, False), "K22f-c68": ("K22f", 68, None, False), "K22f-c256": ("K22f", 256, None, False),
    "K22f-add-c36": ("K22f-grouped", 36, None, True), "K22f-add-c68": ("K22f-grouped", 68, None, True),
    "K22h-c68": ("K22h", 68, 68, False), "K22h-c256": ("K22h", 256, 128, False),
}
# name -> (kernel, cins, cout): K9c takes 32 .. 128 channels per source and 64 or n * 128 output channels, K9b-XP more than 64
# (K9c-c256: two 128-channel chunks in the output, whose plane form carries one scale per (row, chunk))
CONV_CASES = {"K9": ("K9", (32,), 68), "K9b": ("K9b", (32,), 68), "K9c": ("K9c", (32,), 64), "K9c-2src": ("K9c", (32, 32), 64),
              "K9c-c256": ("K9c", (32,), 256), "K9b-XP": ("K9b-XP", (32,), 68)}
CONV_TABLES = {"K9": ("subm", "strided", "inverse"), "K9b": ("subm",), "K9c": ("subm", "strided", "inverse"), "K9c-2src": ("subm",),
               "K9c-c256": ("subm",), "K9b-XP": ("subm",)}
WGRAD_CIN, WGRAD_COUT = 32, 68
ADD_ROWS = 9  # the addend table: row j at MAGS[j % 3], read by row i as j = i % 9 — an addend of the row's own magnitude


@functools.lru_cache(maxsize=None)
def linear_case(name, n):
    """x, w, cls, addend table / index (or None), the product and its budget — computed once, never modified."""
    kernel, c, slice_c, addend = LINEAR_CASES[name]
    x, w, cls = linear_family(n, c)
    table = index = add = None
    if addend:
        rng = np.random.default_rng(9 * n + c)
        table = rng.standard_normal((ADD_ROWS, c)) * np.asarray(MAGS)[np.arange(ADD_ROWS) % 3][:, None]
        _channel_treatment(table)
        table = table.astype(np.float32)
        index = (np.arange(n) % ADD_ROWS).astype(np.int64)
        add = table[index]
    prod = linear_product(x, w, add)
    return dict(kernel=kernel, c=c, slice_c=slice_c, x=x, w=w, cls=cls, table=table, index=index, prod=prod, budget=Budget(prod, kernel))


def conv_x_rule(name):
    kernel, cins, _ = CONV_CASES[name]
    return ("sources", cins) if kernel == "K9c" else SCALE_RULES[kernel][0]


@functools.lru_cache(maxsize=None)
def conv_case(name, table):
    kernel, cins, cout = CONV_CASES[name]
    feat, w, cls = conv_family(table, sum(cins), cout)
    nbr = conv_tables()[table][0]
    prod = conv_product(feat, w, nbr)
    return dict(kernel=kernel, cins=cins, cout=cout, feat=feat, w=w, cls=cls, nbr=nbr, prod=prod,
                budget=Budget(prod, kernel, x_rule=conv_x_rule(name)))


class StackedBudget(Budget):
    """The budgets of the 27 offsets of a weight gradient as one [kvol * cin, cout] array, with ONE rho32: the largest of the offsets'."""

    def __init__(self, parts):
        self.kernel, self.g, self.m = parts[0].kernel, parts[0].g, parts[0].m
        self.want, self.A, self.floor, self.err32 = (np.concatenate([getattr(p, f) for p in parts], 0) for f in ("want", "A", "floor", "err32"))
        self.rho32 = max(p.rho32 for p in parts)
        self.rel = self.g + self.m * max(self.rho32, U32)
        self.B = self.rel * self.A + self.floor


def wgrad_pair_capacity(table):
    """The pair capacity K10p plans with: rulebook_to_pairs sizes every offset's list for m_out pairs; a dense layer has n."""
    return int(table[6:]) if table.startswith("dense-") else conv_tables()[table][0].shape[0]


def wgrad_plan(cap, cin, cout, kvol):
    """bwd_plan of csrc/spconv_bwd.hip (its lines are pinned by tests/test_product_budget_cpu.py): (ta, tb, tiles_a, tiles_b, nsplit,
    range) — the channel tile, the channel tiles per side, into how many ranges an offset's pair list is split, pairs per range."""
    cdiv = lambda a, b: -(-a // b)
    ta, tb = 64 if cin <= 64 else 128, 64 if cout <= 64 else 128
    tiles = cdiv(cin, ta) * cdiv(cout, tb)
    s = max(1, min(cdiv(6144 if kvol >= 8 else 512, kvol * tiles), cdiv(cap, 8 * BW_RT)))
    r = max(BW_RT, cdiv(cdiv(cap, s), BW_RT) * BW_RT)
    return ta, tb, cdiv(cin, ta), cdiv(cout, tb), cdiv(max(cap, 1), r), r


def wgrad_nsplit(cap, cin, cout, kvol):
    """Into how many ranges the weight gradient splits an offset's pair list."""
    return wgrad_plan(cap, cin, cout, kvol)[4]


def wgrad_kernel(cin, cout):
    """Which kernel fsf_spconv_backward_weight launches: `if (cap > 0 && ta == 128 && tb == 128)` is the bf16 one."""
    ta, tb = wgrad_plan(1, cin, cout, 1)[:2]
    return "K10p" if ta == 128 and tb == 128 else "K10"


@functools.lru_cache(maxsize=None)
def wgrad_case(table, cin=WGRAD_CIN, cout=WGRAD_COUT, absolute=False):
    """spconv_backward_weight on a table of the sparse family; 'dense-<n>': linear_backward_weight (identity pairs) on n rows — 192 = the
    family's rows, WGRAD_SPLIT_N = the first pair count at which the pair range of a dense layer is split.  Which cases split is
    `wgrad_nsplit(wgrad_pair_capacity(table), ...)`, asserted in tests/test_product_budget_cpu.py.  The channel counts pick the kernel
    (`wgrad_kernel`) and with it the budget's rule.  `absolute`: both operands replaced by their absolute values — the truncating split
    keeps the sign, so every piece is then non-negative and whatever a dropped cross term leaves out adds up coherently."""
    if table.startswith("dense-"):
        n = int(table[6:])
        cls = sparse_sites()[2] if n == sparse_sites()[0].shape[0] else dense_rows_classes(n)
        feat, gout = wgrad_family(n, n, cin, cout, cls)
        nbr = np.arange(n, dtype=np.int32)[:, None]
    else:
        nbr, m_in = conv_tables()[table]
        cls = sparse_sites()[2] if table != "inverse" else np.arange(m_in) % 3
        feat, gout = wgrad_family(m_in, nbr.shape[0], cin, cout, cls)
    if absolute:
        feat, gout = np.abs(feat), np.abs(gout)
    kernel = wgrad_kernel(cin, cout)
    parts = []
    for k in range(nbr.shape[1]):
        out_rows = np.nonzero(nbr[:, k] >= 0)[0]
        parts.append(Budget(wgrad_product(feat, gout, nbr[out_rows, k].astype(np.int64), out_rows), kernel))
    return dict(kernel=kernel, cin=cin, cout=cout, feat=feat, gout=gout, cls=cls, nbr=nbr, parts=parts, budget=StackedBudget(parts))


WGRAD_TABLES = ("subm", "strided", "inverse", "dense-192", "dense-%d" % WGRAD_SPLIT_N)
K10P_SHAPES = ((68, 68), (132, 68))  # one partial 128 x 128 tile; two `a` tiles
K10P_CASES = tuple((t, cin, cout, ab) for ab in (False, True) for cin, cout in K10P_SHAPES for t in WGRAD_TABLES)


def wgrad_emulate_bf16(c, drop=None):
    """The stacked [kvol * cin, cout] result of the six-term bf16 arithmetic on a `wgrad_case`, with one cross term left out (`drop`)."""
    return np.concatenate([emulate_bf16(p.prod, 3, drop) for p in c["parts"]], 0)


def class_name(c):
    return ("2^-12", "1", "2^12")[int(c)]
