"""Cases for the norm kernels (K12: fullysparsefusion_amd/csrc/norm_act.hip, K23: csrc/batch_norm.hip) that reach the kernels'
decisions one by one, and the referees they are judged by: shared by tests/test_norm_cases_cpu.py (the source pin, the reachability
table, the referee against a plain loop, numpy models of both reduction schemes with switchable defects) and tests/test_norm_gpu.py.
No GPU and no product import here.

The dispatch rules of fsf_norm_act / fsf_norm_act_backward (which kernel, rows per workgroup, grid caps) and of K23 (cs_cw_log2,
cs_blocks, the ry * 4 rows of bn_rows_kernel, the 64 / 16 steps of the fold kernels) are restated below and pinned to the kernel text
by test_norm_cases_cpu.py::test_constants_and_rules_equal_the_kernel_source.  Every case is generated from its name and states the
decisions it reaches (`tags`).

Value families and how they are judged
* ints      integers uniform in [-8, 8] without 0; every partial sum of a column stays below 2^24 (asserted), so fp32 column sums are
            exact in ANY order: column sums, grad_beta of K12 with act=None and grad_beta of K23 are compared bit for bit with an
            integer referee.  The mean is fp32(sum) * (1.0f / (float)n): one fp32 product, as the kernel forms it.
* balanced  `ints` arranged so that every column sums to 0: the device mean is exactly 0, the squared deviations are integers and the
            variance is fp32(sum of squares) * fp32(1 / n) bit for bit; invstd, scale, shift and the running statistics follow from it
            in correctly rounded steps the host repeats.
* exact     (K23 backward) integer x and grad_out, an integer mean, a power-of-two invstd, dyadic scale / shift: fma(x, scale, shift)
            is exact (and exactly 0 in places: the mask must be `> 0`), so grad_gamma, grad_beta and the mask are bit-exact; grad_x is
            bit-exact where n is a power of two (asserted by replaying every step in fp32), elsewhere it is held per element to
            `bn_grad_x_bound`.
* normal    standard_normal * exp(standard_normal) per row; normal_off the same plus 1000 (two passes: no E[x^2] - E[x]^2).  Judged
            per element against float64 with the budgets of `fwd_reference` / `bwd_reference`; their constants K_FWD, K_GX, K_COL come
            from torch's own fp32 composition on the host (twice the largest ratio seen, floor 4; test_norm_cases_cpu.py measures them
            again), never from a kernel's output.
ReLU in the backward: where the float64 pre-activation is within MASK_MARGIN budgets of 0 the case's grad_out is 0, so that the mask is
unambiguous; channels 0 and c // 2 of a ReLU case have gamma = beta = 0, where the pre-activation is exactly 0 and `>` differs from `>=`.
NaN and infinite inputs are out of scope, and so is the SyncBN cross-rank path (it keeps its tests in tests/test_hip_ops.py).

Cases are built one at a time (`case(name)`, a small cache) and must not be written to."""
import functools
import zlib
from typing import NamedTuple

import numpy as np
import torch

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24
POISON = F32(1e30)
assert np.finfo(np.longdouble).nmant >= 63  # (the fma of the running statistics is replayed in extended precision)

# restated from csrc/norm_act.hip and csrc/batch_norm.hip
NA_MAX_PER_LANE = 8
NA_MAX_C = 64 * 16        # above: FSF_ERR_UNSUPPORTED
FWD_CAP_V4 = 8192         # workgroups of the 16-byte forward
FWD_CAP_SCALAR = 16384
NA_BWD_BLOCKS = 1024
CS_BLOCKS = 1024
FOLD_SLICES = 16          # slices of the fold kernels: slice s adds partials s, s + 16, ...
FOLD_STEP = 64            # ... four at a time
GELU_FWD_ABS = 6e-8       # fsf_gelu against float64 erf, beyond the rounding (docs/parity_details.md)
ERF_BWD_ABS = 1.5e-7      # Abramowitz & Stegun 7.1.26 as the backward uses it
GELU_LIP = 1.13           # max |gelu'|
GELU_CURV = 0.8           # max |gelu''| = 2 phi(0)

# measured on the host (torch fp32 against float64 over all `normal` cases): twice the largest ratio, floor 4
K_FWD = 5.4
K_GX = 15.0
K_COL = 4.0
MASK_MARGIN = 4.0         # budgets of the forward pre-activation a ReLU backward case stays away from 0


def cdiv(a, b):
    return -(-a // b)


class Kern(NamedTuple):
    form: str   # "v4" (16-byte lanes) or "s" (scalar)
    team: int   # lanes per row
    pl: int     # PLV float4 (v4) or PL floats (scalar) per lane
    ru: int     # rows of a team in flight

    @property
    def rows_per_wg(self):
        return 256 // self.team * self.ru

    @property
    def slots(self):
        """Channels the lanes of a team hold: the padded width."""
        return self.team * self.pl * (4 if self.form == "v4" else 1)

    @property
    def name(self):
        return f"{self.form}_t{self.team}_p{self.pl}_r{self.ru}"


def fwd_kernel(c, v4):
    if c > NA_MAX_C:
        return None
    if v4:
        c4 = c // 4
        return Kern("v4", 16, 1, 2) if c4 <= 16 else Kern("v4", 32, 1, 2) if c4 <= 32 else Kern("v4", 64, 1, 2) if c4 <= 64 else \
            Kern("v4", 64, 2, 1) if c4 <= 128 else Kern("v4", 64, 4, 1)
    if c > 64 * NA_MAX_PER_LANE:
        return Kern("s", 64, 16, 1)
    return Kern("s", 16, 8, 1) if c <= 64 else Kern("s", 32, 8, 1) if c <= 128 else Kern("s", 64, 8, 1)


def bwd_kernel(c, v4):
    if c > NA_MAX_C or (c > 64 * NA_MAX_PER_LANE and not v4):
        return None
    if v4:
        c4 = c // 4
        return Kern("v4", 16, 1, 2) if c4 <= 16 else Kern("v4", 32, 1, 2) if c4 <= 32 else Kern("v4", 64, 1, 1) if c4 <= 64 else \
            Kern("v4", 64, 2, 1) if c4 <= 128 else Kern("v4", 64, 4, 1)
    return Kern("s", 16, 8, 1) if c <= 64 else Kern("s", 32, 8, 1) if c <= 128 else Kern("s", 64, 8, 1)


def fwd_cap(k):
    return FWD_CAP_V4 if k.form == "v4" else FWD_CAP_SCALAR


def grid(n, k, cap):
    return max(1, min(cap, cdiv(n, k.rows_per_wg)))


def cs_cw_log2(c):
    l = 0
    while (1 << l) < c and l < 8:
        l += 1
    return l


def cs_ry(c):
    return 256 >> cs_cw_log2(c)


def cs_blocks(n, c):
    """(workgroups, rows per workgroup) of column_stats_kernel."""
    rpb = max(cdiv(n, CS_BLOCKS), 8 * cs_ry(c))
    return cdiv(n, rpb), rpb


def bn_rows_per_block(c):
    return 4 * cs_ry(c)


# ---- layouts: how the tensors are handed over ------------------------------------------------------------------------------------------

class Layout(NamedTuple):
    x_off: int = 0     # floats the row-major x (and, in the backward, grad_out for "go_off1") starts after a 16-byte boundary
    go_off: int = 0
    gb_off: int = 0    # the same for gamma and beta
    pad: int = 0       # out = buf[:, out_off : out_off + c] of a [n, c + pad] buffer
    out_off: int = 0


LAYOUTS = {
    "plain": Layout(),
    "x_off1": Layout(x_off=1),
    "go_off1": Layout(go_off=1),
    "gb_off1": Layout(gb_off=1),
    "out_col1": Layout(pad=4, out_off=1),     # stride still a multiple of 4: only the pointer is off
    "out_stride_c2": Layout(pad=2),           # pointer aligned, stride c + 2
    "out_aligned": Layout(pad=8, out_off=4),  # a slice that keeps the 16-byte form
}
FWD_FALLBACKS = ("x_off1", "out_col1", "out_stride_c2", "gb_off1")
BWD_FALLBACKS = ("x_off1", "go_off1", "gb_off1")


def is_v4(c, layout, affine):
    lay = LAYOUTS[layout]
    return c % 4 == 0 and (c + lay.pad) % 4 == 0 and lay.x_off % 4 == 0 and lay.go_off % 4 == 0 and lay.out_off % 4 == 0 and \
        (not affine or lay.gb_off % 4 == 0)


# ---- K12 specs ---------------------------------------------------------------------------------------------------------------------------

V4_WIDTHS = (4, 64, 68, 128, 132, 256, 260, 512, 516, 1024)
SCALAR_WIDTHS = (1, 3, 65, 127, 129, 511, 513, 1023)
FALLBACK_WIDTHS = (64, 128, 260, 516)          # scalar t16, t32, t64 and t64 / PL 16 by misalignment
FORMS = ("lna", "ln", "aff")                   # LayerNorm with affine, LayerNorm without, per-channel affine only
ACTS = ("none", "relu", "gelu")
FOLD_BLOCKS = (1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 1023, 1024)
FAMILIES_N = ("normal", "normal_off")

FWD_SPECS = {}   # name -> (c, n, form, act, layout, family)
BWD_SPECS = {}   # name -> (c, n, affine, act, layout, family)


def _fwd(c, n, form, act, layout="plain", family="normal"):
    FWD_SPECS[f"fwd-c{c}-n{n}-{form}-{act}-{layout}-{family}"] = (c, n, form, act, layout, family)


def _bwd(c, n, affine, act, layout="plain", family="normal"):
    BWD_SPECS[f"bwd-c{c}-n{n}-{'lna' if affine else 'ln'}-{act}-{layout}-{family}"] = (c, n, affine, act, layout, family)


def _make_specs():
    i = 0
    for c in V4_WIDTHS + SCALAR_WIDTHS:
        k = fwd_kernel(c, c % 4 == 0)
        rpw = k.rows_per_wg
        for form in FORMS:          # every template instantiation of the width's kernel, two workgroups, the last with one row
            for act in ACTS:
                _fwd(c, rpw + 1, form, act, family=FAMILIES_N[i % 2])
                i += 1
        for n in (1, rpw - 1, rpw, 2 * rpw + 3):
            _fwd(c, n, FORMS[i % 3], ACTS[i % 3 if n > 1 else (i // 3) % 3], family=FAMILIES_N[i % 2])
            i += 1
    for c in FALLBACK_WIDTHS:
        rpw = fwd_kernel(c, False).rows_per_wg
        for layout in FWD_FALLBACKS + ("out_aligned",):
            for form, act in (("lna", "gelu"), ("aff", "relu")) + ((("ln", "none"),) if layout != "gb_off1" else ()):
                _fwd(c, 2 * rpw + 1, form, act, layout, FAMILIES_N[i % 2])
                i += 1
    for c, layout in ((65, "out_col1"), (129, "out_aligned"), (3, "out_stride_c2"), (513, "x_off1")):  # slices of the scalar widths
        _fwd(c, 19, "lna", "gelu", layout)
    for c, v4 in ((4, True), (68, True), (132, True), (260, True), (516, True), (1, False), (65, False), (129, False), (513, False)):
        k = fwd_kernel(c, v4)       # the second trip of the grid-stride loop: one row beyond the capped grid
        _fwd(c, fwd_cap(k) * k.rows_per_wg + 1, "ln", "relu" if c > 4 else "gelu", family="normal")
    _fwd(64, FWD_CAP_SCALAR * 16 + 1, "ln", "none", "x_off1")  # ... and of a scalar kernel reached by misalignment

    for c in V4_WIDTHS + (3, 65, 133, 1, 127, 511):
        k = bwd_kernel(c, c % 4 == 0)
        rpw = k.rows_per_wg
        for act in ACTS:
            _bwd(c, rpw + 1, True, act, family=FAMILIES_N[i % 2])
            i += 1
        _bwd(c, 2 * rpw + 3, False, ACTS[i % 3], family=FAMILIES_N[i % 2])
        _bwd(c, 1, True, ACTS[(i + 1) % 3])
        _bwd(c, rpw - 1, True, "none", family="ints")
        _bwd(c, 1024 * rpw + 1, True, "none", family="ints")  # the second trip: exact grad_beta
        i += 1
    for c in (64, 128, 260):
        rpw = bwd_kernel(c, False).rows_per_wg
        for layout in BWD_FALLBACKS:
            for act in ACTS:
                _bwd(c, 2 * rpw + 1, True, act, layout, FAMILIES_N[i % 2])
                i += 1
            _bwd(c, 3 * rpw + 1, True, "none", layout, "ints")
        _bwd(c, 2 * rpw + 1, False, "gelu", "x_off1")
    for c, layout in ((4, "plain"), (3, "plain"), (64, "x_off1")):  # the fold at every step of its loop
        rpw = bwd_kernel(c, is_v4(c, layout, True)).rows_per_wg
        for b in FOLD_BLOCKS:
            _bwd(c, b * rpw - (b % 2), True, "none", layout, "ints")  # (the last workgroup full or one row short: odd n for RU = 2)
    for b in (17, 48, 49):
        _bwd(132, b * 4, True, "relu", family="ints")
    for c in (4, 3, 132):
        _bwd(c, 0, True, "gelu")
        _bwd(c, 0, False, "none")


_make_specs()
FWD_NAMES = tuple(FWD_SPECS)
BWD_NAMES = tuple(BWD_SPECS)
FWD_UNSUPPORTED = (1025,)                    # FSF_ERR_UNSUPPORTED whatever the alignment
BWD_UNSUPPORTED = ((1025, "plain"), (516, "x_off1"), (1024, "gb_off1"), (513, "plain"))


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _values(rng, n, c, family):
    if family == "ints":
        v = rng.integers(1, 9, (n, c)) * rng.choice((-1, 1), (n, c))
        return v.astype(F32)
    x = rng.standard_normal((n, c), dtype=F32) * np.exp(rng.standard_normal((n, 1), dtype=F32))
    return x + F32(1000) if family == "normal_off" else x


def _erf(a):
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(a))).numpy()


def _row_stats(x64, eps, ln=True):
    if not ln:
        return np.zeros((x64.shape[0], 1)), np.ones((x64.shape[0], 1))
    mean = x64.mean(1, keepdims=True)
    var = ((x64 - mean) ** 2).mean(1, keepdims=True)
    return mean, 1.0 / np.sqrt(var + eps)


def _xhat_unit(x64, mean, rstd):
    """The error of one fp32 xhat in units of K u: rstd (|x - mean| + max |x| of the row)."""
    return U * rstd * (np.abs(x64 - mean) + np.abs(x64).max(1, keepdims=True, initial=0.0))


def fwd_reference(c, lo=0, hi=None):
    """(float64 output, per-element budget) of rows lo .. hi of a forward case.
    B = K_FWD u (|gamma_j| rstd_i (|x_ij - mean_i| + max_j |x_ij|) + |beta_j|): the rounding of x - mean against a mean that carries
    the row's magnitude, scaled like the output, and the rounding of the affine; stretched by the activation's Lipschitz bound, plus
    the 6e-8 of fsf_gelu."""
    x = c["x"][lo:hi].astype(F64)
    ln = c["form"] != "aff"
    g = c["gamma"].astype(F64) if c["gamma"] is not None else np.ones(c["c"])
    b = c["beta"].astype(F64) if c["beta"] is not None else np.zeros(c["c"])
    mean, rstd = _row_stats(x, c["eps"], ln)
    y = (x - mean) * rstd * g + b
    B = K_FWD * (np.abs(g) * _xhat_unit(x, mean, rstd) + U * np.abs(b))
    if c["act"] == "relu":
        y = np.maximum(y, 0.0)
    elif c["act"] == "gelu":
        y = 0.5 * y * (1.0 + _erf(y / np.sqrt(2.0)))
        B = B * GELU_LIP + GELU_FWD_ABS
    return y, B


def bwd_reference(c):
    """float64 (grad_x, grad_gamma, grad_beta) of a backward case and their budgets, split as K * P + A (A: what the erf adds).
    With E = u rstd (|x - mean| + max |x|) the unit error of xhat, gy = grad_out * act'(y), gh = gy gamma, m1 = mean_j gh,
    m2 = mean_j gh xhat:   grad_x = rstd (gh - m1 - xhat m2);
      P_gx = rstd (u (|gh| + mean|gh| + |xhat| mean|gh xhat|) + e + mean_j e + |xhat| mean_j(e |xhat|) + E mean|gh xhat| + |xhat| mean_j(|gh| E))
      with e = |go gamma| curv |gamma| E the effect of xhat's error on act' (GELU only), and A_gx the same three places with
      e = |go gamma| 1.5e-7.
    grad_gamma_j = sum_i gy xhat: gamma(n + 20) sum_i |gy xhat| for the summation in any order (Higham §4.2; 20 covers the team,
      workgroup and fold stages) plus, per term, K (u |gy xhat| + |gy| E + e |xhat| / |gamma|); grad_beta the same without xhat."""
    x, go = c["x"].astype(F64), c["go"].astype(F64)
    n, ch = x.shape
    g = c["gamma"].astype(F64) if c["gamma"] is not None else np.ones(ch)
    b = c["beta"].astype(F64) if c["beta"] is not None else np.zeros(ch)
    mean, rstd = _row_stats(x, c["eps"])
    xh = (x - mean) * rstd
    y = xh * g + b
    E = _xhat_unit(x, mean, rstd)
    e_k = np.zeros_like(x)   # scaled by K
    e_a = np.zeros_like(x)   # absolute
    if c["act"] == "relu":
        d = (y > 0).astype(F64)
    elif c["act"] == "gelu":
        d = 0.5 * (1.0 + _erf(y / np.sqrt(2.0))) + y * np.exp(-0.5 * y * y) / np.sqrt(2.0 * np.pi)
        e_k = np.abs(go) * GELU_CURV * np.abs(g) * E
        e_a = np.abs(go) * ERF_BWD_ABS
    else:
        d = np.ones_like(y)
    gy = go * d
    gh = gy * g
    m = lambda a: a.mean(1, keepdims=True) if ch else a
    gx = rstd * (gh - m(gh) - xh * m(gh * xh))
    axh, agh = np.abs(xh), np.abs(gh)

    def spread(e):  # an error e of gy reaches grad_x through gh, m1 and m2
        eg = e * np.abs(g)
        return eg + m(eg) + axh * m(eg * axh)

    P_gx = rstd * (U * (agh + m(agh) + axh * m(agh * axh)) + spread(e_k) + E * m(agh * axh) + axh * m(agh * E))
    A_gx = rstd * spread(e_a)
    gam = (n + 20) * U / (1.0 - (n + 20) * U)
    agy = np.abs(gy)
    dg, db = (gy * xh).sum(0), gy.sum(0)
    P_dg = (U * agy * axh + agy * E + e_k * axh).sum(0)
    P_db = (U * agy + e_k).sum(0)
    S_dg, S_db = gam * (agy * axh).sum(0), gam * agy.sum(0)
    return dict(gx=gx, dg=dg, db=db, y=y, gy=gy, xh=xh, P_gx=P_gx, A_gx=A_gx, P_dg=P_dg, A_dg=(e_a * axh).sum(0) + S_dg,
                P_db=P_db, A_db=e_a.sum(0) + S_db)


def _affine(rng, c, form_affine, act, backward):
    if not form_affine:
        return None, None
    g = (rng.standard_normal(c) * 0.5 + 1.0).astype(F32)
    b = (rng.standard_normal(c) * 0.3).astype(F32)
    if backward and act == "relu":
        for j in {0, c // 2}:
            g[j] = b[j] = 0  # a pre-activation that is exactly 0: masked by `>`, passed by `>=`
    return g, b


def fwd_tags(c, n, form, act, layout):
    """The decisions of fsf_norm_act a forward case reaches, from its spec alone."""
    v4 = is_v4(c, layout, form != "ln")
    k = fwd_kernel(c, v4)
    tags = {f"fwd:{k.name}:{'affine' if form == 'aff' else 'ln'}:{act}", f"fwd:form_{form}", f"fwd:layout_{layout}"}
    if n > fwd_cap(k) * k.rows_per_wg:
        tags.add(f"fwd:{k.name}:second_trip")
    if k.ru == 2 and n % 2:
        tags.add("fwd:dead_ru_row")
    if n == 1:
        tags.add("fwd:n1")
    if c < k.slots:
        tags.add(f"fwd:{k.name}:ragged")
    if layout in FWD_FALLBACKS and c % 4 == 0:
        assert not v4
        tags.add(f"fwd:fallback_{layout}:{k.name}")
    if layout == "out_aligned" and v4:
        tags.add("fwd:slice_keeps_v4")
    return frozenset(tags)


def bwd_tags(c, n, affine, act, layout):
    """The decisions of fsf_norm_act_backward a backward case reaches, from its spec alone."""
    if n == 0:
        return frozenset({"bwd:n0"})
    k = bwd_kernel(c, is_v4(c, layout, affine))
    blocks = grid(n, k, NA_BWD_BLOCKS)
    tags = {f"bwd:{k.name}:{act}", f"bwd:layout_{layout}", "bwd:affine" if affine else "bwd:no_affine"}
    if blocks in FOLD_BLOCKS:
        tags.add(f"bwd:fold_blocks_{blocks}")
    if n > NA_BWD_BLOCKS * k.rows_per_wg:
        tags.add(f"bwd:{k.name}:second_trip")
    if k.ru == 2 and n % 2:
        tags.add("bwd:dead_ru_row")
    if k.form == "s":
        tags.add(f"bwd:{k.name}:by_misalignment" if c % 4 == 0 else f"bwd:{k.name}:by_width")
    return frozenset(tags)


def tags_of(name):
    if name.startswith("fwd"):
        return fwd_tags(*FWD_SPECS[name][:5])
    if name.startswith("bwd"):
        return bwd_tags(*BWD_SPECS[name][:5])
    return bn_tags(*BN_SPECS[name])


@functools.lru_cache(maxsize=4)
def fwd_case(name):
    c, n, form, act, layout, family = FWD_SPECS[name]
    rng = _rng(name)
    gamma, beta = _affine(rng, c, form != "ln", act, False)
    v4 = is_v4(c, layout, gamma is not None)
    return dict(name=name, c=c, n=n, form=form, act=act, layout=layout, family=family, eps=1e-3, x=_values(rng, n, c, family),
                gamma=gamma, beta=beta, kern=fwd_kernel(c, v4), v4=v4, tags=tags_of(name))


@functools.lru_cache(maxsize=4)
def bwd_case(name):
    c, n, affine, act, layout, family = BWD_SPECS[name]
    rng = _rng(name)
    gamma, beta = _affine(rng, c, affine, act, True)
    v4 = is_v4(c, layout, affine)
    k = bwd_kernel(c, v4)
    x = _values(rng, n, c, family)
    go = _values(rng, n, c, "ints" if family == "ints" else "normal")
    d = dict(name=name, c=c, n=n, form="lna" if affine else "ln", act=act, layout=layout, family=family, eps=1e-3, x=x, go=go,
             gamma=gamma, beta=beta, kern=k, v4=v4)
    if n and act == "relu":  # keep the mask unambiguous: no gradient where the float64 pre-activation is within rounding of 0
        y, B = fwd_reference(dict(d, act="none"))
        near = np.abs(y) <= MASK_MARGIN * B
        if gamma is not None:
            near[:, (gamma == 0) & (beta == 0)] = False  # exactly 0 in fp32 and in float64
        d["go"] = go = np.where(near, F32(0), go)
        d["mask_margin"] = (y, B)
    d["tags"] = tags_of(name)
    d["blocks"] = grid(n, k, NA_BWD_BLOCKS)
    if family == "ints":
        assert 8 * max(n, 1) < 2 ** 24
        if act == "none":
            d["want_db"] = go.astype(np.int64).sum(0).astype(F32)
    return d


def case(name):
    return fwd_case(name) if name.startswith("fwd") else bwd_case(name) if name.startswith("bwd") else bn_case(name)


# ---- K12 judges --------------------------------------------------------------------------------------------------------------------------

ROW_CHUNK = 1 << 15


def _per_element(got, want, bound, what):
    err = np.abs(got.astype(F64) - want)
    bad = ~(err <= bound)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.size} elements outside their budget; worst at {i}: got {got[i]!r}, "
                             f"want {want[i]!r}, |err| {err[i]:.3e} > {np.broadcast_to(bound, err.shape)[i]:.3e}")


def check_fwd(c, out):
    """`out` f32 [n, c] against the float64 referee, per element."""
    assert out.shape == (c["n"], c["c"]) and out.dtype == F32
    for lo in range(0, c["n"], ROW_CHUNK):
        y, B = fwd_reference(c, lo, lo + ROW_CHUNK)
        _per_element(out[lo:lo + ROW_CHUNK], y, B, f"{c['name']} rows {lo}..")


def check_bwd(c, gx, dg, db, ref=None):
    """grad_x per element; grad_beta bit for bit where the case has an integer referee, else per channel; grad_gamma per channel on
    the cases small enough for the bound to see a row (`gamma_judged`)."""
    n, ch = c["n"], c["c"]
    assert gx.shape == (n, ch) and gx.dtype == F32
    affine = c["gamma"] is not None
    assert (dg is not None) == affine and (db is not None) == affine
    if n == 0:
        if affine:
            np.testing.assert_array_equal(dg, np.zeros(ch, F32), err_msg=f"{c['name']} grad_gamma")
            np.testing.assert_array_equal(db, np.zeros(ch, F32), err_msg=f"{c['name']} grad_beta")
        return
    r = ref or bwd_reference(c)
    _per_element(gx, r["gx"], K_GX * r["P_gx"] + r["A_gx"], f"{c['name']} grad_x")
    if not affine:
        return
    if "want_db" in c:
        np.testing.assert_array_equal(db, c["want_db"], err_msg=f"{c['name']} grad_beta (exact)")
    else:
        _per_element(db, r["db"], K_COL * r["P_db"] + r["A_db"], f"{c['name']} grad_beta")
    if gamma_judged(c):
        _per_element(dg, r["dg"], K_COL * r["P_dg"] + r["A_dg"], f"{c['name']} grad_gamma")


GAMMA_MAX_ROWS = 600


def gamma_judged(c):
    return c["n"] <= GAMMA_MAX_ROWS


# ---- K23 ---------------------------------------------------------------------------------------------------------------------------------

BN_WIDTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 131, 256, 257, 300, 512, 513)
BN_SPECS = {}   # name -> (c, n)


def _bn(c, n):
    BN_SPECS[f"bn-c{c}-n{n}"] = (c, n)


def _make_bn_specs():
    for c in BN_WIDTHS:
        ry = cs_ry(c)
        for n in (1, 2 * ry, 3 * ry, 3 * ry + 1, 4 * ry, 5 * ry, 8 * ry + 1, 16 * ry + 7):
            _bn(c, n)
    for c in (131, 64):           # the fold's block counts: whole workgroups of 8 ry rows
        for b in FOLD_BLOCKS:
            _bn(c, b * 8 * cs_ry(c))
    for c in (64, 128, 131, 300):  # rows_per_block leaves its floor (and, for ry > 1, stops being a multiple of ry)
        _bn(c, CS_BLOCKS * 8 * cs_ry(c))
        _bn(c, CS_BLOCKS * 8 * cs_ry(c) + 1)


_make_bn_specs()
BN_NAMES = tuple(BN_SPECS)
BN_EPS = 1e-3
BN_MOMENTUM = 0.125


def bn_tail_tags(n, c):
    """Tail lengths (0..3) of the by-4 unroll for the first and the last `ty` of the last workgroup of column_stats_kernel."""
    ry = cs_ry(c)
    blocks, rpb = cs_blocks(n, c)
    R = n - (blocks - 1) * rpb
    return cdiv(R, ry) % 4, (R // ry) % 4, R


def _is_pow2(n):
    return n > 0 and n & (n - 1) == 0


def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 operands: the product is exact in 64 mantissa bits, the sum is formed there and rounded once to fp32
    (callers keep the exponents of product and addend close enough for the sum to be exact: asserted)."""
    a, b, c = (np.asarray(v, F32).astype(np.longdouble) for v in (a, b, c))
    s = a * b + c
    assert np.array_equal(s - c, a * b)  # nothing was lost before the final rounding
    return s.astype(F32)


def bn_tags(c, n):
    """The decisions of the K23 kernels a (c, n) case reaches."""
    ry, l = cs_ry(c), cs_cw_log2(c)
    blocks, rpb = cs_blocks(n, c)
    tf, tl, R = bn_tail_tags(n, c)
    tags = {f"bn:cw_log2_{l}", "bn:c_at_pow2" if _is_pow2(c) else "bn:c_below_pow2", f"bn:tail_first_{tf}", f"bn:tail_last_{tl}"}
    if c > 256:
        tags.add("bn:column_passes" if c % 256 == 0 else "bn:column_passes_ragged")
    if n == 1:
        tags.add("bn:n1")
    if R == 1 and blocks > 1:
        tags.add("bn:last_block_one_row")
    if blocks in FOLD_BLOCKS:
        tags.add(f"bn:fold_blocks_{blocks}")
    if rpb > 8 * ry:
        tags.add("bn:rpb_above_floor" + ("_not_multiple_of_ry" if rpb % ry else ""))
    elif n == CS_BLOCKS * 8 * ry:
        tags.add("bn:rpb_floor_at_1024_blocks")
    if n % bn_rows_per_block(c):
        tags.add("bn:rows_kernel_partial_block")
    return frozenset(tags)


@functools.lru_cache(maxsize=4)
def bn_case(name):
    c, n = BN_SPECS[name]
    rng = _rng(name)
    blocks, rpb = cs_blocks(n, c)
    d = dict(name=name, c=c, n=n, blocks=blocks, rpb=rpb, tags=bn_tags(c, n))
    inv_n = F32(1.0) / F32(n)

    # ints: exact sums, the mean one fp32 product
    x = _values(rng, n, c, "ints")
    assert 8 * n < 2 ** 24
    d["x"] = x
    d["want_sum"] = x.astype(np.int64).sum(0).astype(F32)
    d["want_mean"] = d["want_sum"] * inv_n

    # balanced: every column sums to 0 (pairs v, -v; an odd n closes with a, a, -2a), rows shuffled
    if n >= 2:
        half = _values(rng, n // 2, c, "ints")
        xb = np.empty((n, c), F32)
        xb[0:2 * (n // 2):2], xb[1:2 * (n // 2):2] = half, -half
        if n % 2:
            a = rng.integers(1, 5, c) * rng.choice((-1, 1), c)
            xb[n - 3], xb[n - 2], xb[n - 1] = a, a, -2 * a
        xb = xb[rng.permutation(n)]
        sq = (xb.astype(np.int64) ** 2).sum(0)
        assert (xb.astype(np.int64).sum(0) == 0).all() and sq.max() < 2 ** 24 and (xb != 0).all()
        d["xb"] = xb
        d["want_var"] = sq.astype(F32) * inv_n
        w = (rng.integers(1, 8, c) * 0.25).astype(F32) * rng.choice((-1, 1), c).astype(F32)
        b = (rng.integers(-8, 9, c) * 0.125).astype(F32)
        rm, rv = (rng.integers(-8, 9, c) * 0.25).astype(F32), (rng.integers(1, 9, c) * 0.5).astype(F32)
        invstd = (1.0 / np.sqrt(d["want_var"].astype(F64) + F64(F32(BN_EPS)))).astype(F32)  # correctly rounded, as the kernel's
        keep, mom = F32(1.0 - BN_MOMENTUM), F32(BN_MOMENTUM)
        var_alpha = F32(BN_MOMENTUM * n / max(n - 1, 1))
        zero = np.zeros(c, F32)
        d["stats"] = dict(weight=w, bias=b, running_mean=rm, running_var=rv, invstd=invstd, scale=w * invstd, shift=b,
                          scale_plain=invstd, shift_plain=zero, new_running_mean=fma32(mom, zero, rm * keep),
                          new_running_var=fma32(var_alpha, d["want_var"], rv * keep))

    # exact backward: y = fma(x, scale, shift) exact, and exactly 0 wherever x equals the integer mean
    go = (rng.integers(1, 5, (n, c)) * rng.choice((-1, 1), (n, c))).astype(F32)
    mean = rng.integers(-2, 3, c).astype(F32)
    invstd = rng.choice((0.5, 1.0), c).astype(F32)
    w = rng.choice((-1.5, -0.5, 0.5, 1.0, 2.0), c).astype(F32)
    bb = rng.choice((0.0, 0.25, -0.5, 1.0), c).astype(F32)
    scale = w * invstd
    shift = bb - mean * scale
    assert 2 * 4 * 10 * n < 2 ** 24  # |g (x - mean) invstd| <= 40, a multiple of 1/2: every partial sum is exact
    d["bwd"] = dict(x=x, go=go, mean=mean, invstd=invstd, scale=scale, shift=shift)
    for key, (sc, sh) in (("affine", (scale, shift)), ("plain", (invstd, -mean * invstd))):
        y = x.astype(F64) * sc + sh
        assert np.array_equal(y.astype(F32).astype(F64), y)
        for relu in (False, True):
            g = np.where(y > 0, go, F32(0)) if relu else go
            t = (x - mean) * invstd
            sum_g, sum_gx = g.astype(F64).sum(0), (g.astype(F64) * t).sum(0)
            sg, sgx = sum_g.astype(F32) * inv_n, sum_gx.astype(F32) * inv_n
            want = dict(db=sum_g.astype(F32), dg=sum_gx.astype(F32), y=y.astype(F32))
            assert np.array_equal(want["db"].astype(F64), sum_g) and np.array_equal(want["dg"].astype(F64), sum_gx)
            ref = sc.astype(F64) * (g - (sum_g / n + t.astype(F64) * (sum_gx / n)))
            want["gx64"] = ref
            want["gx_bound"] = bn_grad_x_bound(sc, g, sum_g / n, t * (sum_gx / n))
            want["gx_exact"] = None
            if _is_pow2(n):  # replay every step in fp32 and in float64: equal means no step rounded
                p32, p64 = t * sgx, t.astype(F64) * sgx.astype(F64)
                s32, s64 = sg + p32, sg.astype(F64) + p64
                d32, d64 = g - s32, g.astype(F64) - s64
                r32, r64 = sc * d32, sc.astype(F64) * d64
                if all(np.array_equal(a.astype(F64), b) for a, b in ((p32, p64), (s32, s64), (d32, d64), (r32, r64))):
                    want["gx_exact"] = r32
                    assert np.array_equal(r64, ref)
            d["bwd"][(key, relu)] = want
    return d


def bn_grad_x_bound(sc, g, sg, tsgx):
    """grad_x = sc (g - (sg + t sgx)), sg = sum_g inv_n, sgx = sum_gx inv_n with inv_n = fl(1 / n); sum_g, sum_gx, t are exact.
    Roundings, each at most u times the magnitude it produces: inv_n (reaches sg and t sgx), sg, sgx, the product t sgx, the inner sum
    (<= |sg| + |t sgx|), the difference and the final product (each <= |g| + |sg| + |t sgx|).  In all
    u |sc| (5 |sg| + 6 |t sgx| + 2 |g|); a contraction to fma only removes roundings; 1.001 covers the second order."""
    return 1.001 * U * np.abs(sc) * (5 * np.abs(sg) + 6 * np.abs(tsgx) + 2 * np.abs(g))


def check_bn_grad_x(c, key, relu, gx):
    w = c["bwd"][(key, relu)]
    if w["gx_exact"] is not None:
        np.testing.assert_array_equal(gx, w["gx_exact"], err_msg=f"{c['name']} grad_x {key} relu={relu} (exact)")
    else:
        _per_element(gx, w["gx64"], w["gx_bound"], f"{c['name']} grad_x {key} relu={relu}")


# the normal family of K23: the two-pass claim, per column
def bn_normal(c, n, off):
    rng = _rng(f"bn-normal-{c}-{n}-{off}")
    x = _values(rng, n, c, "normal_off" if off else "normal")
    x64 = x.astype(F64)
    mean = x64.mean(0)
    dev = x64 - mean
    var = (dev ** 2).mean(0)
    gam = (n + 20) * U / (1.0 - (n + 20) * U)
    mean_b = gam * np.abs(x64).mean(0) + 2 * U * np.abs(mean)
    # The device's deviations are d_i = (x_i - mean - delta) (1 + e_i), |delta| <= mean_b, |e_i| <= u.  Because sum_i (x_i - mean) = 0
    # the common error delta enters the variance only as delta^2; what remains are the roundings of the differences (2 u), of the
    # squares (u), of the summation (gamma) and of the product with fl(1 / n) (2 u), on the mean of (|x_i - mean| + |delta|)^2.
    var_b = mean_b ** 2 + 1.01 * (5 * U + gam) * ((np.abs(dev) + mean_b) ** 2).mean(0)
    return dict(x=x, mean=mean, var=var, mean_bound=mean_b, var_bound=var_b, sum=x64.sum(0), sum_bound=gam * np.abs(x64).sum(0))


BN_NORMAL = ((5, 300, False), (5, 300, True), (131, 133, True), (300, 77, True), (64, 515, True), (64, 2051, False))


def check_columns(got, want, bound, what):
    _per_element(got, want, bound, what)
