"""K39 on the device (docs/kernels/K39_optimizer_step.md): `FusedAdamW.step()` — fsf_optim_grad_sumsq + fsf_optim_adamw_step over the
chunk table — against `FusedAdamW(fused=False)`, the torch restatement of the same arithmetic on the same bucket layout, bit for bit.

With C = FSF_OPTIM_CHUNK the toy module has parameters of [1, 3, 128, C - 1, C, C + 1, 2 C + 5] elements in two registration orders.
`FrameDataParallel` fills its buckets in reverse registration order and closes one when the next parameter would pass
`int(bucket_mb * 2**20) // 4` floats:
  * "unaligned", cap 2 C + 8: buckets [1, 2C+5] [C+1, C-1, 3] [128, C]; the 2C+5 and C-1 parameters sit 1 and C + 1 floats into their
    buckets (the one-float-at-a-time form of gradient and moments beside a 16-byte aligned parameter), the others on 16-byte bounds;
  * "aligned", cap C + 4: buckets [128, 1] [C, 3] [C-1] [C+1] [2C+5], every offset a multiple of 4 floats."""
import copy
import math

import numpy as np
import pytest
import torch

from test_optim_cpu import NUS_LR, NUS_MOMENTUM, NUS_OPTIMIZER, NUS_OPTIMIZER_CONFIG, exact_norm, ulp_distance

pytestmark = pytest.mark.gpu

LRS = [1e-3, 2e-3, 1.5e-3, 5e-4]
BETA1 = [0.9, 0.88, 0.85, 0.45]  # (the last one takes lerp's other branch: 1 - beta1 >= 0.5)
KEYS = {"slow": dict(lr_mult=0.2), "norm": dict(decay_mult=0.)}


def chunk():
    from fullysparsefusion_amd import _lib

    return _lib.DEFINES["FSF_OPTIM_CHUNK"]


def layout(name):
    """(registration order of the sizes, bucket_mb, expected bucket contents in fill order)."""
    c = chunk()
    if name == "unaligned":
        return [c, 128, 3, c - 1, c + 1, 2 * c + 5, 1], (2 * c + 8) * 4 / 2 ** 20, [[1, 2 * c + 5], [c + 1, c - 1, 3], [128, c]]
    return [2 * c + 5, c + 1, c - 1, 3, c, 1, 128], (c + 4) * 4 / 2 ** 20, [[128, 1], [c, 3], [c - 1], [c + 1], [2 * c + 5]]


class Toy(torch.nn.Module):
    """loss = sum_i <p_i, x_i>: the gradient of p_i is x_i.  Parameter 0 is in the lr_mult group, parameter 1 in the decay_mult = 0 one."""

    def __init__(self, sizes, seed=7):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        names = ["slow", "norm"] + [f"w{i}" for i in range(2, len(sizes))]
        for name, n in zip(names, sizes):
            m = torch.nn.Module()
            m.register_parameter("weight", torch.nn.Parameter(torch.randn(n, generator=g)))
            self.add_module(name, m)

    def forward(self, xs):
        return sum((p * x).sum() for p, x in zip(self.parameters(), xs))


def make(name, device, fused, grad_clip):
    from fullysparsefusion_amd.data_parallel import FrameDataParallel
    from fullysparsefusion_amd.optim import FusedAdamW

    sizes, bucket_mb, want = layout(name)
    toy = Toy(sizes).to(device)
    dp = FrameDataParallel(toy, bucket_mb=bucket_mb)
    assert [[p.numel() for p in b.params] for b in dp.buckets] == want and len(dp.buckets) >= 3
    opt = FusedAdamW(dp, lr=1e-3, weight_decay=0.05, paramwise_cfg=dict(custom_keys=KEYS), grad_clip=grad_clip, fused=fused)
    assert len(opt.groups) == 3
    return toy, dp, opt


def grads_for(sizes, steps, scale, seed=13):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(n, generator=g) * scale for n in sizes] for _ in range(steps)]


def set_grads(opt, grads, device):
    for p, g in zip(opt.params, grads):
        p.grad.copy_(g.to(device))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def assert_same_state(opt_a, opt_b, what):
    for i, (sa, sb) in enumerate(zip(opt_a._slots, opt_b._slots)):
        for k, part in enumerate(("parameter", "gradient", "exp_avg", "exp_avg_sq")):
            assert torch.equal(bits(sa[k]), bits(sb[k])), f"{what}: {part} of parameter {i} ({sa[0].numel()} elements) differs"


def test_the_two_layouts_are_what_the_docstring_says(device):
    for name, some_unaligned in (("unaligned", True), ("aligned", False)):
        _, dp, opt = make(name, device, True, None)
        rows = opt.table.cpu().numpy()
        assert int((rows[:, 4] & 0xFFFFFFFF).sum()) == sum(p.numel() for p in opt.params)
        assert (rows[:, 0] % 16 == 0).all(), "the caching allocator hands out 16-byte aligned parameters"
        off = rows[:, 1] % 16 != 0
        assert ((rows[:, 1] % 16) == (rows[:, 2] % 16)).all() and ((rows[:, 1] % 16) == (rows[:, 3] % 16)).all()
        assert off.any() == some_unaligned and (not some_unaligned or (~off).any())


@pytest.mark.parametrize("name", ["unaligned", "aligned"])
@pytest.mark.parametrize("mode", ["active", "inactive", "off"])
def test_device_step_equals_the_restatement_bit_for_bit(device, name, mode):
    """4 steps, lr and beta1 changing per step.  |g| ~ 3 sqrt(5 C) ~ 430: max_norm 35 clips every step ("active"), max_norm 1e6 never does
    (coef exactly 1), grad_clip=None launches K39b alone and leaves the norm output as it was."""
    clip = dict(active=dict(max_norm=35, norm_type=2), inactive=dict(max_norm=1e6, norm_type=2), off=None)[mode]
    _, dp_a, opt_a = make(name, device, True, clip)
    _, dp_b, opt_b = make(name, device, False, clip)
    grads = grads_for([p.numel() for p in opt_a.params], 4, 3.0)
    opt_a.grad_norm.fill_(-7.0), opt_b.grad_norm.fill_(-7.0)
    for s in range(4):
        for opt in (opt_a, opt_b):
            opt.group_lr = [LRS[s] * lm for lm, _ in opt.groups]
            opt.beta1 = BETA1[s]
            set_grads(opt, grads[s], device)
            opt.step()
        assert_same_state(opt_a, opt_b, f"{name} / {mode}, step {s}")
        assert torch.equal(bits(opt_a.grad_norm), bits(opt_b.grad_norm))
        assert all(float(b.flat.abs().max()) == 0.0 for b in dp_a.buckets), "the consumed gradient is cleared"
    norm = float(opt_a.grad_norm)
    assert (norm == -7.0) if mode == "off" else (300.0 < norm < 600.0)
    moved = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(opt_a.params, Toy(layout(name)[0]).to(device).parameters()))
    assert moved > 1e-3
    if mode == "inactive":  # coef is EXACTLY 1: the same bits as without clipping
        _, _, opt_c = make(name, device, True, None)
        for s in range(4):
            opt_c.group_lr, opt_c.beta1 = [LRS[s] * lm for lm, _ in opt_c.groups], BETA1[s]
            set_grads(opt_c, grads[s], device)
            opt_c.step()
        assert_same_state(opt_a, opt_c, "max_norm never reached against no clipping")


@pytest.mark.parametrize("name", ["unaligned", "aligned"])
def test_norm_is_within_one_ulp_and_the_same_bits_on_every_run_and_zero_grads_false_leaves_the_gradient(device, name):
    _, dp, opt = make(name, device, True, dict(max_norm=35, norm_type=2))
    set_grads(opt, grads_for([p.numel() for p in opt.params], 1, 3.0, seed=17)[0], device)
    before = [b.flat.clone() for b in dp.buckets]
    want = exact_norm([b.cpu() for b in before])
    seen = []
    for _ in range(2):
        opt.grad_norm.fill_(0.0)
        opt.step(zero_grads=False)
        seen.append(bits(opt.grad_norm).clone())
        for b, was in zip(dp.buckets, before):
            assert torch.equal(bits(b.flat), bits(was)), "zero_grads=False leaves the gradient bits alone"
    assert torch.equal(seen[0], seen[1])
    print(f"K39a {name}: device norm {float(opt.grad_norm)!r}, exactly summed {float(want)!r}")
    assert ulp_distance(float(opt.grad_norm), want) <= 1
    opt.step()
    assert all(float(b.flat.abs().max()) == 0.0 for b in dp.buckets)


def test_after_zero_grads_true_the_next_backward_accumulates_onto_zeros(device):
    """Route A: step(zero_grads=True), forward, backward, no dp.zero_grad().  Route B: step(zero_grads=False), dp.zero_grad(), forward,
    backward.  The buckets and the following step must agree bit for bit; a third backward inside no_sync() doubles the gradient."""
    clip = dict(max_norm=35, norm_type=2)
    routes = []
    for route in "AB":
        toy, dp, opt = make("unaligned", device, True, clip)
        sizes = [p.numel() for p in opt.params]
        first, xs = grads_for(sizes, 1, 3.0, seed=19)[0], [x.to(device) for x in grads_for(sizes, 1, 0.5, seed=23)[0]]
        set_grads(opt, first, device)
        if route == "A":
            opt.step()
        else:
            opt.step(zero_grads=False)
            dp.zero_grad()
        dp.backward(dp(xs))
        for p, x in zip(toy.parameters(), xs):
            assert torch.equal(bits(p.grad), bits(x)) and p.grad.data_ptr() == dp._view[p].data_ptr()
        with dp.no_sync():
            dp.backward(dp(xs))
        for p, x in zip(toy.parameters(), xs):
            assert torch.equal(bits(p.grad), bits(x + x))
        opt.step()
        routes.append(opt)
    assert_same_state(routes[0], routes[1], "zero_grads=True against dp.zero_grad()")


def test_one_infinite_gradient_element_as_torch_makes_it_on_the_device(device):
    toy, dp, opt = make("unaligned", device, True, dict(max_norm=35, norm_type=2))
    sizes = [p.numel() for p in opt.params]
    grads = grads_for(sizes, 1, 3.0, seed=29)[0]
    big = max(range(len(sizes)), key=lambda i: sizes[i])
    grads[big][chunk() + 77] = float("inf")
    ref = Toy(layout("unaligned")[0]).to(device)
    params = list(ref.parameters())
    topt = torch.optim.AdamW([dict(params=[p], lr=1e-3 * (0.2 if i == 0 else 1.0), weight_decay=0.0 if i == 1 else 0.05)
                              for i, p in enumerate(params)], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    for p, g in zip(params, grads):
        p.grad = g.to(device).clone()
    tnorm = torch.nn.utils.clip_grad_norm_(params, 35, norm_type=2, foreach=False)
    topt.step()
    set_grads(opt, grads, device)
    opt.step()
    assert math.isinf(float(tnorm)) and math.isinf(float(opt.grad_norm))
    for i, (a, b) in enumerate(zip(opt.params, params)):
        nan = torch.isnan(b)
        assert int(nan.sum()) == (1 if i == big else 0) and torch.equal(torch.isnan(a), nan)
        assert torch.equal(bits(a)[~nan], bits(b)[~nan])  # p * f32(1 - lr wd), then minus step * 0
        eff = opt._slots[i][2]  # exp_avg = lerp(0, g * coef, w): NaN where torch's clipped gradient is NaN, 0 elsewhere
        assert torch.equal(torch.isnan(eff), nan) and torch.equal(torch.isnan(b.grad), nan)
        assert float(torch.nan_to_num(eff, nan=0.0).abs().max()) == 0.0 and float(torch.nan_to_num(b.grad, nan=0.0).abs().max()) == 0.0
    assert all(float(b.flat.abs().max()) == 0.0 for b in dp.buckets)


def test_a_module_without_trainable_parameters_steps_as_a_no_op(device):
    from fullysparsefusion_amd import _lib
    from fullysparsefusion_amd.data_parallel import FrameDataParallel
    from fullysparsefusion_amd.optim import CyclicSchedule, FusedAdamW

    frozen = torch.nn.Linear(4, 4).to(device).requires_grad_(False)
    was = frozen.weight.clone()
    opt = FusedAdamW(FrameDataParallel(frozen), lr=1e-3, grad_clip=dict(max_norm=35, norm_type=2))
    CyclicSchedule(NUS_LR, NUS_MOMENTUM, 10).apply(opt, 3)
    opt.step()
    assert opt.step_count == 0 and opt.table is None and torch.equal(frozen.weight, was)
    assert opt.state_dict() == dict(state={}, param_groups=[])
    h = _lib.lib()
    ok = _lib.DEFINES["FSF_OK"]
    assert h.fsf_optim_grad_sumsq(None, 0, None, 0, _lib.stream_ptr()) == ok
    assert h.fsf_optim_adamw_step(None, 0, 0, None, None, 0.1, 0.999, 0.001, 1.0, 1e-8, 35.0, 1, 1, None, 0, None, _lib.stream_ptr()) == ok
    assert h.fsf_optim_table_bytes(0) == 0 and h.fsf_optim_workspace_bytes(0) == 8
    one = torch.zeros((1, 5), dtype=torch.int64, device=device)
    unsupported, invalid, workspace = (_lib.DEFINES[k] for k in ("FSF_ERR_UNSUPPORTED", "FSF_ERR_INVALID_ARG", "FSF_ERR_WORKSPACE"))
    arr = _lib.f32_array([1.0] * 9)
    assert h.fsf_optim_adamw_step(_lib.ptr(one), 1, 9, arr, arr, 0.1, 0.999, 0.001, 1.0, 1e-8, 35.0, 0, 1, None, 0, None, _lib.stream_ptr()) == unsupported
    assert h.fsf_optim_adamw_step(None, 1, 1, arr, arr, 0.1, 0.999, 0.001, 1.0, 1e-8, 35.0, 0, 1, None, 0, None, _lib.stream_ptr()) == invalid
    assert h.fsf_optim_grad_sumsq(None, 1, _lib.ptr(one), 8, _lib.stream_ptr()) == invalid
    assert h.fsf_optim_grad_sumsq(_lib.ptr(one), 1, _lib.ptr(one), 7, _lib.stream_ptr()) == workspace


def test_step_and_schedule_never_wait_for_the_device(device):
    from fullysparsefusion_amd.optim import CyclicSchedule

    _, dp, opt = make("unaligned", device, True, dict(max_norm=35, norm_type=2))
    sched = CyclicSchedule(NUS_LR, NUS_MOMENTUM, 10)
    grads = [g.to(device) for g in grads_for([p.numel() for p in opt.params], 1, 3.0)[0]]
    sched.apply(opt, 0)
    torch._foreach_copy_([p.grad for p in opt.params], grads)
    opt.step()  # (the first call may allocate scratch)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for it in (1, 2):
            sched.apply(opt, it)
            torch._foreach_copy_([p.grad for p in opt.params], grads)
            opt.step(zero_grads=it == 1)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert opt.step_count == 3 and 300.0 < float(opt.grad_norm) < 600.0


def test_whole_model_three_steps_equal_the_restatement_and_the_table_covers_every_parameter_once(device):
    from conftest import build_test_fsf
    from fullysparsefusion_amd.data_parallel import FrameDataParallel
    from fullysparsefusion_amd.optim import CyclicSchedule, build_optimizer

    model_a = build_test_fsf().to(device)
    model_b = copy.deepcopy(model_a)
    dp_a, dp_b = FrameDataParallel(model_a), FrameDataParallel(model_b)
    opt_a = build_optimizer(dp_a, NUS_OPTIMIZER, NUS_OPTIMIZER_CONFIG)
    opt_b = build_optimizer(dp_b, NUS_OPTIMIZER, NUS_OPTIMIZER_CONFIG, fused=False)
    total = sum(p.numel() for p in model_a.parameters() if p.requires_grad)
    rows = opt_a.table.cpu().numpy()
    count, group = rows[:, 4] & 0xFFFFFFFF, rows[:, 4] >> 32
    assert int(count.sum()) == total and count.min() >= 1 and count.max() <= chunk() and set(group.tolist()) == {0, 1}
    for col, tensors in ((0, opt_a.params), (1, [b.flat for b in dp_a.buckets])):  # every row inside a tensor, no two rows overlapping
        order = np.argsort(rows[:, col])
        lo, hi = rows[order, col], rows[order, col] + 4 * count[order]
        assert (hi[:-1] <= lo[1:]).all()
        spans = sorted((t.data_ptr(), t.data_ptr() + 4 * t.numel()) for t in tensors)
        starts = np.array([s for s, _ in spans])
        owner = np.searchsorted(starts, lo, side="right") - 1
        assert (owner >= 0).all() and (hi <= np.array([e for _, e in spans])[owner]).all()
    sched = CyclicSchedule(NUS_LR, NUS_MOMENTUM, 10)
    torch.manual_seed(5)
    for s, scale in enumerate((1.0, 1e-4, 0.5)):  # |g| ~ scale sqrt(total): clipped, not clipped, clipped
        for fa, fb in zip((b.flat for b in dp_a.buckets), (b.flat for b in dp_b.buckets)):
            fa.normal_().mul_(scale)
            fb.copy_(fa)
        for opt in (opt_a, opt_b):
            sched.apply(opt, s + 3)
            opt.step()
        assert torch.equal(bits(opt_a.grad_norm), bits(opt_b.grad_norm))
    print(f"K39 whole model: {total} parameters in {len(opt_a.params)} tensors, {len(dp_a.buckets)} buckets, {rows.shape[0]} table rows, "
          f"last norm {float(opt_a.grad_norm):.4f}")
    for pa, pb in zip(dp_a.buckets, dp_b.buckets):
        assert float(pa.flat.abs().max()) == 0.0 and float(pb.flat.abs().max()) == 0.0
    for m_a, m_b in zip(opt_a.exp_avg + opt_a.exp_avg_sq, opt_b.exp_avg + opt_b.exp_avg_sq):
        assert torch.equal(bits(m_a), bits(m_b))
    for name, pa, pb in zip(opt_a.names, opt_a.params, opt_b.params):
        assert torch.equal(bits(pa), bits(pb)), name
    assert float((model_a.segmentor_updated_mlp[-1].weight.detach() - build_test_fsf().segmentor_updated_mlp[-1].weight.detach().to(device)).abs().max()) > 0
