"""The optimizer step on the host (K39, docs/kernels/K39_optimizer_step.md): mmcv's `custom_keys` rule, the cyclic schedule's closed
form, `FusedAdamW(fused=False)` — the torch restatement the kernels are tested against on the device — against torch's own clip +
AdamW judged through float64, the gradient norm, the non-finite case, checkpoints in torch's layout, the refusals, the C ABI surface
and the static guard-band check of the new wrapper module."""
import ast
import math
import os
import re

import numpy as np
import pytest
import torch

from fullysparsefusion_amd import optim
from fullysparsefusion_amd.data_parallel import FrameDataParallel
from fullysparsefusion_amd.optim import CyclicSchedule, FusedAdamW, annealing_cos, build_optimizer, param_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the reference's dicts (projects/configs/_base_/schedules/cyclic_20e.py, cosine_2x.py, FSF_nuScenes_config.py, FSF_AV2_config.py)
NUS_OPTIMIZER = dict(type="AdamW", lr=1e-4, weight_decay=0.01,
                     paramwise_cfg=dict(custom_keys={"segmentor.backbone": dict(lr_mult=0.2), "segmentor.voxel_encoder": dict(lr_mult=0.2)}))
NUS_OPTIMIZER_CONFIG = dict(grad_clip=dict(max_norm=35, norm_type=2))
NUS_LR = dict(policy="cyclic", target_ratio=(10, 1e-4), cyclic_times=1, step_ratio_up=0.4)
NUS_MOMENTUM = dict(policy="cyclic", target_ratio=(0.85 / 0.95, 1), cyclic_times=1, step_ratio_up=0.4)
AV2_KEYS = {"norm": dict(decay_mult=0.), "segmentor.backbone": dict(lr_mult=0.2), "segmentor.voxel_encoder": dict(lr_mult=0.2)}
AV2_LR = dict(policy="cyclic", target_ratio=(100, 1e-3), cyclic_times=1, step_ratio_up=0.1)


# ------------------------------------------------------------------------------------------------ param groups
class _Named(torch.nn.Module):
    """Parameters under given dotted names (nested modules are made on the way)."""

    def __init__(self, names_sizes):
        super().__init__()
        g = torch.Generator().manual_seed(7)
        for name, n in names_sizes:
            mod, parts = self, name.split(".")
            for part in parts[:-1]:
                if not hasattr(mod, part):
                    mod.add_module(part, torch.nn.Module())
                mod = getattr(mod, part)
            mod.register_parameter(parts[-1], torch.nn.Parameter(torch.randn(n, generator=g)))


def test_custom_keys_on_a_toy_module_with_the_expected_pairs_written_out():
    toy = _Named([("segmentor.backbone.conv.weight", 4), ("segmentor.backbone.norm.weight", 4), ("segmentor.voxel_encoder.fc.bias", 2),
                  ("segmentor.decode_head.norm.bias", 2), ("head.fc.weight", 3), ("norm.weight", 5), ("frozen.weight", 2)])
    toy.frozen.weight.requires_grad_(False)
    mults, groups = param_groups(toy, dict(custom_keys=AV2_KEYS))
    # the keys in mmcv's order: "segmentor.voxel_encoder" (longest), "segmentor.backbone", "norm".  A norm INSIDE segmentor.backbone
    # matches "segmentor.backbone" and "norm": the longer key is tried first and wins, so that norm keeps its weight decay.
    assert mults == {"segmentor.backbone.conv.weight": (0.2, 1.0), "segmentor.backbone.norm.weight": (0.2, 1.0),
                     "segmentor.voxel_encoder.fc.bias": (0.2, 1.0), "segmentor.decode_head.norm.bias": (1.0, 0.0),
                     "head.fc.weight": (1.0, 1.0), "norm.weight": (1.0, 0.0)}
    assert list(mults) == [n for n, p in toy.named_parameters() if p.requires_grad]
    assert groups == [(0.2, 1.0), (1.0, 0.0), (1.0, 1.0)]
    assert param_groups(toy, None)[1] == [(1.0, 1.0)]
    opt = build_optimizer(FrameDataParallel(toy), dict(type="AdamW", lr=1e-5, betas=(0.9, 0.999), weight_decay=0.05,
                                                       paramwise_cfg=dict(custom_keys=AV2_KEYS)),
                          dict(grad_clip=dict(max_norm=10, norm_type=2)), fused=False)  # the Argoverse 2 dicts as they stand
    assert opt.max_norm == 10.0 and opt.group_wd == [0.05, 0.0, 0.05] and opt.initial_lr == [0.2 * 1e-5, 1e-5, 1e-5]
    assert opt.names == list(mults) and "frozen.weight" not in opt.names
    # equal lengths stay alphabetical: "ab" is tried before "bc"
    two = _Named([("abc.weight", 1)])
    assert param_groups(two, dict(custom_keys={"bc": dict(lr_mult=3.0), "ab": dict(lr_mult=2.0)}))[0] == {"abc.weight": (2.0, 1.0)}
    with pytest.raises(NotImplementedError, match="bias_lr_mult"):
        param_groups(toy, dict(bias_lr_mult=2.0))


def test_custom_keys_on_the_detector():
    from conftest import build_test_fsf

    model = build_test_fsf()
    mults, groups = param_groups(model, NUS_OPTIMIZER["paramwise_cfg"])
    assert len(mults) == sum(1 for p in model.parameters() if p.requires_grad)
    slow = [n for n in mults if n.startswith("segmentor.backbone.") or n.startswith("segmentor.voxel_encoder.")]
    assert len(slow) >= 2 and any("backbone" in n for n in slow) and any("voxel_encoder" in n for n in slow)
    for name, pair in mults.items():
        assert pair == ((0.2, 1.0) if name in slow else (1.0, 1.0)), name
    assert sorted(groups) == [(0.2, 1.0), (1.0, 1.0)]
    opt = build_optimizer(FrameDataParallel(model), NUS_OPTIMIZER, NUS_OPTIMIZER_CONFIG, fused=False)
    assert len(opt.groups) == 2 and opt.max_norm == 35.0 and sorted(opt.initial_lr) == [0.2 * 1e-4, 1e-4]
    assert opt.names == list(mults) and [opt.groups[k] for k in opt.group_of] == list(mults.values())


# ------------------------------------------------------------------------------------------------ schedule
def test_cyclic_schedule_closed_form():
    n = 1000
    s = CyclicSchedule(NUS_LR, NUS_MOMENTUM, n)
    up = 400
    cos = lambda a, b, f: b + 0.5 * (a - b) * (math.cos(math.pi * f) + 1)  # noqa: E731
    ok = lambda x: pytest.approx(x, rel=1e-12, abs=0)  # noqa: E731
    assert s.lr(1e-4, 0) == ok(1e-4) and s.lr(1e-4, up) == ok(1e-3)
    assert s.lr(1e-4, up - 1) == ok(cos(1e-4, 1e-3, 399 / 400)) and 9.9e-4 < s.lr(1e-4, up - 1) < 1e-3
    assert s.lr(1e-4, n - 1) == ok(cos(1e-3, 1e-8, 599 / 600)) and 1e-8 < s.lr(1e-4, n - 1) < 2e-8
    low = 0.9 * 0.85 / 0.95
    assert s.momentum(0.9, 0) == ok(0.9) and s.momentum(0.9, up) == ok(low)
    assert s.momentum(0.9, up - 1) == ok(cos(0.9, low, 399 / 400)) and s.momentum(0.9, n - 1) == ok(cos(low, 0.9, 599 / 600))
    assert low < s.momentum(0.9, n - 1) < 0.9 and s.momentum(0.9, n - 1) == pytest.approx(0.9, abs=1e-5)
    assert annealing_cos(3.0, 5.0, 0.0) == 3.0 and annealing_cos(3.0, 5.0, 1.0) == 5.0 and annealing_cos(3.0, 5.0, 0.5) == ok(4.0)
    # Argoverse 2: no momentum schedule
    a = CyclicSchedule(AV2_LR, None, 2400)
    assert a.lr(1e-5, 0) == ok(1e-5) and a.lr(1e-5, 240) == ok(1e-3) and a.lr(1e-5, 239) == ok(cos(1e-5, 1e-3, 239 / 240))
    assert a.lr(1e-5, 2399) == ok(cos(1e-3, 1e-8, 2159 / 2160)) and a.momentum(0.9, 777) == 0.9


def test_schedule_scales_every_group_with_its_own_base_and_sets_beta1():
    toy = _Named([("segmentor.backbone.w", 3), ("head.w", 5)])
    opt = build_optimizer(FrameDataParallel(toy), NUS_OPTIMIZER, NUS_OPTIMIZER_CONFIG, fused=False)
    assert opt.groups == [(0.2, 1.0), (1.0, 1.0)] and opt.initial_lr == [0.2 * 1e-4, 1e-4]
    s = CyclicSchedule(NUS_LR, NUS_MOMENTUM, 50)
    s.apply(opt, 20)  # iter_up
    assert opt.group_lr == pytest.approx([0.2 * 1e-3, 1e-3], rel=1e-12) and opt.beta1 == pytest.approx(0.9 * 0.85 / 0.95, rel=1e-12)
    s.apply(opt, 7)
    assert opt.group_lr[0] == pytest.approx(0.2 * opt.group_lr[1], rel=1e-12) and opt.group_lr[1] == s.lr(1e-4, 7)
    assert opt.initial_lr == [0.2 * 1e-4, 1e-4] and opt.initial_beta1 == 0.9
    CyclicSchedule(AV2_LR, None, 50).apply(opt, 3)
    assert opt.beta1 == 0.9


@pytest.mark.parametrize("what,cfg", [("cyclic_times", dict(NUS_LR, cyclic_times=2)), ("policy", dict(NUS_LR, policy="CosineAnnealing")),
                                      ("anneal_strategy", dict(NUS_LR, anneal_strategy="linear")), ("gamma", dict(NUS_LR, gamma=0.5)),
                                      ("by_epoch", dict(NUS_LR, by_epoch=True))])
def test_schedule_refuses_by_name(what, cfg):
    with pytest.raises(NotImplementedError, match=what):
        CyclicSchedule(cfg, None, 100)
    with pytest.raises(NotImplementedError, match=what):
        CyclicSchedule(NUS_LR, cfg, 100)


# ------------------------------------------------------------------------------------------------ restatement against torch
SIZES = [1, 3, 128, 4097]
TOY_NAMES = [("slow.a", 1), ("plain.b", 3), ("norm.c", 128), ("wide.d", 4097)]
TOY_KEYS = {"slow": dict(lr_mult=0.2), "norm": dict(decay_mult=0.)}
GRAD_SCALE = [1.0, 0.1, 2.0, 0.05, 1.0]  # |g| ~ 65 scale against max_norm 35: clipped on steps 0, 2, 4, not on 1, 3
LRS = [1e-3, 2e-3, 1.5e-3, 5e-4, 1e-3]
BETA1 = [0.9, 0.88, 0.85, 0.87, 0.9]


def toy_grads(steps=5, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(n, generator=g) * GRAD_SCALE[s % 5] for _, n in TOY_NAMES] for s in range(steps)]


def make_toy(fused=False, grad_clip=dict(max_norm=35, norm_type=2), device="cpu", bucket_mb=96):
    toy = _Named(TOY_NAMES).to(device)
    dp = FrameDataParallel(toy, bucket_mb=bucket_mb)
    opt = FusedAdamW(dp, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, paramwise_cfg=dict(custom_keys=TOY_KEYS),
                     grad_clip=grad_clip, fused=fused)
    return toy, dp, opt


def set_grads(opt, grads):
    for p, g in zip(opt.params, grads):
        p.grad.copy_(g)


def torch_route(dtype, grads, steps, max_norm=35):
    """clip_grad_norm_ + torch.optim.AdamW(foreach=False), one group per parameter as mmcv builds them."""
    toy = _Named(TOY_NAMES).to(dtype)
    mults, _ = param_groups(toy, dict(custom_keys=TOY_KEYS))
    params = [p for _, p in toy.named_parameters()]
    opt = torch.optim.AdamW([dict(params=[p], lr=1e-3 * mults[n][0], weight_decay=0.05 * mults[n][1]) for n, p in toy.named_parameters()],
                            lr=1e-3, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    norms = []
    for s in range(steps):
        for grp, (n, p) in zip(opt.param_groups, toy.named_parameters()):
            grp["lr"], grp["betas"] = LRS[s] * mults[n][0], (BETA1[s], 0.999)
        for p, g in zip(params, grads[s]):
            p.grad = g.to(dtype).clone()
        norms.append(torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2, foreach=False))
        opt.step()
    return toy, opt, norms


def restated_route(grads, steps, **kw):
    toy, dp, opt = make_toy(**kw)
    for s in range(steps):
        opt.group_lr = [LRS[s] * lm for lm, _ in opt.groups]
        opt.beta1 = BETA1[s]
        set_grads(opt, grads[s])
        opt.step()
    return toy, dp, opt


def test_restatement_against_torch_through_float64():
    """(i) FusedAdamW(fused=False), (ii) torch fp32, (iii) torch float64; sizes [1, 3, 128, 4097], two lr_mult groups and a
    decay_mult = 0 group, 5 steps, clipping active on steps 0, 2, 4, beta1 and lr changing per step.  max |(i) - (iii)| may be at most
    2 x max |(ii) - (iii)| over the parameters (the factor covers the one differently rounded scalar per group and the float64 norm)."""
    grads = toy_grads()
    toy_i, _, opt_i = restated_route(grads, 5)
    toy_ii, opt_ii, norms = torch_route(torch.float32, grads, 5)
    toy_iii, opt_iii, norms64 = torch_route(torch.float64, grads, 5)
    assert [bool(n > 35) for n in norms64] == [True, False, True, False, True]
    assert opt_i.groups == [(0.2, 1.0), (1.0, 1.0), (1.0, 0.0)]
    ours = max(float((a.detach().double() - c.detach()).abs().max()) for a, c in zip(toy_i.parameters(), toy_iii.parameters()))
    theirs = max(float((b.detach().double() - c.detach()).abs().max()) for b, c in zip(toy_ii.parameters(), toy_iii.parameters()))
    moved = max(float((c.detach() - d.detach().double()).abs().max()) for c, d in zip(toy_iii.parameters(), _Named(TOY_NAMES).parameters()))
    print(f"K39 restatement against float64 torch over 5 steps: restatement {ours:.3e}, torch fp32 {theirs:.3e} (parameters moved by up to {moved:.3e})")
    for k, name in ((2, "exp_avg"), (3, "exp_avg_sq")):
        mo = max(float((opt_i._slots[i][k].double() - opt_iii.state[p][name]).abs().max()) for i, p in enumerate(toy_iii.parameters()))
        mt = max(float((opt_ii.state[q][name].double() - opt_iii.state[p][name]).abs().max()) for q, p in zip(toy_ii.parameters(), toy_iii.parameters()))
        print(f"    {name}: restatement {mo:.3e}, torch fp32 {mt:.3e}")
    assert moved > 1e-3 and theirs > 0
    assert ours <= 2 * theirs


def ulp_distance(a, b):
    """How many f32 steps apart two positive finite f32 values are."""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def exact_norm(flats):
    """f32(sqrt(fsum of squares in float64))."""
    return np.float32(math.sqrt(math.fsum(float(x) * float(x) for f in flats for x in f.double().tolist())))


def test_restated_norm_is_within_one_ulp_of_the_exactly_summed_one():
    """float64 accumulation of n < 2^27 squares (each exact in float64) has a relative error below n 2^-53 < 2^-26, the root halves
    it, the rounding to f32 adds half an ulp: at most 1 ulp from the exactly summed value."""
    grads = toy_grads(steps=3, seed=5)
    toy, dp, opt = make_toy()
    for s in range(3):
        set_grads(opt, grads[s])
        want = exact_norm([b.flat for b in dp.buckets])
        opt.step()
        assert ulp_distance(opt.grad_norm.item(), want) <= 1, (opt.grad_norm.item(), want)
    assert all(float(b.flat.abs().max()) == 0.0 for b in dp.buckets)  # zero_grads=True is the default


def test_one_infinite_gradient_element_as_torch_makes_it():
    """norm = inf, coef = 0: that element's gradient is inf * 0 = NaN, every other one 0.  torch stores the clipped gradient; here it
    is applied on the fly and shows in exp_avg (= lerp(0, g, w): NaN there, 0 elsewhere) and in the parameters."""
    grads = toy_grads(steps=1)
    grads[0][3][1234] = float("inf")
    toy_i, dp, opt_i = restated_route(grads, 1)
    toy_ii, opt_ii, norms = torch_route(torch.float32, grads, 1)
    assert math.isinf(float(norms[0])) and math.isinf(opt_i.grad_norm.item())
    for i, (a, b) in enumerate(zip(toy_i.parameters(), toy_ii.parameters())):
        nan = torch.isnan(b)
        assert int(nan.sum()) == (1 if i == 3 else 0) and torch.equal(torch.isnan(a), nan)
        assert torch.equal(a.detach()[~nan], b.detach()[~nan])  # (p * decay, then - step * 0: the same single rounding)
        eff, clipped = opt_i._slots[i][2], b.grad
        assert torch.equal(torch.isnan(eff), torch.isnan(clipped)) and torch.equal(torch.isnan(clipped), nan)
        assert float(eff[~nan].abs().max() if (~nan).any() else 0.0) == 0.0 and float(clipped[~nan].abs().max() if (~nan).any() else 0.0) == 0.0
    assert all(float(b.flat.abs().max()) == 0.0 for b in dp.buckets)  # consumed and cleared, the infinite one included


# ------------------------------------------------------------------------------------------------ checkpoints
def torch_optimizer_for(toy, betas=(0.9, 0.999)):
    return torch.optim.AdamW([dict(params=[p]) for p in toy.parameters()], lr=1e-3, betas=betas, eps=1e-8, weight_decay=0.05, foreach=False)


def test_state_dict_round_trip_with_torch_and_a_bit_identical_resume():
    grads = toy_grads(steps=4, seed=3)
    sched = CyclicSchedule(dict(NUS_LR), dict(NUS_MOMENTUM), 4)

    def run(opt, steps):
        for s in steps:
            sched.apply(opt, s)
            set_grads(opt, grads[s])
            opt.step()

    toy_a, _, opt_a = make_toy()
    run(opt_a, range(4))
    toy_b, _, opt_b = make_toy()
    run(opt_b, range(2))
    sd = opt_b.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    assert [g["params"] for g in sd["param_groups"]] == [[0], [1], [2], [3]] and float(sd["state"][3]["step"]) == 2.0
    assert [g["weight_decay"] for g in sd["param_groups"]] == [0.05, 0.05, 0.0, 0.05]
    assert sd["param_groups"][0]["lr"] == pytest.approx(0.2 * sd["param_groups"][1]["lr"], rel=1e-12)
    assert sd["param_groups"][1]["betas"] == (opt_b.beta1, 0.999) and sd["state"][3]["exp_avg"].shape == (4097,)
    # -> torch.optim.AdamW (one group per parameter) -> its own state_dict -> a fresh FusedAdamW on a copy of the parameters
    toy_t = _Named(TOY_NAMES)
    toy_t.load_state_dict(toy_b.state_dict())
    topt = torch_optimizer_for(toy_t)
    topt.load_state_dict(sd)
    assert [g["lr"] for g in topt.param_groups] == [g["lr"] for g in sd["param_groups"]]
    assert torch.equal(topt.state[toy_t.wide.d]["exp_avg"], sd["state"][3]["exp_avg"])
    toy_c, _, opt_c = make_toy()
    toy_c.load_state_dict(toy_b.state_dict())
    opt_c.load_state_dict(topt.state_dict())
    assert opt_c.step_count == 2 and opt_c.group_lr == opt_b.group_lr and opt_c.beta1 == opt_b.beta1 and opt_c.initial_lr == opt_b.initial_lr
    run(opt_c, range(2, 4))
    for a, c in zip(toy_a.parameters(), toy_c.parameters()):
        assert torch.equal(a, c)
    for sa, sc in zip(opt_a._slots, opt_c._slots):
        assert torch.equal(sa[2], sc[2]) and torch.equal(sa[3], sc[3])
    # the loaded torch optimizer steps from that state too: one step of each from the same point agree to rounding
    toy_d, _, opt_d = make_toy()
    toy_d.load_state_dict(toy_b.state_dict())
    opt_d.load_state_dict(sd)
    opt_d.max_norm = None
    set_grads(opt_d, grads[2])
    opt_d.step()
    for p, g in zip(toy_t.parameters(), grads[2]):
        p.grad = g.clone()
    topt.step()
    for d, t in zip(toy_d.parameters(), toy_t.parameters()):
        assert float((d.detach() - t.detach()).abs().max()) <= 1e-6
    # a torch optimizer that stepped on its own loads too
    opt_d.load_state_dict(topt.state_dict())
    assert opt_d.step_count == 3 and torch.equal(opt_d._slots[3][2], topt.state[toy_t.wide.d]["exp_avg"])
    uneven = topt.state_dict()
    uneven["state"][1]["step"] = torch.tensor(7.0)
    with pytest.raises(NotImplementedError, match="step counts"):
        opt_d.load_state_dict(uneven)


# ------------------------------------------------------------------------------------------------ refusals
def test_what_is_not_built_is_refused_by_name():
    dp = FrameDataParallel(_Named(TOY_NAMES))
    with pytest.raises(NotImplementedError, match="amsgrad"):
        FusedAdamW(dp, lr=1e-3, amsgrad=True, fused=False)
    with pytest.raises(NotImplementedError, match="maximize"):
        FusedAdamW(dp, lr=1e-3, maximize=True, fused=False)
    with pytest.raises(NotImplementedError, match="norm_type"):
        FusedAdamW(dp, lr=1e-3, grad_clip=dict(max_norm=35, norm_type=1), fused=False)
    with pytest.raises(NotImplementedError, match="SGD"):
        build_optimizer(dp, dict(type="SGD", lr=0.1, momentum=0.9), NUS_OPTIMIZER_CONFIG, fused=False)
    with pytest.raises(NotImplementedError, match="Fp16OptimizerHook"):
        build_optimizer(dp, NUS_OPTIMIZER, dict(type="Fp16OptimizerHook", grad_clip=None), fused=False)
    with pytest.raises(NotImplementedError, match="FSF_OPTIM_MAX_GROUPS"):
        FusedAdamW(FrameDataParallel(_Named([(f"k{i}.w", 1) for i in range(9)])), lr=1e-3, fused=False,
                   paramwise_cfg=dict(custom_keys={f"k{i}": dict(lr_mult=1.0 + i) for i in range(9)}))
    with pytest.raises(TypeError, match="FrameDataParallel"):
        FusedAdamW(_Named(TOY_NAMES), lr=1e-3, fused=False)
    FusedAdamW(dp, lr=1e-3, amsgrad=False, maximize=False, foreach=None, fused=False)  # the spelled-out defaults pass


def test_half_precision_parameters_are_refused_by_name():
    class _DP:  # (FrameDataParallel itself asserts f32 buckets: the optimizer's own check, on a stand-in)
        def __init__(self, module):
            self.module, self.buckets = module, []

    with pytest.raises(NotImplementedError, match="float16"):
        FusedAdamW(_DP(_Named(TOY_NAMES).half()), lr=1e-3, fused=False)


# ------------------------------------------------------------------------------------------------ C ABI surface and guard-band cover
def test_entry_points_are_declared_documented_and_the_abi_version_stays():
    from fullysparsefusion_amd import _lib

    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for name in ("fsf_optim_grad_sumsq", "fsf_optim_adamw_step", "fsf_optim_workspace_bytes", "fsf_optim_table_bytes"):
        assert name in _lib.SIGNATURES and name in doc, name
    for name in ("FSF_OPTIM_CHUNK", "FSF_OPTIM_MAX_PARTIALS", "FSF_OPTIM_MAX_GROUPS", "FSF_OPTIM_TABLE_WORDS"):
        assert name in _lib.DEFINES, name
    assert _lib.DEFINES["FSF_ABI_VERSION"] == 23
    assert _lib.DEFINES["FSF_OPTIM_CHUNK"] % 1024 == 0 and _lib.DEFINES["FSF_OPTIM_MAX_GROUPS"] == 8
    args = _lib.SIGNATURES["fsf_optim_adamw_step"][0]
    assert len(args) == 17 and args[3] is _lib.c_p and args[4] is _lib.c_p and args[5:11] == [_lib.c_f32] * 6  # host arrays, f32 scalars


def test_chunk_rows_cover_every_element_once():
    rows = optim.chunk_rows([(4096, 8192, 12288, 16384, 10, 0), (40960, 81920, 122880, 163840, 2 * 4096 + 5, 3), (64, 128, 192, 256, 4096, 1)],
                            4096).numpy()
    assert rows.shape == (5, 5) and (rows[:, 4] & 0xFFFFFFFF).tolist() == [10, 4096, 4096, 5, 4096] and (rows[:, 4] >> 32).tolist() == [0, 3, 3, 3, 1]
    assert rows[1:4, 0].tolist() == [40960, 40960 + 16384, 40960 + 32768] and rows[3, 3] == 163840 + 32768
    assert optim.chunk_rows([], 4096).shape == (0, 5) and optim.chunk_rows([(8, 8, 8, 8, 0, 0)], 4096).shape == (0, 5)


_ALLOCATES = re.compile(r"torch\.empty|empty_like|torch\.zeros|torch\.full|_lib\.workspace\(|_workspace_bytes|_arena_bytes")
_SCRATCH = re.compile(r"_lib\.workspace\(|_workspace_bytes|_arena_bytes")


def test_every_allocating_wrapper_of_the_new_module_has_guard_band_cases():
    import test_guard_bands_optim_gpu as gb
    from fullysparsefusion_amd import hip_ops_optim

    with open(os.path.join(ROOT, "fullysparsefusion_amd", "hip_ops_optim.py")) as f:
        src = f.read()
    alloc, scratch = set(), set()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef):
            body = ast.get_source_segment(src, node)
            if _ALLOCATES.search(body):
                alloc.add(node.name)
                if _SCRATCH.search(body):
                    scratch.add(node.name)
    assert alloc == {"chunk_table", "adamw_step"} and scratch == {"adamw_step"}
    assert sorted(alloc - set(gb.CASES)) == []
    for name, cases in gb.CASES.items():
        assert hasattr(hip_ops_optim, name)
        kinds = [k for k, _ in cases]
        assert "ragged" in kinds and "minimal" in kinds and "empty" in kinds, name
    assert not re.search(r"torch\.zeros|torch\.full|empty_like|torch\.ones|new_zeros|new_empty|new_full", src)
