"""The optimizer step on the nuScenes model's gradient buckets, two routes alternating in one process (docs/kernels/K39_optimizer_step.md):
  (a) torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(fused=True) + dp.zero_grad()  — existing code, the baseline;
  (b) FusedAdamW.step()  — K39a + K39b, gradient cleared in the same pass.
No forward pass: before every step the same random numbers are copied into the buckets (outside the timed window).  Per route: the
device span of one step (events around it, median and spread over ROUNDS x ITERS steps), the host time to issue it, the launches of
one step (torch.profiler, after the timed rounds) and for (b) the bytes K39 must move over the span, beside the 6.29 TB/s of a float4
copy (MI355X_MICROARCH.md).  (a) gets the TWO (lr, weight decay) groups of the nuScenes recipe, not mmcv's group per parameter."""
import copy
import os
import sys
import time

import torch

ROOT = os.path.abspath(os.environ.get("FSF_ROOT") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
from fullysparsefusion_amd import mmdet3d_plugin  # noqa: E402
from fullysparsefusion_amd.compat import Config  # noqa: E402
from fullysparsefusion_amd.data_parallel import FrameDataParallel  # noqa: E402
from fullysparsefusion_amd.optim import CyclicSchedule, build_optimizer  # noqa: E402

ROUNDS, ITERS = int(os.environ.get("ROUNDS", 7)), int(os.environ.get("ITERS", 20))
OPTIMIZER = dict(type="AdamW", lr=1e-4, weight_decay=0.01,
                 paramwise_cfg=dict(custom_keys={"segmentor.backbone": dict(lr_mult=0.2), "segmentor.voxel_encoder": dict(lr_mult=0.2)}))
OPTIMIZER_CONFIG = dict(grad_clip=dict(max_norm=35, norm_type=2))
LR = dict(policy="cyclic", target_ratio=(10, 1e-4), cyclic_times=1, step_ratio_up=0.4)
MOMENTUM = dict(policy="cyclic", target_ratio=(0.85 / 0.95, 1), cyclic_times=1, step_ratio_up=0.4)

if not torch.cuda.is_available():
    raise SystemExit("optim_step_bench.py needs a HIP device")
dev = torch.device("cuda:0")
torch.manual_seed(0)
model_b = mmdet3d_plugin.build_model(Config.fromfile(os.path.join(ROOT, "configs", "fsf_nuscenes.py")).model).to(dev)
model_a = copy.deepcopy(model_b)
dp_a, dp_b = FrameDataParallel(model_a), FrameDataParallel(model_b)
opt_b = build_optimizer(dp_b, OPTIMIZER, OPTIMIZER_CONFIG)
sched = CyclicSchedule(LR, MOMENTUM, 10 ** 6)
params_a = [p for p in model_a.parameters() if p.requires_grad]
by_group = {}
for i, p in enumerate(params_a):
    by_group.setdefault(opt_b.group_of[i], []).append(p)
opt_a = torch.optim.AdamW([dict(params=ps, lr=opt_b.initial_lr[k], weight_decay=opt_b.group_wd[k]) for k, ps in sorted(by_group.items())],
                          lr=1e-4, fused=True)
noise = [torch.randn_like(b.flat) * 0.01 for b in dp_b.buckets]  # |g| ~ 0.01 sqrt(n) ~ 90: clipping is active
n = sum(p.numel() for p in params_a)
it = [0]


def step_a():
    torch.nn.utils.clip_grad_norm_(params_a, 35, norm_type=2)
    opt_a.step()
    dp_a.zero_grad()


def step_b():
    it[0] += 1
    sched.apply(opt_b, it[0])
    opt_b.step()


def refill(dp):
    for b, x in zip(dp.buckets, noise):
        b.flat.copy_(x)


def timed(step, dp):
    """(device span us, host issue us) of each of ITERS steps."""
    spans, hosts = [], []
    for _ in range(ITERS):
        refill(dp)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        step()
        e1.record()
        hosts.append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
        spans.append(e0.elapsed_time(e1) * 1e3)
    return spans, hosts


def launches(step, dp):
    """Device kernels (and memsets / copies) one step enqueues, counted by torch.profiler; None where the profiler gives nothing."""
    refill(dp)
    torch.cuda.synchronize()
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        count = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return count or None
    except Exception as exc:  # noqa: BLE001
        print(f"# torch.profiler: {type(exc).__name__}: {exc}")
        return None


for step, dp in ((step_a, dp_a), (step_b, dp_b)):  # warm-up: code objects, optimizer state, scratch
    for _ in range(3):
        refill(dp)
        step()
torch.cuda.synchronize()
med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
res = {"a": ([], []), "b": ([], [])}
for _ in range(ROUNDS):
    for key, step, dp in (("a", step_a, dp_a), ("b", step_b, dp_b)):
        spans, hosts = timed(step, dp)
        res[key][0].append(med(spans))
        res[key][1].append(med(hosts))
count = {"a": launches(step_a, dp_a), "b": launches(step_b, dp_b)}
moved = 36 * n  # K39a reads g (4 n); K39b reads p, g, m, v and writes p, m, v, g (32 n)
print(f"# nuScenes FSF: {n} trainable elements in {len(params_a)} tensors, {len(dp_b.buckets)} buckets, {opt_b.table.size(0)} table rows "
      f"of <= {opt_b._ops.CHUNK}; {len(opt_b.groups)} (lr, weight decay) groups")
print(f"# us per optimizer step: median over {ROUNDS} rounds of the median of {ITERS} steps, the two routes alternating; spread = max - min "
      "of the round medians")
print(f"# {'route':58s} | {'device span':>11s} {'(spread)':>9s} | {'host issue':>10s} | launches")
for key, label in (("a", "(a) clip_grad_norm_ + AdamW(fused=True) + dp.zero_grad()"), ("b", "(b) FusedAdamW.step()  [K39a + K39b]")):
    spans, hosts = res[key]
    print(f"  {label:58s} | {med(spans):11.1f} ({max(spans) - min(spans):7.1f}) | {med(hosts):10.1f} | {count[key] if count[key] else 'n/a'}")
span_b = med(res["b"][0])
print(f"# (b) must move 36 bytes per element = {moved / 1e9:.3f} GB: {moved / span_b / 1e6:.2f} TB/s over its device span, "
      f"{100 * moved / span_b / 1e6 / 6.29:.0f} % of the 6.29 TB/s of a float4 copy")
print(f"# (b) - (a) device span: {span_b - med(res['a'][0]):+.1f} us; host issue: {med(res['b'][1]) - med(res['a'][1]):+.1f} us")
