"""The optimizer step of the reference's training recipe on `FrameDataParallel`'s gradient buckets (K39,
docs/kernels/K39_optimizer_step.md).

Stands in for what the reference gets from mmcv: `DefaultOptimizerConstructor` (`paramwise_cfg.custom_keys`) around
`torch.optim.AdamW`, `OptimizerHook(grad_clip=dict(max_norm=..., norm_type=2))` and the cyclic learning-rate / momentum hooks
(projects/configs/_base_/schedules/cyclic_20e.py, cosine_2x.py and the two FSF configs).

  * `param_groups(model, paramwise_cfg)`   mmcv's `custom_keys` rule -> per-parameter (lr_mult, decay_mult) and the distinct groups
  * `FusedAdamW(dp, ...)`                  clip + AdamW + gradient clear: two HIP launches per step (one without clipping), no host wait
  * `CyclicSchedule(lr_config, momentum_config, max_iters)`   the per-iteration learning rates and beta1
  * `build_optimizer(dp, optimizer, optimizer_config)`        from the reference's dicts as they stand

`fused=False` is the torch restatement of the same arithmetic on the same buckets (it also runs on CPU tensors); it DEFINES what the
kernels compute, and the device tests hold the two to the same bits.
"""
import math

import numpy as np
import torch

_PARAMWISE_NOT_BUILT = ("bias_lr_mult", "bias_decay_mult", "norm_decay_mult", "dwconv_decay_mult", "dcn_offset_lr_mult",
                        "bypass_duplicate")


def _f32(x):
    """A double rounded to the nearest f32, as a Python float: what the kernels are handed."""
    return float(np.float32(x))


def param_groups(model, paramwise_cfg=None):
    """mmcv's `DefaultOptimizerConstructor.add_params` for `custom_keys`, restated: the keys sorted alphabetically, then by length with
    the longest first (a stable sort, so equal lengths stay alphabetical); the FIRST key that is a substring of a parameter's full
    name decides its `lr_mult` / `decay_mult` (1 where the entry does not name one), no key leaves both at 1.
    -> ({name: (lr_mult, decay_mult)} over the trainable parameters in `named_parameters()` order, [distinct pairs, first seen first])."""
    cfg = dict(paramwise_cfg or {})
    custom = cfg.pop("custom_keys", {})
    for key in cfg:
        raise NotImplementedError(f"paramwise_cfg: '{key}' is not built (only custom_keys with lr_mult / decay_mult is)"
                                  if key in _PARAMWISE_NOT_BUILT else f"paramwise_cfg: unknown option '{key}'")
    for key, entry in custom.items():
        for opt in entry:
            if opt not in ("lr_mult", "decay_mult"):
                raise NotImplementedError(f"paramwise_cfg.custom_keys['{key}']: '{opt}' is not built (lr_mult and decay_mult are)")
    keys = sorted(sorted(custom), key=len, reverse=True)
    mults, groups = {}, []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        pair = (1.0, 1.0)
        for key in keys:
            if key in name:
                pair = (float(custom[key].get("lr_mult", 1.0)), float(custom[key].get("decay_mult", 1.0)))
                break
        mults[name] = pair
        if pair not in groups:
            groups.append(pair)
    return mults, groups


def chunk_rows(entries, chunk):
    """The host form of K39's chunk table: `entries` = (parameter address, gradient address, exp_avg address, exp_avg_sq address,
    element count, group id) per parameter -> i64 [n, 5], one row per `chunk` elements of a parameter (the last row of a parameter
    takes the rest), word 4 = count | group << 32."""
    rows = []
    for p, g, m, v, numel, group in entries:
        assert numel >= 0 and 0 <= group < (1 << 31) and all(a % 4 == 0 for a in (p, g, m, v))
        start = np.arange(0, numel, chunk, dtype=np.int64)
        count = np.minimum(numel - start, chunk)
        rows.append(np.stack([p + 4 * start, g + 4 * start, m + 4 * start, v + 4 * start, count | (np.int64(group) << 32)], 1))
    rows = np.concatenate(rows) if rows else np.zeros((0, 5), np.int64)
    return torch.from_numpy(np.ascontiguousarray(rows.reshape(-1, 5)))


class FusedAdamW:
    """AdamW with the reference's global-norm gradient clip on a `FrameDataParallel`'s gradient buckets.

    `step(zero_grads=True)` runs after `dp.backward(loss)` (or `loss.backward()` + `dp.finish()`): K39a sums the squares of every
    bucket as float64 partials, K39b forms the clip coefficient, steps every parameter and clears the gradient element it consumed
    — two launches whatever the number of buckets and parameters (one with `grad_clip=None`), nothing waits for the device.
    `grad_norm` (f32 [1] on the device) holds the last step's gradient norm before clipping, for logging; without clipping it is never
    written.  The parameters stay where they are (conv weight planes and other caches hold their addresses): a device table of
    fixed-size chunks, built here once, carries each parameter's address beside its slice of the gradient bucket and of the two flat
    state buffers `exp_avg[b]` / `exp_avg_sq[b]` (one pair per bucket, the bucket's offsets).  Build the optimizer AFTER the model is on
    its device; a parameter whose storage moved afterwards is refused at the next `step()`.

    The arithmetic per element is the order of torch's single-tensor AdamW, every operation rounded on its own:
        g = g_raw * coef;  p *= f32(1 - lr * wd);  m = lerp(m, g, f32(1 - beta1));  v = v * f32(beta2) + (f32(1 - beta2) * g) * g
        denom = sqrt(v) / f32(sqrt(1 - beta2^t)) + f32(eps);  p -= f32(lr / (1 - beta1^t)) * (m / denom)
    with coef = min(f32(max_norm) / (norm + 1e-6f), 1), norm = f32(sqrt(float64 sum of squares)) — `clip_grad_norm_`'s rule.
    `fused=False` runs exactly this as torch operations (`_step_restated`), on CPU tensors too.

    `zero_grads=True` (the default) makes `dp.zero_grad()` unnecessary: do NOT call it.  `param.grad` stay the bucket views, so the next
    forward's `_arm(zero=False)` finds them in place and the next backward adds onto zeros.  `zero_grads=False` leaves the gradient
    bits alone (the clip coefficient is applied on the fly, never stored), for a caller that wants to look at them.

    Where this differs from torch / mmcv:
      * EVERY trainable parameter steps on EVERY iteration, with one global step count.  A parameter that received no gradient has a
        zero gradient (`FrameDataParallel`'s standing contract), so its moments decay and weight decay applies; torch and the
        reference skip a parameter whose `.grad` is None and keep a step count per parameter.
      * the clip coefficient is one division, max_norm / (norm + 1e-6); torch's `max_norm / tensor` is a reciprocal and a product.
      * the scalars 1 - lr * wd, lr / (1 - beta1^t), sqrt(1 - beta2^t) are computed in double and rounded ONCE to f32; lerp and addcmul /
        addcdiv are stated as separately rounded operations where torch's kernels may contract to fma.
    Refused by name: amsgrad, maximize, a norm_type other than 2, error_if_nonfinite, parameters that are not f32, more than
    FSF_OPTIM_MAX_GROUPS (lr, weight decay) groups, paramwise options other than custom_keys' lr_mult / decay_mult."""

    def __init__(self, dp, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, paramwise_cfg=None, grad_clip=None, fused=True, **options):
        harmless = dict(amsgrad=False, maximize=False, capturable=False, differentiable=False, foreach=None, decoupled_weight_decay=True)
        for name, value in options.items():
            if not (name in harmless and value is harmless[name]):
                raise NotImplementedError(f"FusedAdamW: {name}={value!r} is not built")
        if not hasattr(dp, "buckets"):
            raise TypeError("FusedAdamW steps on a FrameDataParallel's gradient buckets: wrap the model first (a world of 1 needs no "
                            "process group)")
        self.max_norm = None
        if grad_clip is not None:
            clip = dict(grad_clip)
            if float(clip.pop("norm_type", 2)) != 2.0:
                raise NotImplementedError(f"FusedAdamW: grad_clip norm_type={grad_clip['norm_type']!r} is not built (norm_type=2 is)")
            if clip.pop("error_if_nonfinite", False):
                raise NotImplementedError("FusedAdamW: grad_clip error_if_nonfinite=True is not built (it needs a host wait)")
            clip.pop("foreach", None)
            self.max_norm = float(clip.pop("max_norm"))
            for key in clip:
                raise NotImplementedError(f"FusedAdamW: grad_clip option '{key}' is not built")
        self.dp, self.fused = dp, bool(fused)
        named = [(n, p) for n, p in dp.module.named_parameters() if p.requires_grad]
        self.names, self.params = [n for n, _ in named], [p for _, p in named]
        for n, p in named:
            if p.dtype != torch.float32:
                raise NotImplementedError(f"FusedAdamW: parameter '{n}' is {p.dtype}; only float32 parameters are built")
        mults, self.groups = param_groups(dp.module, paramwise_cfg)
        if len(self.groups) > self._max_groups():
            raise NotImplementedError(f"FusedAdamW: {len(self.groups)} distinct (lr_mult, decay_mult) groups, FSF_OPTIM_MAX_GROUPS is "
                                      f"{self._max_groups()}")
        self.group_of = [self.groups.index(mults[n]) for n in self.names]
        self.base_lr, self.weight_decay, self.eps = float(lr), float(weight_decay), float(eps)
        self.initial_lr = [self.base_lr * lm for lm, _ in self.groups]  # what a schedule scales
        self.group_lr = list(self.initial_lr)                           # what the next step() uses
        self.group_wd = [self.weight_decay * dm for _, dm in self.groups]
        self.initial_beta1, self.beta1, self.beta2 = float(betas[0]), float(betas[0]), float(betas[1])
        self.step_count = 0
        index = {id(p): i for i, p in enumerate(self.params)}
        assert sorted(index[id(p)] for b in dp.buckets for p in b.params) == list(range(len(self.params))), \
            "the buckets hold every trainable parameter once"
        self.exp_avg = [torch.zeros_like(b.flat) for b in dp.buckets]
        self.exp_avg_sq = [torch.zeros_like(b.flat) for b in dp.buckets]
        self._slots = [None] * len(self.params)  # parameter index -> (parameter, gradient view, exp_avg view, exp_avg_sq view)
        for b, m, v in zip(dp.buckets, self.exp_avg, self.exp_avg_sq):
            off = 0
            for p, view in zip(b.params, b.views):
                n = p.numel()
                self._slots[index[id(p)]] = (p, view, m[off:off + n].view_as(p), v[off:off + n].view_as(p))
                off += n
        device = self.params[0].device if self.params else torch.device("cpu")
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=device)
        self.table, self._addresses = None, None
        if self.fused and self.params:
            from . import hip_ops_optim

            self._ops = hip_ops_optim
            entries = [(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), self.group_of[i])
                       for i, (p, g, m, v) in enumerate(self._slots)]
            for n, p in named:
                if not p.is_contiguous():
                    raise NotImplementedError(f"FusedAdamW: parameter '{n}' is not contiguous")
            self._addresses = [e[0] for e in entries]
            self.table = hip_ops_optim.chunk_table(chunk_rows(entries, hip_ops_optim.CHUNK), device)

    @staticmethod
    def _max_groups():
        from . import _lib

        return _lib.DEFINES["FSF_OPTIM_MAX_GROUPS"]

    # ------------------------------------------------------------------------------------------------ the step
    def scalars(self):
        """The step's scalars as the kernels get them: computed in double from the current `group_lr` / `beta1` and the step count,
        each rounded once to f32."""
        t, b1, b2 = self.step_count, self.beta1, self.beta2
        bc1 = 1.0 - b1 ** t
        return dict(decay=[_f32(1.0 - lr * wd) for lr, wd in zip(self.group_lr, self.group_wd)],
                    step=[_f32(lr / bc1) for lr in self.group_lr], w=_f32(1.0 - b1), beta2=_f32(b2), omb2=_f32(1.0 - b2),
                    bc2_sqrt=_f32(math.sqrt(1.0 - b2 ** t)), eps=_f32(self.eps),
                    max_norm=None if self.max_norm is None else _f32(self.max_norm))

    @torch.no_grad()
    def step(self, zero_grads=True):
        if not self.params:  # nothing trainable: nothing to launch
            return
        self.step_count += 1
        s = self.scalars()
        if not self.fused:
            return self._step_restated(s, zero_grads)
        for i, p in enumerate(self.params):
            if p.data_ptr() != self._addresses[i]:
                raise RuntimeError(f"FusedAdamW: the storage of parameter '{self.names[i]}' moved after the optimizer was built (the "
                                   "chunk table holds its address): build the optimizer after the model is placed")
        self._ops.adamw_step(self.table, s["decay"], s["step"], s["w"], s["beta2"], s["omb2"], s["bc2_sqrt"], s["eps"], s["max_norm"],
                             zero_grads, self.grad_norm)

    def _step_restated(self, s, zero_grads):
        """K39 in torch operations, each of them one rounding: the definition the kernels are tested against."""
        coef = None
        if s["max_norm"] is not None:
            total = None
            for b in self.dp.buckets:
                part = b.flat.double().square().sum()
                total = part if total is None else total + part
            if total is None:
                return
            norm = total.sqrt().float()
            c = torch.full((), s["max_norm"], dtype=torch.float32, device=norm.device) / (norm + _f32(1e-6))
            coef = torch.clamp(c, max=1.0)
            self.grad_norm.copy_(norm.reshape(1))
        w = np.float32(s["w"])
        one_minus_w = float(np.float32(1.0) - w)
        for i, (p, g_raw, m, v) in enumerate(self._slots):
            k = self.group_of[i]
            g = g_raw * coef if coef is not None else g_raw
            p.mul_(s["decay"][k])
            d = g - m
            if w < 0.5:
                m.add_(d * s["w"])
            else:
                m.copy_(g - d * one_minus_w)
            v.mul_(s["beta2"]).add_((g * s["omb2"]) * g)
            # (a division by a Python scalar may run as a product with its reciprocal: divide by a tensor)
            denom = v.sqrt() / torch.full((), s["bc2_sqrt"], dtype=torch.float32, device=v.device) + s["eps"]
            p.sub_((m / denom) * s["step"][k])
            if zero_grads:
                g_raw.zero_()

    # ------------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """torch's optimizer layout with ONE param group per trainable parameter in `named_parameters()` order, as mmcv's constructor
        builds them under a paramwise_cfg: `state[i] = {step, exp_avg, exp_avg_sq}` (copies, parameter-shaped), and each group carries
        its own lr, weight_decay and betas — a `torch.optim.AdamW` built that way loads it, and `load_state_dict` takes that one's."""
        state, groups = {}, []
        for i, (p, _, m, v) in enumerate(self._slots):
            k = self.group_of[i]
            state[i] = dict(step=torch.tensor(float(self.step_count), dtype=torch.float32), exp_avg=m.detach().clone(),
                            exp_avg_sq=v.detach().clone())
            groups.append(dict(lr=self.group_lr[k], betas=(self.beta1, self.beta2), eps=self.eps, weight_decay=self.group_wd[k],
                               amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                               decoupled_weight_decay=True, initial_lr=self.initial_lr[k], params=[i]))
        return dict(state=state, param_groups=groups)

    @torch.no_grad()
    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        order = [i for g in groups for i in g["params"]]
        if order != list(range(len(self.params))) or any(len(g["params"]) != 1 for g in groups):
            raise ValueError("FusedAdamW.load_state_dict: expected one param group per trainable parameter, in named_parameters() order "
                             f"({len(self.params)} parameters, got {len(groups)} groups over {len(order)})")
        for g in groups:
            if g.get("amsgrad") or g.get("maximize"):
                raise NotImplementedError("FusedAdamW.load_state_dict: amsgrad / maximize is not built")
        steps = {int(float(st["step"])) for st in sd["state"].values()}
        if len(steps) > 1:
            raise NotImplementedError(f"FusedAdamW.load_state_dict: per-parameter step counts {sorted(steps)} (one global step count is built)")
        if sd["state"] and sorted(sd["state"]) != list(range(len(self.params))):
            raise NotImplementedError("FusedAdamW.load_state_dict: state for some parameters only (every parameter steps on every iteration)")
        betas = {tuple(float(x) for x in g["betas"]) for g in groups}
        eps = {float(g["eps"]) for g in groups}
        if len(betas) > 1 or len(eps) > 1:
            raise NotImplementedError("FusedAdamW.load_state_dict: betas / eps that differ between parameters")
        for k in range(len(self.groups)):
            mine = [groups[i] for i in range(len(self.params)) if self.group_of[i] == k]
            for name in ("lr", "weight_decay"):
                if len({float(g[name]) for g in mine}) > 1:
                    raise NotImplementedError(f"FusedAdamW.load_state_dict: '{name}' differs inside the (lr_mult, decay_mult) group "
                                              f"{self.groups[k]}")
            self.group_lr[k], self.group_wd[k] = float(mine[0]["lr"]), float(mine[0]["weight_decay"])
            self.initial_lr[k] = float(mine[0].get("initial_lr", self.initial_lr[k]))
        if betas:
            self.beta1, self.beta2 = betas.pop()
            self.eps = eps.pop()
        self.step_count = steps.pop() if steps else 0
        for i, (_, _, m, v) in enumerate(self._slots):
            st = sd["state"].get(i)
            if st is None:
                m.zero_(), v.zero_()
            else:
                m.copy_(st["exp_avg"]), v.copy_(st["exp_avg_sq"])


def annealing_cos(start, end, factor):
    """mmcv's: end + 0.5 (start - end) (cos(pi factor) + 1)."""
    return end + 0.5 * (start - end) * (math.cos(math.pi * factor) + 1.0)


class CyclicSchedule:
    """mmcv's CyclicLrUpdaterHook / CyclicMomentumUpdaterHook for one cycle (`cyclic_times == 1`), by iteration:
    iter_up = int(step_ratio_up * max_iters); ratio 1 -> target_ratio[0] over [0, iter_up), target_ratio[0] -> target_ratio[1] over
    [iter_up, max_iters), value(i) = annealing_cos(base * start_ratio, base * end_ratio, (i - start) / (end - start)) — applied to every
    group's initial learning rate and, with a momentum config, to the optimizer's initial beta1.  `apply(optimizer, it)` sets the
    scalars of the NEXT `step()`; host arithmetic only.  Other policies, cyclic_times, anneal strategies, gamma, warm-up and by_epoch are
    refused by name: mmcv versions differ there."""

    def __init__(self, lr_config, momentum_config, max_iters):
        self.max_iters = int(max_iters)
        assert self.max_iters >= 1
        self.lr_phases = self._phases(lr_config, "lr_config", (10, 1e-4))
        self.momentum_phases = None if momentum_config is None else self._phases(momentum_config, "momentum_config", (0.85 / 0.95, 1))

    def _phases(self, cfg, what, default_ratio):
        cfg = dict(cfg)
        policy = cfg.pop("policy", None)
        if policy not in ("cyclic", "Cyclic"):
            raise NotImplementedError(f"CyclicSchedule: {what} policy={policy!r} is not built (policy='cyclic' is)")
        times = cfg.pop("cyclic_times", 1)
        if times != 1:
            raise NotImplementedError(f"CyclicSchedule: {what} cyclic_times={times!r} is not built (cyclic_times=1 is)")
        ratio = tuple(cfg.pop("target_ratio", default_ratio))
        up = float(cfg.pop("step_ratio_up", 0.4))
        if len(ratio) != 2 or not 0.0 <= up < 1.0:
            raise ValueError(f"CyclicSchedule: {what} needs target_ratio of two values and 0 <= step_ratio_up < 1")
        allowed = dict(by_epoch=False, anneal_strategy="cos", gamma=1, warmup=None)
        for key, value in cfg.items():
            if key not in allowed or value != allowed[key]:
                raise NotImplementedError(f"CyclicSchedule: {what} {key}={value!r} is not built")
        iter_up = int(up * self.max_iters)
        return [(0, iter_up, 1.0, float(ratio[0])), (iter_up, self.max_iters, float(ratio[0]), float(ratio[1]))]

    def value(self, base, it, phases=None):
        cur = int(it) % self.max_iters
        for start, end, r0, r1 in (self.lr_phases if phases is None else phases):
            if start <= cur < end:
                return annealing_cos(base * r0, base * r1, (cur - start) / (end - start))
        raise AssertionError("the phases cover [0, max_iters)")

    def lr(self, base, it):
        return self.value(base, it, self.lr_phases)

    def momentum(self, base, it):
        return base if self.momentum_phases is None else self.value(base, it, self.momentum_phases)

    def apply(self, optimizer, it):
        optimizer.group_lr = [self.lr(base, it) for base in optimizer.initial_lr]
        optimizer.beta1 = self.momentum(optimizer.initial_beta1, it)


def build_optimizer(dp, optimizer, optimizer_config=None, fused=True):
    """`FusedAdamW` from the reference's `optimizer` / `optimizer_config` dicts as they stand (type='AdamW' only)."""
    cfg = dict(optimizer)
    typ = cfg.pop("type", None)
    if typ != "AdamW":
        raise NotImplementedError(f"build_optimizer: optimizer type={typ!r} is not built (type='AdamW' is)")
    hook = dict(optimizer_config or {})
    hook_type = hook.pop("type", "OptimizerHook")
    if hook_type != "OptimizerHook":
        raise NotImplementedError(f"build_optimizer: optimizer_config type={hook_type!r} is not built")
    grad_clip = hook.pop("grad_clip", None)
    for key in hook:
        raise NotImplementedError(f"build_optimizer: optimizer_config option '{key}' is not built")
    return FusedAdamW(dp, grad_clip=grad_clip, fused=fused, **cfg)
