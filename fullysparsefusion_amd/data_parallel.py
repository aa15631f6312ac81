"""Frame-level data parallelism for training (collective C1): one process per GPU, every rank owns
whole frames, the only exchange per iteration is the gradient all-reduce.

Stands in for what the reference gets from `MMDistributedDataParallel` (tools/train.py -> mmdet3d.apis.train_model,
launched by tools/dist_train.sh:8-9 with one process per GPU).  Differences that matter on MI355X:

  * gradients live in a few large flat fp32 buckets (default 96 MB: xGMI is point-to-point, 7 links x ~153 GB/s, so
    ring steps are per-link bound and small buckets pay the ring latency many times over; ~340 MB of FSF gradients
    become 4 collectives), and `param.grad` are VIEWS into the bucket — no flatten / unflatten copies;
  * a bucket's all-reduce is launched (async, RCCL's own stream) from the autograd hook of its last-arriving
    parameter, so it overlaps the rest of the backward pass; buckets are filled in reverse registration order, which
    is the order gradients become ready;
  * the FSF graph is data dependent (a class group without points skips its layers on one rank only), so parameters
    that received no gradient are treated as zeros and their buckets are reduced in `finish()` — every rank always
    issues the same BUCKET collectives in the same order.  Where in the backward pass a bucket is launched still differs
    between ranks on such a step (mid-backward on one, `finish()` on the other), and `naiveSyncBN1d`'s backward issues
    its own all-reduces in between: RCCL pairs collectives by issue order PER COMMUNICATOR, so the buckets travel on
    their own process group (`dist.new_group`), never on the one the SyncBN statistics use;
  * `backward(loss)` detaches `param.grad` from the views for the duration of the pass: autograd hands each gradient over and a
    bucket adds its parameters' gradients in one multi-tensor kernel when the last one has arrived (264 per-parameter `add_`
    launches per FSF step otherwise, most of them on 128 floats);
  * gradient accumulation: `no_sync()` (as in DDP) keeps micro-batch gradients local; the first backward outside it
    reduces the accumulated sum.  The buckets are cleared by `zero_grad()` — or by the optimizer's own
    `zero_grad()`: with `set_to_none=False` it zeroes the views in place, with `set_to_none=True` (torch's default) it drops
    `param.grad`, and the next forward / backward then zeroes that parameter's slice before re-pointing `param.grad` at it
    (a dropped gradient means "cleared", never "resume from what the bucket last held");
  * `optim.FusedAdamW.step(zero_grads=True)` (K39) steps straight on the buckets and stores 0 to every gradient element it has
    consumed, so a loop that uses it does NOT call `zero_grad()`: `param.grad` stay the bucket views, the next forward's
    `_arm(zero=False)` finds them in place and the next backward adds onto zeros.  It reads `buckets` (`params`, `views`, `flat`) and
    changes nothing else here.
"""
import contextlib

import torch
import torch.distributed as dist


class _Bucket:
    def __init__(self, params, device):
        self.params = params
        self.numel = sum(p.numel() for p in params)
        self.flat = torch.zeros(self.numel, dtype=torch.float32, device=device)
        self.views = []
        off = 0
        for p in params:
            self.views.append(self.flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        self.pending = 0
        self.work = None
        self.launched = False
        self.arrived = []  # (view, gradient autograd handed over) of the running backward pass, added into the bucket in one go


class FrameDataParallel(torch.nn.Module):
    """model wrapper: `forward` delegates; after `loss.backward()` call `finish()` (or use `backward(loss)`) and every
    `param.grad` holds the mean over ranks."""

    def __init__(self, module, bucket_mb=96, process_group=None):
        super().__init__()
        self.module = module
        active = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(process_group) if active else 1
        # a communicator of their own for the gradient buckets (collective call: every rank constructs the wrapper)
        self.group = process_group if process_group is not None or self.world == 1 else dist.new_group()
        self._sync = True
        params = [p for p in module.parameters() if p.requires_grad]
        assert all(p.dtype == torch.float32 for p in params), "gradient buckets are fp32"
        cap = int(bucket_mb * (1 << 20)) // 4
        self.buckets, cur, cur_n = [], [], 0
        for p in reversed(params):  # reverse registration order ~ gradient-ready order
            if cur and cur_n + p.numel() > cap:
                self.buckets.append(_Bucket(cur, p.device))
                cur, cur_n = [], 0
            cur.append(p)
            cur_n += p.numel()
        if cur:
            self.buckets.append(_Bucket(cur, cur[0].device))
        self._where, self._view = {}, {}
        for b in self.buckets:
            for p, v in zip(b.params, b.views):
                p.grad = v  # gradients accumulate straight into the bucket
                self._where[p], self._view[p] = b, v
                p.register_post_accumulate_grad_hook(self._on_grad)
        if self.world > 1:  # same starting point on every rank (what DDP's constructor broadcast does)
            for t in list(module.parameters()) + list(module.buffers()):
                dist.broadcast(t.data, src=0, group=self.group)
        self._armed = False

    def forward(self, *args, **kwargs):
        self._arm(zero=False)
        return self.module(*args, **kwargs)

    @contextlib.contextmanager
    def no_sync(self):
        """Gradient accumulation: backward passes inside this context add into the buckets without any collective."""
        old, self._sync = self._sync, False
        try:
            yield
        finally:
            self._sync = old

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(self.module, name)

    # ------------------------------------------------------------------------------------------------
    def _arm(self, zero=True):
        """Start of a backward pass: re-point grads at the buckets, reset the ready counters; `zero` (zero_grad only)
        also clears the accumulated gradients."""
        for b in self.buckets:
            if b.work is not None:
                raise RuntimeError("FrameDataParallel: the previous backward was not completed with finish()")
            if zero:
                b.flat.zero_()
            b.pending = len(b.params)
            b.work, b.launched = None, False
            b.arrived = []  # (a backward pass that raised may have left hand-overs behind: they belong to no step)
            if not zero:
                dropped = [v for p, v in zip(b.params, b.views) if p.grad is None]
                if len(dropped) == len(b.params):
                    b.flat.zero_()  # optimizer.zero_grad(set_to_none=True) on the whole bucket: one fill
                else:
                    for v in dropped:
                        v.zero_()
            for p, v in zip(b.params, b.views):
                if p.grad is None:
                    p.grad = v
                elif p.grad.data_ptr() != v.data_ptr():
                    # a gradient tensor that is not the bucket view (the caller's, or autograd's after a backward that ran
                    # un-armed): its values carry over into the bucket — except under zero_grad(), which clears them
                    if not zero:
                        v.copy_(p.grad)
                    p.grad = v
        self._armed = True

    def zero_grad(self, set_to_none=False):
        self._arm(zero=True)

    def _launch(self, b):
        b.launched = True
        if self.world > 1 and self._sync:
            b.work = dist.all_reduce(b.flat, op=dist.ReduceOp.SUM, group=self.group, async_op=True)

    def _flush(self, b):
        """The gradients autograd handed over for this bucket's parameters -> the bucket, as ONE multi-tensor add (the views hold
        zeros or what earlier backward passes of an accumulation window left), and `param.grad` back onto the views."""
        if b.arrived:
            torch._foreach_add_([v for v, _ in b.arrived], [g for _, g in b.arrived])
            b.arrived = []
        for p, v in zip(b.params, b.views):
            p.grad = v

    def _on_grad(self, p):
        if not self._armed:
            return
        b, view = self._where[p], self._view[p]
        if p.grad.data_ptr() != view.data_ptr():  # autograd's own tensor (`backward()` detached the view: no per-parameter add)
            b.arrived.append((view, p.grad))
        b.pending -= 1
        # launch in bucket order only: every rank must issue the same sequence of collectives
        if b.pending == 0:
            self._flush(b)
            for nb in self.buckets:
                if nb.launched:
                    continue
                if nb.pending == 0:
                    self._launch(nb)
                else:
                    break

    def finish(self):
        """After backward: reduce the buckets whose parameters did not all receive gradients (zeros stand in), wait for
        every collective and turn sums into means."""
        for b in self.buckets:
            if not b.launched:
                self._flush(b)
                self._launch(b)
        for b in self.buckets:
            if b.work is not None:
                b.work.wait()
                b.work = None
            if self.world > 1 and self._sync:
                b.flat.div_(self.world)
        self._armed = False

    def backward(self, loss):
        """`loss.backward()` + `finish()`.  For the duration of the pass `param.grad` is detached from the bucket views (None), so
        autograd HANDS OVER each parameter's gradient instead of adding it into the view with a kernel of its own — FSF has 264
        parameters per step, most of them 128 floats — and a bucket takes its parameters' gradients in ONE multi-tensor add when the
        last of them has arrived (`_flush`), right before its all-reduce is launched.  The sums are the same additions in the same
        order (view + gradient).  A caller that runs `loss.backward()` itself and then `finish()` gets the in-place path."""
        if not self._armed:
            self._arm(zero=False)
        for b in self.buckets:
            for p, v in zip(b.params, b.views):
                if p.grad is not None and p.grad.data_ptr() == v.data_ptr():
                    p.grad = None
        try:
            loss.backward()
        except BaseException:
            self._abort()
            raise
        self.finish()

    def _abort(self):
        """A backward pass that raised mid-way (a skip-on-OOM loop catches it and goes on): drop the gradients autograd had handed
        over, wait for bucket collectives already in flight (their ranks' peers issued them too), re-point every `param.grad` at its
        view and disarm.  The buckets then hold a partial sum of the failed step; the caller's `zero_grad()` (either style) clears
        it as after any step, and nothing of the failed pass reaches the next one."""
        for b in self.buckets:
            b.arrived = []
            if b.work is not None:
                b.work.wait()
                b.work = None
            b.launched = False
            for p, v in zip(b.params, b.views):
                p.grad = v
        self._armed = False
