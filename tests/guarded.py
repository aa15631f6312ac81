"""Guard bands and poison for everything the C-ABI wrappers allocate (a plain helper module, not a conftest).

`guarded(fill)` replaces `torch.empty` (tensors of one device type only) and `fullysparsefusion_amd._lib.workspace` for its
duration.  Every intercepted request becomes a view into a larger uint8 buffer laid out as

    [ front guard 0xA5 ... | payload, filled with byte `fill` | back guard 0xA5 ... ]

with the payload 256-byte aligned and ending exactly at the requested byte count.  A kernel that writes past either end of what it was
given damages a guard, which `violations()` reports; a kernel that leaves part of its output or scratch unwritten, or relies on scratch
being zero, computes from `fill` and differs between the 0xFF and the 0x00 run.  The guards are the test's own live memory: a stray
write up to `guard_bytes` wide is recorded, never a fault.
"""
import contextlib
import sys

import torch

GUARD_BYTE = 0xA5
FILLS = (0xFF, 0x00)
ALIGN = 256


class Guard:
    def __init__(self, fill, device_type, guard_bytes, real_empty):
        assert 0 <= fill <= 0xFF and guard_bytes >= 1
        self.fill, self.device_type, self.guard_bytes = int(fill), device_type, int(guard_bytes)
        self.records = []  # dict(kind, site, nbytes, base, off): every base buffer is kept alive until the Guard goes
        self.counts = {"empty": 0, "workspace": 0}
        self.workspace_sizes = []  # the nbytes of every scratch request, as asked
        self._real_empty = real_empty

    # ------------------------------------------------------------------------------------------ allocation
    def _payload(self, nbytes, device, kind, site):
        nbytes, g = int(nbytes), self.guard_bytes
        base = self._real_empty((g + nbytes + g + ALIGN,), dtype=torch.uint8, device=device)
        off = g + (-(base.data_ptr() + g)) % ALIGN  # (the base is not assumed aligned: CPU bases are 64-byte aligned only)
        base.fill_(GUARD_BYTE)
        payload = base[off:off + nbytes]
        if nbytes:
            payload.fill_(self.fill)
        self.records.append(dict(kind=kind, site=site, nbytes=nbytes, base=base, off=off))
        self.counts[kind] += 1
        return payload

    def empty(self, *args, **kwargs):
        caller = sys._getframe(1).f_code.co_name
        kw = dict(kwargs)
        device = kw.pop("device", None)
        dtype = kw.pop("dtype", None)
        requires_grad = kw.pop("requires_grad", False)
        size = kw.pop("size", None)
        dev = torch.device(device) if device is not None else self._real_empty(0).device
        if kw or dev.type != self.device_type or (size is None) == (len(args) == 0):
            return self._real_empty(*args, **kwargs)  # out=, pin_memory=, layout=, memory_format=, another device: not ours
        if size is None:
            size = args[0] if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)) else args
        shape = tuple(int(s) for s in size)
        dtype = dtype if dtype is not None else torch.get_default_dtype()
        n = 1
        for s in shape:
            n *= s
        itemsize = self._real_empty((), dtype=dtype).element_size()
        t = self._payload(n * itemsize, dev, "empty", caller).view(dtype).view(shape)
        if requires_grad:
            t.requires_grad_(True)
        return t

    def workspace(self, nbytes, device):
        caller = sys._getframe(1).f_code.co_name
        self.workspace_sizes.append(int(nbytes))
        return self._payload(max(int(nbytes), 1), torch.device(device), "workspace", caller)

    # ------------------------------------------------------------------------------------------ checks
    def violations(self):
        """Records whose guards are no longer all 0xA5: dict(kind, site, nbytes, side 'front' | 'back', offset) where offset is the
        first damaged byte relative to the payload's end (back, >= 0) or start (front, < 0).  The per-buffer comparisons are
        accumulated on the device and read back once."""
        if not self.records:
            return []
        if self.device_type == "cuda":
            torch.cuda.synchronize()
        bad = []
        for r in self.records:
            base, off, nb = r["base"], r["off"], r["nbytes"]
            bad.append(torch.count_nonzero(base[:off] != GUARD_BYTE))
            bad.append(torch.count_nonzero(base[off + nb:] != GUARD_BYTE))
        bad = torch.stack(bad).cpu().view(-1, 2)
        out = []
        for r, (front, back) in zip(self.records, bad.tolist()):
            base, off, nb = r["base"], r["off"], r["nbytes"]
            if front:
                first = int((base[:off] != GUARD_BYTE).nonzero()[0])
                out.append(dict(kind=r["kind"], site=r["site"], nbytes=nb, side="front", offset=first - off, damaged=front))
            if back:
                first = int((base[off + nb:] != GUARD_BYTE).nonzero()[0])
                out.append(dict(kind=r["kind"], site=r["site"], nbytes=nb, side="back", offset=first, damaged=back))
        return out

    def payload_of(self, index):
        """The payload bytes (uint8 view) of the index-th intercepted request."""
        r = self.records[index]
        return r["base"][r["off"]:r["off"] + r["nbytes"]]


@contextlib.contextmanager
def guarded(fill, device_type="cuda", guard_bytes=65536):
    from fullysparsefusion_amd import _lib

    real_empty, real_workspace = torch.empty, _lib.workspace
    g = Guard(fill, device_type, guard_bytes, real_empty)
    torch.empty, _lib.workspace = g.empty, g.workspace
    try:
        yield g
    finally:
        torch.empty, _lib.workspace = real_empty, real_workspace
