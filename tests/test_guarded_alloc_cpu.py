"""tests/guarded.py on the CPU (no GPU): layout, alignment, poison, pass-through, restoration, the two one-byte overruns — and the
static condition that every allocating wrapper of hip_ops.py has a case in tests/test_guard_bands_gpu.py."""
import ast
import os
import re

import pytest
import torch

from fullysparsefusion_amd import _lib
from guarded import ALIGN, GUARD_BYTE, guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_views_are_aligned_shaped_typed_and_poisoned(fill):
    real = torch.empty
    with guarded(fill, device_type="cpu", guard_bytes=4096) as g:
        a = torch.empty((7, 3), dtype=torch.float32)  # tuple size, default device
        b = torch.empty(5, 2, dtype=torch.int64, device="cpu")  # positional sizes
        c = torch.empty((0, 4), dtype=torch.int32, device=torch.device("cpu"))  # zero elements
        d = torch.empty((), dtype=torch.float32, device="cpu")  # zero dimensions
        e = torch.empty(131, dtype=torch.uint8, device="cpu")  # one int
        f = torch.empty((3,), dtype=torch.bool, device="cpu")
        h = torch.empty(size=(2, 2), dtype=torch.float64, device="cpu")
        i = torch.empty([3, 1], device="cpu")  # list size, default dtype
        for t, shape, dtype in ((a, (7, 3), torch.float32), (b, (5, 2), torch.int64), (c, (0, 4), torch.int32), (d, (), torch.float32),
                                (e, (131,), torch.uint8), (f, (3,), torch.bool), (h, (2, 2), torch.float64), (i, (3, 1), torch.float32)):
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.data_ptr() % ALIGN == 0
        assert g.counts == {"empty": 8, "workspace": 0}
        assert [r["nbytes"] for r in g.records] == [84, 80, 0, 4, 131, 3, 32, 12]  # exact byte counts, no rounding
        assert [r["site"] for r in g.records] == ["test_views_are_aligned_shaped_typed_and_poisoned"] * 8
        if fill == 0xFF:
            assert bool(torch.isnan(a).all()) and bool((b == -1).all()) and bool(torch.isnan(d))
        else:
            assert bool((a == 0).all()) and bool((b == 0).all()) and float(d) == 0.0
        for k in range(8):
            assert bool((g.payload_of(k) == fill).all())  # a payload left untouched is still all poison
        for r in g.records:  # the guards on both sides are whole and at least guard_bytes wide
            base, off, nb = r["base"], r["off"], r["nbytes"]
            assert off >= 4096 and base.numel() - off - nb >= 4096
            assert bool((base[:off] == GUARD_BYTE).all()) and bool((base[off + nb:] == GUARD_BYTE).all())
        assert g.violations() == []
        # not ours: out=, pinned requests and other devices go to the real torch.empty
        o = real(4)
        assert torch.empty(4, out=o) is o and g.counts["empty"] == 8
        m = torch.empty((3,), device="meta")
        assert m.device.type == "meta" and g.counts["empty"] == 8
    assert torch.empty is real


def test_other_device_type_passes_through():
    with guarded(0xFF, device_type="cuda") as g:
        t = torch.empty((4, 4), dtype=torch.float32)
        u = torch.empty(3, device="cpu")
        assert g.counts == {"empty": 0, "workspace": 0} and t.shape == (4, 4) and u.shape == (3,)
        assert g.violations() == []


def test_workspace_is_exact_poisoned_and_never_reused():
    dev = torch.device("cpu")
    with guarded(0xFF, device_type="cpu", guard_bytes=1024) as g:
        w1 = _lib.workspace(3072, dev)
        w2 = _lib.workspace(100, dev)
        w0 = _lib.workspace(0, dev)  # floor of one byte so that ptr() stays valid
        assert (w1.numel(), w2.numel(), w0.numel()) == (3072, 100, 1)
        assert w1.dtype == torch.uint8 and w1.data_ptr() % ALIGN == 0 and w2.data_ptr() % ALIGN == 0 and w0.data_ptr() % ALIGN == 0
        assert w1.data_ptr() != w2.data_ptr() and bool((w1 == 0xFF).all())
        assert g.counts == {"empty": 0, "workspace": 3} and g.workspace_sizes == [3072, 100, 0]
        assert g.violations() == []


def test_both_replacements_are_restored_after_an_exception():
    real_empty, real_ws = torch.empty, _lib.workspace
    with pytest.raises(ZeroDivisionError):
        with guarded(0x00, device_type="cpu"):
            assert torch.empty is not real_empty and _lib.workspace is not real_ws
            1 / 0
    assert torch.empty is real_empty and _lib.workspace is real_ws


def _kernel_one_past_the_end(n):
    out = torch.empty((n,), dtype=torch.float32, device="cpu")
    torch.as_strided(out.view(torch.uint8), (n * 4 + 1,), (1,)).fill_(7)  # n * 4 bytes of output and one more
    return out


def _kernel_one_before_the_start(dev):
    ws = _lib.workspace(640, dev)
    raw = torch.as_strided(ws, (641,), (1,), storage_offset=ws.storage_offset() - 1)
    raw[0] = 9
    return ws


def test_one_byte_overruns_are_reported_with_record_and_offset():
    with guarded(0xFF, device_type="cpu", guard_bytes=512) as g:
        clean = torch.empty((10,), dtype=torch.int32, device="cpu")
        _kernel_one_past_the_end(33)
        _kernel_one_before_the_start(torch.device("cpu"))
        v = g.violations()
        assert len(v) == 2
        assert (v[0]["kind"], v[0]["site"], v[0]["side"], v[0]["offset"], v[0]["nbytes"], v[0]["damaged"]) == \
            ("empty", "_kernel_one_past_the_end", "back", 0, 132, 1)
        assert (v[1]["kind"], v[1]["site"], v[1]["side"], v[1]["offset"], v[1]["nbytes"], v[1]["damaged"]) == \
            ("workspace", "_kernel_one_before_the_start", "front", -1, 640, 1)
        assert bool((clean == -1).all())


def test_a_write_further_into_the_guard_reports_its_first_byte():
    with guarded(0x00, device_type="cpu", guard_bytes=512) as g:
        t = torch.empty((4, 4), dtype=torch.float32, device="cpu")
        raw = torch.as_strided(t.view(torch.uint8).view(-1), (64 + 300,), (1,))
        raw[64 + 256:64 + 260] = 1  # one float 256 bytes past the end
        (v,) = g.violations()
        assert (v["side"], v["offset"], v["damaged"], v["nbytes"]) == ("back", 256, 4, 64)


# ------------------------------------------------------------------------------------------------ coverage of hip_ops.py
# `_prepare_weight` is the shared body of the three spconv_prepare_weight_* wrappers, no wrapper itself: each of them allocates by
# calling it (and counts here for that), and their guard-band cases run it
_SHARED_BODIES = {"_prepare_weight"}
_ALLOCATES = re.compile(r"torch\.empty|empty_like|torch\.zeros|torch\.full|_lib\.workspace\(|_workspace_bytes|_arena_bytes|_prepare_weight\(")
_SCRATCH = re.compile(r"_lib\.workspace\(|_workspace_bytes|_arena_bytes")


def allocating_wrappers():
    """({name}, {name}) of hip_ops.py's top-level functions whose body allocates on the device or requests scratch, and of those
    that use scratch."""
    with open(os.path.join(ROOT, "fullysparsefusion_amd", "hip_ops.py")) as f:
        src = f.read()
    alloc, scratch = set(), set()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and node.name not in _SHARED_BODIES:
            body = ast.get_source_segment(src, node)
            if _ALLOCATES.search(body):
                alloc.add(node.name)
                if _SCRATCH.search(body):
                    scratch.add(node.name)
    return alloc, scratch


def test_every_allocating_wrapper_has_a_guard_band_case():
    import test_guard_bands_gpu as gb

    alloc, scratch = allocating_wrappers()
    assert len(alloc) >= 88 and len(scratch) >= 36
    covered = set(gb.CASES) | set(gb.EXEMPT)
    assert sorted(alloc - covered) == [], "wrappers of hip_ops.py without a case in tests/test_guard_bands_gpu.py (or a reason in EXEMPT)"
    assert sorted(scratch - set(gb.CASES)) == [], "every wrapper that uses scratch needs a case: EXEMPT is not open to them"
    assert all(isinstance(r, str) and r.strip() for r in gb.EXEMPT.values())
    from fullysparsefusion_amd import hip_ops
    assert all(hasattr(hip_ops, name) for name in covered)
    for name, cases in gb.CASES.items():
        kinds = [k for k, _ in cases]
        assert "ragged" in kinds and "minimal" in kinds, f"{name}: needs a ragged and a minimal input set"
        assert ("empty" in kinds) != (name in gb.NO_EMPTY), f"{name}: needs an empty input set, or the refusing argument check in NO_EMPTY"
    assert set(gb.NO_EMPTY) <= set(gb.CASES) and all(isinstance(r, str) and r.strip() for r in gb.NO_EMPTY.values())
