"""ctypes loader for libfsf_hip.so — the only way the package reaches the GPU kernels.

There is deliberately NO CPU fallback: if the library is missing or a call is made without a HIP device the
product path raises.  (The CPU oracle under `oracle/` is test infrastructure and is never imported here.)
"""
import ctypes
import os
import re
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# FSF_LIB_PATH: another BUILD of the same library (same ABI version, checked below) — same-box A/B of two source states by
# tools/profiling/ab_bench.sh; never set in product runs
LIB_PATH = os.environ.get("FSF_LIB_PATH") or os.path.join(_HERE, "libfsf_hip.so")

_lib = None
_lock = threading.Lock()

c_i32 = ctypes.c_int32
c_i64 = ctypes.c_int64
c_f32 = ctypes.c_float
c_p = ctypes.c_void_p


class FsfHipError(RuntimeError):
    pass


HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fsf_hip.h")

_ARG_TYPES = {"int": c_i32, "int32_t": c_i32, "int64_t": c_i64, "float": c_f32}
_RES_TYPES = {"int": c_i32, "int32_t": c_i32, "int64_t": c_i64, "const char*": ctypes.c_char_p}


def parse_header(text):
    """(signatures, defines) of a C header: {name: (argtypes, restype)} for every `fsf_*` function it declares and {name: value}
    for every integer `#define FSF_*`.  A parameter written with `*` or `[N]` binds as c_void_p; a by-value type other than int /
    int32_t / int64_t / float, or a return type other than those integers and const char*, raises FsfHipError: nothing is guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {k: int(v) for k, v in re.findall(r"^\s*#\s*define\s+(FSF_\w+)\s+\(?(-?\d+)\)?\s*$", text, flags=re.M)}
    signatures = {}
    for stmt in re.split(r"[;{}]", re.sub(r"^\s*#.*$", "", text, flags=re.M)):
        m = re.fullmatch(r"(.*?)\b(fsf_\w+)\s*\((.*)\)", " ".join(stmt.split()))
        if m is None:
            continue
        ret, name, params = re.sub(r" ?\* ?", "*", m.group(1).strip()), m.group(2), m.group(3).strip()
        if ret not in _RES_TYPES:
            raise FsfHipError(f"{name}: no ctypes binding for the return type '{ret}'")
        argtypes = []
        for p in params.split(",") if params not in ("", "void") else []:
            if "*" in p or "[" in p:
                argtypes.append(c_p)
                continue
            typ = p.strip().rsplit(" ", 1)[0]  # (the parameter's name dropped)
            if typ not in _ARG_TYPES:
                raise FsfHipError(f"{name}: no ctypes binding for the parameter type '{typ}'")
            argtypes.append(_ARG_TYPES[typ])
        signatures[name] = (argtypes, _RES_TYPES[ret])
    return signatures, defines


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise FsfHipError(f"{HEADER_PATH} cannot be read ({e.strerror}): the library's C ABI (signatures, ABI version, constants) "
                          "is taken from it") from e


# every signature and integer constant of include/fsf_hip.h: the header is the one description of the C ABI
SIGNATURES, DEFINES = _read_header()


def lib():
    """Load (once) and return the ctypes handle, every function the header declares bound to its declared signature.  Fails loudly
    when the extension has not been built or was built against another ABI version."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise FsfHipError(
                        f"{LIB_PATH} is missing: the HIP extension was not built. "
                        "Run `python -m fullysparsefusion_amd.build` (needs hipcc); there is no CPU fallback."
                    )
                h = ctypes.CDLL(LIB_PATH)
                want = DEFINES["FSF_ABI_VERSION"]
                if int(h.fsf_abi_version()) != want:
                    raise FsfHipError(f"{LIB_PATH} has ABI version {int(h.fsf_abi_version())}, include/fsf_hip.h declares {want}: "
                                      "stale build, run `python -m fullysparsefusion_amd.build`")
                for name, (argtypes, restype) in SIGNATURES.items():
                    fn = getattr(h, name)
                    fn.argtypes, fn.restype = argtypes, restype
                _lib = h
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().fsf_status_string(int(status)).decode()
        err = FsfHipError(f"{what} failed: {msg} (status {status})")
        err.status = int(status)
        raise err


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise FsfHipError(
                "fullysparsefusion_amd ops run on the HIP device only (got a CPU tensor); there is no CPU fallback"
            )


def ptr(t):
    """Device pointer of a contiguous tensor (None -> NULL)."""
    if t is None:
        return c_p(None)
    if not t.is_contiguous():
        raise FsfHipError("non-contiguous tensor passed to the C ABI")
    return c_p(t.data_ptr())


def _raw_stream(device_index=None):
    """hipStream_t of torch's current stream as an int.  `torch.cuda.current_stream()` builds a Stream object (~8 us, and
    the wrappers need it ~300 times per frame); the raw getter is the same value without the object."""
    if device_index is None:
        device_index = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(device_index)


def stream_ptr():
    return c_p(_raw_stream())


_ws_cache = {}


def workspace(nbytes, device):
    """Grow-only scratch buffer per (device, stream).  Stream-ordered reuse is safe because every C-ABI
    call enqueues all of its work on the current stream before returning."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (index, _raw_stream(index))
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def f32_array(vals):
    return (c_f32 * len(vals))(*[float(v) for v in vals])


def i32_array(vals):
    return (c_i32 * len(vals))(*[int(v) for v in vals])


def i64_array(vals):
    return (c_i64 * len(vals))(*[int(v) for v in vals])
