"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/fsf_hip.h declares; the ctypes signatures,
constants and descriptor structs the package uses are the header's.  No compute calls (there is no GPU in the build container)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fsf_hip.h")
P, I32, I64, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float


def declared_symbols():
    from fullysparsefusion_amd import _lib

    return sorted(_lib.SIGNATURES)


def test_header_declares_the_hot_path():
    syms = declared_symbols()
    for must in ["fsf_voxelize_dynamic", "fsf_voxelize_divfloor", "fsf_unique_rows", "fsf_segment_reduce",
                 "fsf_segment_reduce_backward", "fsf_gather_rows", "fsf_voxel2point", "fsf_project_gather_mask",
                 "fsf_cam_select_score", "fsf_rulebook_subm", "fsf_rulebook_strided", "fsf_rulebook_to_pairs",
                 "fsf_spconv_forward", "fsf_connected_components", "fsf_ingroup_rank"]:
        assert must in syms


def test_library_builds_and_exports_every_declared_symbol():
    from fullysparsefusion_amd import _lib, build

    lib_path = build.build()
    assert os.path.exists(lib_path)
    lib = ctypes.CDLL(lib_path)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, f"declared in include/fsf_hip.h but not exported: {missing}"
    lib.fsf_status_string.restype = ctypes.c_char_p
    assert lib.fsf_status_string(0) == b"ok"
    header = _lib.DEFINES["FSF_ABI_VERSION"]
    assert lib.fsf_abi_version() == header  # (the loader in fullysparsefusion_amd/_lib.py refuses a library of another version)


def test_every_declared_function_is_bound_to_its_header_signature():
    from fullysparsefusion_amd import _lib, build, hip_ops

    build.build()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fsf_[a-z0-9_]+)\s*\(", text))) == declared_symbols()  # (the reader skips no declaration)
    h = _lib.lib()
    assert hip_ops._L() is h
    for name, (argtypes, restype) in _lib.SIGNATURES.items():
        fn = getattr(h, name)
        assert list(fn.argtypes) == argtypes and fn.restype is restype, name


def test_signature_rules_on_pinned_declarations():
    from fullysparsefusion_amd._lib import SIGNATURES

    # arrays (`const float voxel_size[3]`) and `void* stream` are pointers
    assert SIGNATURES["fsf_voxelize_dynamic"] == ([P, I64, I32, I32, P, P, P, P, P, P], I32)
    # `const FsfSirBlock*`, `const float* const*`
    assert SIGNATURES["fsf_sir_stack_forward"] == ([P, I32, P, I64, I32, P, P, P, I32, P, I32, P, I64, I32, F32, P, I64, I32, P, I64, I64, P,
                                                    I64, P, P, I64, P], I32)
    assert SIGNATURES["fsf_weighted_xyz"] == ([P, I64, P, I64, F32, P, P], I32)
    assert SIGNATURES["fsf_lidar_cluster_frontend_arena_bytes"] == ([I64, I32, I32], I64)
    assert SIGNATURES["fsf_augment_max"] == ([], I32)
    assert SIGNATURES["fsf_status_string"] == ([I32], ctypes.c_char_p)


SMALL_HEADER = """
#ifndef FSF_SMALL_H_
#define FSF_SMALL_H_
#define FSF_ONE 1
#define FSF_ERR_SMALL (-7)   /* negative */
/* int fsf_commented_out(double x); */
extern "C" {
int64_t fsf_size(int64_t n,
                 int32_t k);  // a declaration over two lines
"""


def test_reader_on_a_small_header():
    from fullysparsefusion_amd._lib import parse_header

    assert parse_header(SMALL_HEADER) == ({"fsf_size": ([I64, I32], I64)}, {"FSF_ONE": 1, "FSF_ERR_SMALL": -7})


@pytest.mark.parametrize("decl, typ", [("int fsf_bad(uint32_t flags);", "uint32_t"), ("int fsf_bad(int64_t n, double x);", "double"),
                                       ("int fsf_bad(FsfSirBlock block);", "FsfSirBlock"), ("double fsf_bad(void);", "double"),
                                       ("void fsf_bad(int32_t n);", "void")])
def test_reader_refuses_a_type_it_cannot_bind(decl, typ):
    from fullysparsefusion_amd._lib import FsfHipError, parse_header

    with pytest.raises(FsfHipError, match=f"fsf_bad: .*'{typ}'"):
        parse_header(SMALL_HEADER + decl)


def test_int64_results_above_2_to_the_31_come_back_whole():
    """An int64_t result bound with ctypes' default int return type loses its upper half: K30's arena size for 10^6 rows, six groups
    (2 337 766 912 bytes then) once read back as -1 957 200 384.  The size is measured from the entry's own layout now: 6 144 bytes
    of slack less than the hand-written sum (docs/kernels/K29_query_glue.md), still whole."""
    from fullysparsefusion_amd import _lib, build, hip_ops

    build.build()
    assert _lib.lib().fsf_lidar_cluster_frontend_arena_bytes(1_000_000, 6, 5) == 2_337_766_912 - 6_144 > 1 << 31
    assert hip_ops._L().fsf_lidar_cluster_frontend_arena_bytes(1_000_000, 6, 5) == 2_337_766_912 - 6_144


def header_structs():
    """{name: [(field, is_pointer, base type, array extent or None)]} of every `typedef struct { ... } name;` of the header."""
    from fullysparsefusion_amd._lib import DEFINES

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *rest = decl.split(",")  # `const float *bias, *gamma, *beta`: one base type, several declarators
            base, first = re.fullmatch(r"(.*?)\s*(\**\s*\w+(?:\[\w+\])?)", first.strip()).groups()
            for d in [first] + rest:
                star, field, ext = re.fullmatch(r"\s*(\*?)\s*(\w+)(?:\[(\w+)\])?\s*", d).groups()
                fields.append((field, star == "*", base, int(DEFINES.get(ext, ext)) if ext else None))
        structs[name] = fields
    return structs


def test_sir_descriptor_structs_match_the_header():
    from fullysparsefusion_amd import hip_ops

    structs = header_structs()
    scalar = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "FsfSirLayer": hip_ops._SirLayerC}
    for cls, name in ((hip_ops._SirLayerC, "FsfSirLayer"), (hip_ops._SirBlockC, "FsfSirBlock")):
        want = [(f, P if ptr else scalar[base], ext) for f, ptr, base, ext in structs[name]]
        got = [(f, t._type_, t._length_) if issubclass(t, ctypes.Array) else (f, t, None) for f, t in cls._fields_]
        assert got == want, name


def test_product_path_fails_loudly_without_a_gpu():
    import torch

    from fullysparsefusion_amd import hip_ops
    from fullysparsefusion_amd._lib import FsfHipError

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(FsfHipError):
        hip_ops.unique_rows(torch.zeros((4, 4), dtype=torch.int64))
    with pytest.raises(FsfHipError):
        hip_ops.voxelize_dynamic(torch.zeros((4, 5)), (0.2, 0.2, 0.2), [-51.2, -51.2, -5, 51.2, 51.2, 3], [512, 512, 40])


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "fullysparsefusion_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(dirpath, f)


def test_prepared_linear_weights_carry_their_format_as_a_tag_not_as_a_size():
    """ADVICE r5 / VERDICT r5 next-7: hip_ops.linear_norm_act picks the entry point (bf16 x 6 or K22f's f16 x 3) from the tag the
    preparing call attached; nothing in the package infers it from the buffer's size any more, and an untagged buffer is refused."""
    import torch

    from fullysparsefusion_amd import hip_ops

    src = open(os.path.join(ROOT, "fullysparsefusion_amd", "hip_ops.py")).read()
    assert "& 1023" not in src
    with pytest.raises(hip_ops.FsfHipError, match="format tag"):
        hip_ops.linear_weight_is_f16(torch.zeros(1280, dtype=torch.uint8))
    t = torch.zeros(1280, dtype=torch.uint8)
    setattr(t, hip_ops._FMT_ATTR, "f16x3")
    assert hip_ops.linear_weight_is_f16(t)
    csrc = open(os.path.join(ROOT, "fullysparsefusion_amd", "csrc", "linear_norm_act.hip")).read()
    assert "LNA_F16_TAG" in csrc and "__builtin_trap()" in csrc  # the f16 kernels verify the header's tag word


def test_every_entry_point_of_the_header_is_named_in_integration_md():
    """INTEGRATION.md shows the reference-side binding of every entry point (size functions are covered by one line)."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    missing = [s for s in declared_symbols() if not s.endswith("_bytes") and s not in doc]
    assert missing == [], missing
