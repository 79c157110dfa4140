"""The C ABI, stated once in include/lead_yolo_hip.h, against the ctypes binding lead-yolo_amd/capi.py generates from it: struct layouts
and constants through the host C compiler (not through capi's own reading of the header), the prototypes by name and count, the
exported symbols through the built library.  No GPU; only the export test needs the .so."""
import ctypes
import functools
import keyword
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from lead_yolo_amd import capi

HDR = re.sub(r"/\*.*?\*/", " ", open(capi.HEADER_PATH).read(), flags=re.S)
STRUCTS = {name: re.findall(r"(\w+)\s*(?:\[\w+\])?\s*[;,]", body) for name, body in re.findall(r"typedef struct (\w+) \{(.*?)\} \1;", HDR, re.S)}
CONSTANTS = {n: ("LY_" + n + "_" * n.startswith("ACT_")).replace("LY_LY_", "LY_") for n in vars(capi)
             if re.match(r"LY_(F\d+|BF\d+)$|ACT_|GATHER_|PRO_|STATS_STRIPES$|F64_ADD_MAX$|SCALE_IMG_MAX$", n)}


def _cc():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (shutil.which("cc"), os.path.join(rocm, "llvm", "bin", "clang"), os.path.join(rocm, "lib", "llvm", "bin", "clang"))
             if c and os.path.exists(c)]
    assert found, "no host C compiler: neither cc nor the clang of the ROCm install"
    return found[0]


@functools.lru_cache(None)
def compiled():
    """{struct: sizeof, (struct, field): (offsetof, sizeof), constant: value} as the C compiler reads the header"""
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "lead_yolo_hip.h"', 'int main(void) {']
    for s, fields in STRUCTS.items():
        src.append(f'  printf("S {s} %zu\\n", sizeof({s}));')
        src += [f'  printf("F {s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));' for f in fields]
    src += [f'  printf("C {c} %lld\\n", (long long)({c}));' for c in CONSTANTS.values()]
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "abi.c"), "w") as f:
            f.write("\n".join(src + ["  return 0;", "}", ""]))
        subprocess.run([_cc(), "-std=c99", "-I", os.path.dirname(capi.HEADER_PATH), "-o", os.path.join(d, "abi"), os.path.join(d, "abi.c")],
                       check=True, capture_output=True, text=True)
        rows = subprocess.run([os.path.join(d, "abi")], check=True, capture_output=True, text=True).stdout.splitlines()
    return {(r[1], r[2]) if r[0] == "F" else r[1]: (int(r[3]), int(r[4])) if r[0] == "F" else int(r[2]) for r in map(str.split, rows)}


def test_struct_layouts_match_the_c_compiler():
    cc = compiled()
    bound = {n for n, v in vars(capi).items() if isinstance(v, type) and issubclass(v, ctypes.Structure)}
    assert bound == set(STRUCTS) and len(STRUCTS) >= 13
    nfields = 0
    for s, fields in STRUCTS.items():
        cls = getattr(capi, s)
        assert [n for n, _ in cls._fields_] == [f + "_" * keyword.iskeyword(f) for f in fields], s
        assert ctypes.sizeof(cls) == cc[s], s
        for (n, _), f in zip(cls._fields_, fields):
            assert (getattr(cls, n).offset, getattr(cls, n).size) == cc[(s, f)], (s, f)
            nfields += 1
    assert nfields >= 237
    assert ctypes.sizeof(capi.LyMosaicTile) == 72 and ctypes.sizeof(capi.LyMosaicImage) == 392      # static_assert in ly_mosaic.hip


def test_struct_fields_the_callers_rely_on():
    assert capi.LyRf1BwdParams.lambda_.size == ctypes.sizeof(ctypes.c_void_p)                        # `lambda` in the header
    spec = capi.LyScaleImgSpec(None, 1, 2, 3, 4, 1)                                                  # positional, as ops.scale_img builds it
    assert (spec.out, spec.Hs, spec.Ws, spec.Ho, spec.Wo, spec.flip) == (None, 1, 2, 3, 4, 1)
    img = capi.LyMosaicImage(mosaic=1)
    assert len(img.tile) == 4 and isinstance(img.tile[3], capi.LyMosaicTile) and len(img.m) == 6 and len(img.minv) == 6 and img.mosaic == 1
    t = capi.LyF64AddTable()
    assert len(t.src) == len(t.dst) == len(t.n) == capi.F64_ADD_MAX == 64
    assert capi.LyAdamTensor._fields_[-1][0] == "step0" and capi.LyOptTensor._fields_[2][0] == "buf"
    assert (capi.STATS_STRIPES, capi.SCALE_IMG_MAX) == (32, 4)


def test_constants_match_the_header():
    cc = compiled()
    assert {"LY_F32", "LY_BF16", "LY_F16", "ACT_SILU", "GATHER_PATCH_NCHW_F16", "PRO_AFFINE_RELU_CA", "STATS_STRIPES"} <= set(CONSTANTS)
    for py, c in CONSTANTS.items():
        assert getattr(capi, py) == cc[c], (py, c)


def test_signatures_one_per_prototype():
    declared = set(re.findall(r"\b(ly_[a-z0-9_]+)\s*\(", HDR))
    assert set(capi.SIGNATURES) == set(capi.RESTYPES) == declared
    assert len(capi.SIGNATURES) == len(re.findall(r"\)\s*;", HDR)) >= 90                              # only prototypes end in `);`
    for name in ("ly_mlpblock_fwd", "ly_gemm_fwd", "ly_conv3x3_fwd", "ly_rfcbam3_fwd", "ly_adam_step", "ly_scale_img", "ly_detect_level_aug",
                 "ly_detect_tail_aug", "ly_mosaic_img", "ly_mosaic_labels"):
        assert name in capi.SIGNATURES
    scalars = {ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double, ctypes.c_ulonglong, ctypes.c_void_p}
    for name, args in capi.SIGNATURES.items():
        assert set(args) <= scalars, name                                                            # every pointer is a c_void_p
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, HDR).group(1)
        assert len(args) == (0 if params.strip() == "void" else params.count(",") + 1), name
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    assert capi.SIGNATURES["ly_abi_version"] == [] and capi.RESTYPES["ly_abi_version"] is I
    assert capi.SIGNATURES["ly_last_error"] == [] and capi.RESTYPES["ly_last_error"] is ctypes.c_char_p
    assert capi.SIGNATURES["ly_mlpblock_bwd_slab_floats"] == [I] and capi.RESTYPES["ly_mlpblock_bwd_slab_floats"] is L
    assert capi.SIGNATURES["ly_gemm_fwd"] == [P, P] and capi.SIGNATURES["ly_event_create"] == [P]
    assert capi.SIGNATURES["ly_sum_rows"] == [P, L, L, L, P, I, P]
    assert capi.SIGNATURES["ly_nms_candidates"] == [P, I, I, I, F, ctypes.c_ulonglong, P, P, P]
    assert capi.SIGNATURES["ly_bn_bwd_coeffs"][:5] == [P, I, I, I, ctypes.c_double]
    assert sum(r is I for r in capi.RESTYPES.values()) == len(capi.RESTYPES) - 2


@pytest.mark.parametrize("line, edit, msg", [
    ("int ly_mlpblock_hidden_tiles(int C);", "int ly_mlpblock_hidden_tiles(size_t C);", "unknown type 'size_t'"),
    ("const float* x_scale; const float* x_shift;", "const float* x_scale, x_shift;", "cannot split"),
    ("#define LY_SCALE_IMG_MAX 4", "#define LY_SCALE_IMG_MAX (2 + 2)", "cannot evaluate"),
    ("int ly_mlpblock_hidden_tiles(int C);", "static inline int twice(int c) { return 2 * c; }", "not a declaration"),
])
def test_parser_refuses_what_it_does_not_know(tmp_path, line, edit, msg):
    text = open(capi.HEADER_PATH).read()
    assert text.count(line) == 1
    (tmp_path / "bad.h").write_text(text.replace(line, edit))
    with pytest.raises(capi.HipLibraryError, match=re.escape(msg)) as e:
        capi._parse_header(str(tmp_path / "bad.h"))
    assert f"bad.h:{text[:text.index(line)].count(chr(10)) + 1}:" in str(e.value)                   # the error names the header line
    with pytest.raises(capi.HipLibraryError, match="missing.h"):
        capi._parse_header(str(tmp_path / "missing.h"))


def test_capi_exports_every_declared_symbol():
    """The shared library loads and exports every function include/lead_yolo_hip.h declares."""
    declared = set(re.findall(r"\b(ly_[a-z0-9_]+)\s*\(", open(capi.HEADER_PATH).read()))
    assert {"ly_mlpblock_fwd", "ly_gemm_fwd", "ly_conv3x3_fwd", "ly_rfcbam3_fwd"} <= declared
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    assert set(capi.SIGNATURES) >= declared
    assert capi.lib().ly_abi_version() == 5
