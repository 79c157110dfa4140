"""ctypes binding of the C-ABI in include/lead_yolo_hip.h (libleadyolo_hip.so, built in-tree from
lead-yolo_amd/csrc).  The header is the only statement of the ABI: the parameter structs, every entry
point's argument and return types and the size constants below are read from it at import.
There is NO fallback: if the shared library is missing or a call fails the
product raises — the oracle / CPU code is never substituted."""
import ctypes
import keyword
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libleadyolo_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lead_yolo_hip.h")

_lib = None

_P = ctypes.c_void_p
_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
            "unsigned long long": ctypes.c_ulonglong}
_POINTEES = {"void", "char", "unsigned char"}            # what a pointer may point to, besides the scalars and the structs


class HipLibraryError(RuntimeError):
    pass


# the forms of declaration the header uses; anything else is refused (comments are blanked out first)
_ITEM = re.compile(r"""\s*(?:
      \#define[ \t]+(?P<define>\w+)(?P<value>[^\n]*)
    | \#(?:ifndef|ifdef|endif)[^\n]* | extern\s+"C"\s*\{ | \}
    | enum\s*\{(?P<enum>[^{}]*)\}\s*;
    | typedef\s+struct\s+(?P<struct>\w+)\s*\{(?P<body>[^{}]*)\}\s*(?P=struct)\s*;
    | (?P<ret>[\w\s*]+?)\b(?P<fn>ly_[a-z0-9_]+)\s*\((?P<args>[^()]*)\)\s*;
    )""", re.X)
_DECL = re.compile(r"(.*?[\s*])(\w+(?:\[\w+\])?(?:\s*,\s*\w+(?:\[\w+\])?)*)$", re.S)     # type, declarators


def _parse_header(path):
    """(defines, structs, argtypes, restypes) of the header.  Every pointer is a c_void_p, whatever it points to: several struct-pointer
    parameters take device addresses.  Strict: a construct this does not know raises HipLibraryError with the header line."""
    try:
        with open(path) as f:
            text = re.sub(r"/\*.*?\*/", lambda c: re.sub(r"[^\n]", " ", c.group()), f.read(), flags=re.S)    # lines stay where they are
    except OSError as e:
        raise HipLibraryError(f"{path}: {e.strerror}: the ctypes binding is generated from this header") from None
    defines, structs, argtypes, restypes = {}, {}, {}, {}

    def fail(pos, why):
        pos += len(text[pos:]) - len(text[pos:].lstrip())
        raise HipLibraryError(f"{path}:{text.count(chr(10), 0, pos) + 1}: {why}")

    def number(word, pos):
        return int(word) if word.isdigit() else defines[word] if word in defines else fail(pos, f"cannot evaluate '{word}'")

    def ctype(spec, pos):
        base, known = " ".join(spec.replace("*", " ").split()).removeprefix("const "), {**_SCALARS, **structs}
        if "*" in spec and (base in known or base in _POINTEES):
            return _P
        return known[base] if "*" not in spec and base in known else fail(pos, f"unknown type '{spec.strip()}'")

    def decls(src, pos, sep):
        for d in re.finditer(f"[^{sep}]*[^{sep}\\s][^{sep}]*", src):
            m, at = _DECL.match(d.group().strip()), pos + d.start()
            if not m or ("*" in m[1] and "," in m[2]):
                fail(at, f"cannot split the declaration '{d.group().strip()}'")
            for decl in m[2].split(","):
                name, _, dim = decl.strip().rstrip("]").partition("[")
                yield name + "_" * keyword.iskeyword(name), ctype(m[1], at) * number(dim, at) if dim else ctype(m[1], at)

    pos = 0
    while text[pos:].strip():
        m = _ITEM.match(text, pos) or fail(pos, "not a declaration this binding knows")
        pos = m.end()
        if m["define"] and m["value"].strip():
            defines[m["define"]] = number(m["value"].strip(), m.start("value"))
        elif m["enum"] and not all(re.fullmatch(r"\s*\w+\s*=\s*\d+\s*", e) for e in m["enum"].split(",")):
            fail(m.start("enum"), "enumerators must be NAME = number")
        elif m["struct"]:
            fields = list(decls(m["body"], m.start("body"), ";"))
            structs[m["struct"]] = type(m["struct"], (ctypes.Structure,), {"_fields_": fields, "__module__": __name__})
        elif m["fn"]:
            if "[" in m["args"] or not m["args"].strip():
                fail(m.start("args"), f"cannot read the parameter list of {m['fn']}")
            restypes[m["fn"]] = ctypes.c_char_p if "".join(m["ret"].split()) == "constchar*" else ctype(m["ret"], m.start("ret"))
            argtypes[m["fn"]] = [t for _, t in decls(m["args"], m.start("args"), ",")] if m["args"].strip() != "void" else []
    found = set(re.findall(r"\b(ly_[a-z0-9_]+)\s*\(", text))
    if found != set(argtypes):
        raise HipLibraryError(f"{path}: no prototype read for {sorted(found ^ set(argtypes))}")
    return defines, structs, argtypes, restypes


# LyGemmParams, LyConv3Params, ...: one ctypes.Structure per `typedef struct LyX`, fields in header order (`lambda` is spelled `lambda_`;
# ops.py / grad.py / pack.py fill several of them positionally: moving a field in the header means editing those calls);
# SIGNATURES / RESTYPES: name -> argtypes / restype of every ly_* prototype (int: 0 ok, <0 error with ly_last_error())
_DEFINES, _STRUCTS, SIGNATURES, RESTYPES = _parse_header(HEADER_PATH)
globals().update(_STRUCTS)
STATS_STRIPES, F64_ADD_MAX, SCALE_IMG_MAX = _DEFINES["LY_STATS_STRIPES"], _DEFINES["LY_F64_ADD_MAX"], _DEFINES["LY_SCALE_IMG_MAX"]
ANCHOR_NA_MAX, ANCHOR_SLICES_MAX = _DEFINES["LY_ANCHOR_NA_MAX"], _DEFINES["LY_ANCHOR_SLICES_MAX"]

# the semantic constants keep their Python spelling (tests/test_capi_abi.py holds them to the header's enums)
LY_F32, LY_BF16 = 0, 1                     # `dtype` codes of the C ABI
LY_F16 = 2                                 # fp16 storage: ly_scale_img only


def dtype_code(t):
    """LY_F32 / LY_BF16 for a tensor (or torch dtype)"""
    import torch
    d = t if isinstance(t, torch.dtype) else t.dtype
    if d == torch.float32:
        return LY_F32
    if d == torch.bfloat16:
        return LY_BF16
    raise HipLibraryError(f"the HIP kernels are built for float32 and bfloat16 activations (got {d})")


ACT_NONE, ACT_RELU, ACT_SILU = 0, 1, 2
GATHER_ROWS, GATHER_UP2, GATHER_PATCH, GATHER_PATCH_NCHW, GATHER_PATCH_NCHW_U8, GATHER_PATCH_NCHW_BF16, GATHER_PATCH_NCHW_F16 = 0, 1, 2, 3, 4, 5, 6
PRO_NONE, PRO_GATE, PRO_AFFINE_RELU_CA = 0, 1, 2


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C lead-yolo_amd/csrc`). There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, args in SIGNATURES.items():
            fn = getattr(L, name)        # AttributeError if the symbol is not exported
            fn.restype = RESTYPES[name]
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        raise HipLibraryError(f"{what} failed (rc={rc}): {lib().ly_last_error().decode()}")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
