"""ctypes binding of libpvrl_hip.so (the C ABI declared in include/pvrl.h).

The prototypes, the struct layouts and the integer `#define`s (enums, limits) are parsed from the
header itself, so the header is the single source of truth: `tests/test_cabi.py` checks that every
declared symbol is exported and the parsed layouts against a C compiler's.
There is NO fallback: if the library is missing or a call fails, this raises.
"""
import ctypes
import functools
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(_HERE, "..", "include", "pvrl.h")

# The 16-bit operand type is fixed per library at build time (csrc/common.h).  Default since round 5: fp16 operands
# (libpvrl_hip_f16.so) -- the flavour that meets north_star's 1e-3 on step logits and losses against the fp32 reference (observed
# 2.9e-4 / 4e-6; same MFMA rate as bf16 on gfx950, gradients scaled inside each engine's backward).  PVRL_OPERAND=bf16 selects
# libpvrl_hip.so (8 exponent bits, no gradient scaling, ~3 % faster, logits 2e-3).  One flavour per process.
OPERAND = os.environ.get("PVRL_OPERAND", "f16").lower()
if OPERAND not in ("bf16", "f16"):
    raise RuntimeError(f"PVRL_OPERAND={OPERAND!r}: expected 'f16' or 'bf16'")
LIB_PATH = os.path.join(_HERE, "csrc", "libpvrl_hip.so" if OPERAND == "bf16" else "libpvrl_hip_f16.so")
# A/B runs against another build of the library (e.g. the parent commit's libpvrl_hip*.so); never set in production
LIB_PATH = os.environ.get("PVRL_LIB_PATH", LIB_PATH)


def operand_torch_dtype():
    import torch
    return torch.bfloat16 if OPERAND == "bf16" else torch.float16


class PvrlError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "double": ctypes.c_double}
_TXT = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(HEADER).read(), flags=re.S)      # the header without its comments
_CONSTANTS = {name: int(v) for name, v in re.findall(r"#define\s+(PVRL_\w+)\s+(-?\d+)", _TXT)}


def header_constants():
    """-> {name: value} of the header's integer `#define PVRL_*` (parsed once, at import)"""
    return _CONSTANTS


def parse_header():
    """-> {name: (restype_name, [(ctype_name, argname), ...])}"""
    protos = {}
    for ret, name, args in re.findall(r"\b(int64_t|int)\s+(pvrl_\w+)\s*\(([^)]*)\)\s*;", _TXT):
        parsed = []
        for a in args.split(","):
            a = " ".join(a.split())
            if a in ("void", ""):
                continue
            ty, argname = re.match(r"(.*?)(\w+)$", a).groups()
            parsed.append((ty.strip().replace(" *", "*"), argname))
        protos[name] = (ret, parsed)
    return protos


def _ctype(ty, structs=()):
    """C type spelling -> ctypes type: a scalar of _SCALARS, or c_void_p for a pointer to one, to void or to one of `structs`"""
    base = ty.replace("const ", "").rstrip("*")
    if ty.endswith("*") and (base == "void" or base in _SCALARS or base in structs):
        return ctypes.c_void_p
    return _SCALARS[ty]


def parse_structs(txt=_TXT):
    """-> {name: [(field, C type, array length or None), ...]} for every `typedef struct name {...} name;` of the header (or of
    the comment-free text `txt`).  A field is a scalar of _SCALARS, a pointer to one or to void, or a fixed array of those; anything
    else (bit-fields, nested or anonymous structs, function pointers, other types) raises PvrlError."""
    structs = {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", txt, flags=re.S):
        tag, body, name = m.groups()
        if tag != name or "{" in body:
            raise PvrlError(f"struct {tag}: expected `typedef struct {name} {{ plain fields }} {name};`")
        structs[name] = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            dm = re.fullmatch(r"((?:const )?\w+ ?\**) ?(\w+(?:\[\d+\])?(?:, ?\w+(?:\[\d+\])?)*)", decl)
            try:
                ty = dm.group(1).replace(" ", "").replace("const", "const ")
                _ctype(ty)
            except (AttributeError, KeyError):
                raise PvrlError(f"struct {name}: cannot parse the declaration `{decl}`") from None
            for item in dm.group(2).replace(" ", "").split(","):
                field, _, n = item.rstrip("]").partition("[")
                structs[name].append((field, ty, int(n) if n else None))
    if len(structs) != len(re.findall(r"\bstruct\b", txt)):
        raise PvrlError("a `struct` of the header is not of the form `typedef struct name { plain fields } name;`")
    return structs


# every argument type of the header's prototypes (a KeyError here: something other than a pointer or a plain scalar at the boundary)
_CTYPES = {ty: _ctype(ty, parse_structs()) for _, args in parse_header().values() for ty, _ in args}


def _struct_class(name):
    """the ctypes.Structure of the header's struct `name`; setting anything but a field of the header raises AttributeError"""
    fields = [(f, _ctype(ty) * n if n else _ctype(ty)) for f, ty, n in parse_structs()[name]]
    return type(name, (ctypes.Structure,), {"_fields_": fields, "__slots__": (), "__doc__": f"`{name}` of include/pvrl.h"})


def struct_dtype(name):
    """the numpy structured dtype of the header's struct `name`: the C layout, with explicit offsets and itemsize"""
    return np.dtype(_struct_class(name))


TnProblem, NtProblem, LnReduce = _struct_class("pvrl_tn_problem"), _struct_class("pvrl_nt_problem"), _struct_class("pvrl_ln_reduce")
# pvrl_rows: rows [0, rows16) in the 16-bit matrix `lo`, the rest in the fp32 matrix `hi`
Rows, CastProblem = _struct_class("pvrl_rows"), _struct_class("pvrl_cast_problem")


class _Lib:
    def __init__(self):
        if not os.path.exists(LIB_PATH):
            other = os.path.join(_HERE, "csrc", "libpvrl_hip_f16.so" if OPERAND == "bf16" else "libpvrl_hip.so")
            hint = (f"; {os.path.basename(other)} IS there: PVRL_OPERAND={'f16' if OPERAND == 'bf16' else 'bf16'} selects it "
                    "(the default is the fp16-operand library since round 5)") if os.path.exists(other) else ""
            raise PvrlError(
                f"{LIB_PATH} (PVRL_OPERAND={OPERAND}) is missing: build it with `python -m procedurevrl_amd.csrc.build_ext` "
                f"(there is no CPU or PyTorch fallback for the HIP path){hint}")
        self.cdll = ctypes.CDLL(LIB_PATH)
        self.protos = parse_header()
        self._fn = {}
        for name, (ret, args) in self.protos.items():
            fn = getattr(self.cdll, name)  # AttributeError -> loud failure on a missing export
            fn.restype = _SCALARS[ret]
            fn.argtypes = [_CTYPES[t] for t, _ in args]
            self._fn[name] = (fn, ret == "int", len(args))
        for k, v in header_constants().items():
            setattr(self, k, v)
        built = self.cdll.pvrl_operand_dtype()
        if built != (0 if OPERAND == "bf16" else 1):
            raise PvrlError(f"{LIB_PATH} was built for operand code {built}, PVRL_OPERAND={OPERAND}")

    def call(self, name, *args):
        fn, is_status, nargs = self._fn[name]
        if len(args) != nargs:     # ctypes itself refuses too few arguments but passes any number too many
            raise PvrlError(f"{name} takes {nargs} arguments (include/pvrl.h), {len(args)} given")
        rc = fn(*args)
        if is_status and rc != 0:
            raise PvrlError(f"{name} failed with status {rc}")
        return rc


@functools.lru_cache(maxsize=None)
def lib():
    return _Lib()
