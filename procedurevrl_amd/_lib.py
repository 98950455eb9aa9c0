"""ctypes binding of libpvrl_hip.so (the C ABI declared in include/pvrl.h).

The prototypes are parsed from the header itself, so the header is the single source of
truth and `tests/test_cabi.py` can check that every declared symbol is exported.
There is NO fallback: if the library is missing or a call fails, this raises.
"""
import ctypes
import os
import re

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

_CTYPES = {
    "const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "void**": ctypes.c_void_p,
    "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p, "int*": ctypes.c_void_p, "const void**": ctypes.c_void_p, "const float**": ctypes.c_void_p, "float**": ctypes.c_void_p,
    "const int64_t*": ctypes.c_void_p, "const pvrl_mix_desc*": ctypes.c_void_p, "const pvrl_ra_desc*": ctypes.c_void_p,
    "int32_t*": ctypes.c_void_p, "int64_t*": ctypes.c_void_p,
    "const pvrl_tn_problem*": ctypes.c_void_p, "const pvrl_cast_problem*": ctypes.c_void_p, "const pvrl_nt_problem*": ctypes.c_void_p, "const pvrl_ln_reduce*": ctypes.c_void_p, "const pvrl_rows*": ctypes.c_void_p,
    "int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
}
_RET = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}


def parse_header(path=HEADER):
    """-> {name: (restype_name, [(ctype_name, argname), ...])}"""
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    protos = {}
    for m in re.finditer(r"\b(int64_t|int)\s+(pvrl_\w+)\s*\(([^)]*)\)\s*;", txt):
        ret, name, args = m.group(1), m.group(2), m.group(3)
        parsed = []
        for a in args.split(","):
            a = " ".join(a.split())
            if a in ("void", ""):
                continue
            mm = re.match(r"(.*?)(\w+)$", a)
            ty = mm.group(1).strip().replace(" *", "*")
            parsed.append((ty, mm.group(2)))
        protos[name] = (ret, parsed)
    return protos


def header_constants(path=HEADER):
    txt = open(path).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(PVRL_\w+)\s+(-?\d+)", txt)}


class TnProblem(ctypes.Structure):
    """`pvrl_tn_problem` of include/pvrl.h"""
    _fields_ = [("P", ctypes.c_void_p), ("ldp", ctypes.c_int64), ("Q", ctypes.c_void_p), ("ldq", ctypes.c_int64),
                ("M", ctypes.c_int64), ("N", ctypes.c_int64), ("K", ctypes.c_int64), ("beta", ctypes.c_float),
                ("dW", ctypes.c_void_p), ("dbias", ctypes.c_void_p), ("gscale", ctypes.c_void_p), ("nonfinite", ctypes.c_void_p)]


class NtProblem(ctypes.Structure):
    """`pvrl_nt_problem` of include/pvrl.h"""
    _fields_ = [("A", ctypes.c_void_p), ("lda", ctypes.c_int64), ("W", ctypes.c_void_p), ("ldw", ctypes.c_int64),
                ("M", ctypes.c_int64), ("N", ctypes.c_int64), ("K", ctypes.c_int64), ("bias", ctypes.c_void_p),
                ("rowscale", ctypes.c_void_p), ("aux", ctypes.c_void_p), ("aux_ld", ctypes.c_int64), ("out0", ctypes.c_void_p),
                ("ld0", ctypes.c_int64)]


class LnReduce(ctypes.Structure):
    """`pvrl_ln_reduce` of include/pvrl.h"""
    _fields_ = [("part", ctypes.c_void_p), ("M", ctypes.c_int64), ("C", ctypes.c_int64), ("want_sum", ctypes.c_int),
                ("beta", ctypes.c_float), ("beta_sum", ctypes.c_float), ("dgamma", ctypes.c_void_p), ("dbeta", ctypes.c_void_p),
                ("dxsum", ctypes.c_void_p)]


class Rows(ctypes.Structure):
    """`pvrl_rows` of include/pvrl.h: rows [0, rows16) in the 16-bit matrix `lo`, the rest in the fp32 matrix `hi`"""
    _fields_ = [("lo", ctypes.c_void_p), ("ldlo", ctypes.c_int64), ("hi", ctypes.c_void_p), ("ldhi", ctypes.c_int64),
                ("rows16", ctypes.c_int64)]


class CastProblem(ctypes.Structure):
    """`pvrl_cast_problem` of include/pvrl.h"""
    _fields_ = [("inp", ctypes.c_void_p), ("out", ctypes.c_void_p), ("out_t", ctypes.c_void_p), ("R", ctypes.c_int64),
                ("C", ctypes.c_int64)]


class PvrlError(RuntimeError):
    pass


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
            fn.restype = _RET[ret]
            fn.argtypes = [_CTYPES[t] for t, _ in args]
            self._fn[name] = (fn, ret == "int")
        for k, v in header_constants().items():
            setattr(self, k, v)
        built = self.cdll.pvrl_operand_dtype()
        if built != (0 if OPERAND == "bf16" else 1):
            raise PvrlError(f"{LIB_PATH} was built for operand code {built}, PVRL_OPERAND={OPERAND}")

    def call(self, name, *args):
        fn, is_status = self._fn[name]
        rc = fn(*args)
        if is_status and rc != 0:
            raise PvrlError(f"{name} failed with status {rc}")
        return rc


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _Lib()
    return _lib
