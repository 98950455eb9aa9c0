"""The C-ABI library loads on a CPU-only host and exports every symbol include/pvrl.h declares (no compute calls)."""
import ctypes
import os

from procedurevrl_amd import _lib


def test_header_parses_and_lists_entry_points():
    protos = _lib.parse_header()
    assert len(protos) >= 24
    for must in ("pvrl_gemm_nt_bf16", "pvrl_gemm_tn_bf16", "pvrl_layernorm_fwd", "pvrl_layernorm_bwd", "pvrl_attn_fwd",
                 "pvrl_attn_bwd", "pvrl_attn_t8_fwd", "pvrl_attn_t8_bwd", "pvrl_patchify", "pvrl_kl_topk", "pvrl_mse",
                 "pvrl_adam_step", "pvrl_sgd_step"):
        assert must in protos
    for name, (ret, args) in protos.items():
        assert ret in ("int", "int64_t")
        for ty, _ in args:
            assert ty in _lib._CTYPES, (name, ty)   # plain pointers and sizes only: no torch types at the boundary


def test_library_exports_every_declared_symbol():
    if not os.path.exists(_lib.LIB_PATH):
        from procedurevrl_amd.csrc import build_ext
        build_ext.build(verbose=False)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in _lib.parse_header():
        assert hasattr(cdll, name), f"{name} declared in include/pvrl.h but not exported"
    L = _lib.lib()
    assert L.PVRL_EPI_RESID_F32 == 3 and L.PVRL_EPI_DQGELU == 6 and L.PVRL_EPI_RESID_16 == 7


def test_pure_size_queries_run_without_a_gpu():
    L = _lib.lib()
    assert L.call("pvrl_gemm_tn_workspace_bytes", 768, 768, 8) == 8 * (768 * 768 + 768) * 4 + 256
    # one workgroup per 4 rows + one (a split matrix, pvrl_rows, always has a workgroup for each of its parts), at most 512
    assert L.call("pvrl_layernorm_bwd_workspace_bytes", 100, 768) == 26 * 3 * 768 * 4
    assert L.call("pvrl_layernorm_bwd_workspace_bytes", 50208, 768) == 512 * 3 * 768 * 4


def test_grouped_weight_gradient_plan_runs_without_a_gpu():
    """pvrl_gemm_tn_grouped_plan_splits / _workspace_bytes are pure host functions: a transformer block's seven weight
    gradients (153 tiles of 256x256) are cut into 5 row slices = 765 work items = 2.99 rounds of 256 CUs; shapes that are
    not multiples of 128, an empty list and more than 8 problems are refused."""
    import ctypes as C
    L = _lib.lib()
    M = 50208
    dims = [(768, 3072), (3072, 768), (768, 768), (2304, 768), (768, 768), (768, 768), (2304, 768)]
    arr = (_lib.TnProblem * len(dims))()
    for a, (N, K) in zip(arr, dims):
        a.P, a.ldp, a.Q, a.ldq, a.M, a.N, a.K, a.beta, a.dW, a.dbias = 16, N, 16, K, M, N, K, 0.0, 16, None
    ap = C.addressof(arr)
    assert L.call("pvrl_gemm_tn_grouped_plan_splits", len(dims), ap) == 5
    want = sum(5 * (N * K + N) * 4 for N, K in dims)
    assert L.call("pvrl_gemm_tn_grouped_workspace_bytes", len(dims), ap, 5) == want
    arr[2].N = 640                                            # half tiles (128 mod 256) are staged with zero columns
    assert L.call("pvrl_gemm_tn_grouped_plan_splits", len(dims), ap) >= 1
    arr[2].N = 600                                            # not a multiple of 128
    assert L.call("pvrl_gemm_tn_grouped_plan_splits", len(dims), ap) == -1
    assert L.call("pvrl_gemm_tn_grouped_plan_splits", 0, ap) == -1
    assert L.call("pvrl_gemm_tn_grouped_plan_splits", 9, ap) == -1
    assert L.call("pvrl_mvit_pool_bwd_workspace_bytes") == (2048 * 27 * 96 + 2048 * 2 * 96) * 4


def test_product_path_fails_loudly_without_gpu():
    import pytest
    import torch
    from procedurevrl_amd import ops
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.PvrlError):
        ops.layernorm_fwd(torch.zeros(4, 768), torch.ones(768), torch.zeros(768), 1e-6)


def test_rel_operand_form_round_trips_on_the_host():
    """ops_mvit.rel_pack / rel_unpack (the hi | lo 16-bit pair pvrl_mvit_rel_fwd writes and pvrl_mvit_attn_* read): width from
    the C side, padding columns zero, value recovered to ~2^-16 -- pure host code plus two size queries."""
    import torch
    from procedurevrl_amd import ops_mvit as om
    assert om.rel_width((8, 7, 7)) == 32 and om.rel_width((8, 14, 14)) == 64
    L = _lib.lib()
    assert L.call("pvrl_mvit_attn_keymap_bytes", 8, 7, 7) == 13 * 4096 and L.call("pvrl_mvit_attn_keymap_bytes", 8, 14, 14) == 50 * 4096
    g = torch.Generator().manual_seed(0)
    for k_thw in ((8, 7, 7), (8, 14, 14)):
        J = sum(k_thw)
        rel = torch.randn(3, 10, J, generator=g) * 3
        for osc in (1.0, 96 ** 0.5):
            relp = om.rel_pack(rel, k_thw, osc)
            JP = om.rel_width(k_thw)
            assert relp.shape == (3, 10, 2 * JP)
            assert float(relp[..., J:JP].float().abs().max()) == 0.0 and float(relp[..., JP + J:].float().abs().max()) == 0.0
            back = om.rel_unpack(relp, k_thw, osc)
            assert float((back - rel).abs().max() / rel.abs().max()) < 2e-5


# ---- the header is the one statement of the ABI: struct layouts, enums and limits -------------------------------------
STRUCT_SIZES = {"pvrl_nt_problem": 104, "pvrl_tn_problem": 96, "pvrl_rows": 40, "pvrl_ln_reduce": 64, "pvrl_cast_problem": 40,
                "pvrl_mix_desc": 32, "pvrl_ra_desc": 64}       # sizeof on the LP64 hosts the library is built for
EXPORTED = {"pvrl_nt_problem": "NtProblem", "pvrl_tn_problem": "TnProblem", "pvrl_rows": "Rows", "pvrl_ln_reduce": "LnReduce",
            "pvrl_cast_problem": "CastProblem"}


def _layouts():
    """-> {struct: (ctypes class, numpy dtype)} for every struct of the header; the five exported classes are the exported objects"""
    return {name: (getattr(_lib, EXPORTED[name]) if name in EXPORTED else _lib._struct_class(name), _lib.struct_dtype(name))
            for name in _lib.parse_structs()}


def _host_cc():
    import shutil
    from procedurevrl_amd.csrc import build_ext
    hipcc = shutil.which(build_ext._hipcc()) or ""
    near = [os.path.join(os.path.dirname(os.path.realpath(hipcc)), *rel) for rel in (("clang",), ("..", "llvm", "bin", "clang"),
                                                                                     ("..", "lib", "llvm", "bin", "clang"))]
    return shutil.which("cc") or next((c for c in near if hipcc and os.path.exists(c)), None)


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and every offsetof, as the host C compiler lays out include/pvrl.h, against the ctypes classes and struct_dtype()"""
    import subprocess
    import pytest
    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler")
    structs = _lib.parse_structs()
    lines = [f'  printf("{s} - %zu\\n", sizeof({s}));' for s in structs]
    lines += [f'  printf("{s} {f} %zu\\n", offsetof({s}, {f}));' for s, fields in structs.items() for f, _, _ in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pvrl.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-I", os.path.dirname(os.path.abspath(_lib.HEADER)), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = 0
    for s, f, n in (ln.split() for ln in out if ln):
        cls, dt = _layouts()[s]
        if f == "-":
            assert ctypes.sizeof(cls) == int(n) == dt.itemsize, (s, n)
        else:
            assert getattr(cls, f).offset == int(n) == dt.fields[f][1], (s, f, n)
            assert getattr(cls, f).size == dt.fields[f][0].itemsize, (s, f)
        seen += 1
    assert seen == len(structs) + sum(len(v) for v in structs.values()) and len(structs) == 7


def test_struct_sizes_are_the_pinned_ones():
    """the same seven sizes as literals: holds on a host without a compiler too"""
    lay = _layouts()
    assert sorted(lay) == sorted(STRUCT_SIZES)
    for name, size in STRUCT_SIZES.items():
        cls, dt = lay[name]
        assert ctypes.sizeof(cls) == size == dt.itemsize, name
        assert [f for f, _ in cls._fields_] == list(dt.names) == [f for f, _, _ in _lib.parse_structs()[name]]
    assert [f for f, _ in _lib.TnProblem._fields_] == ["P", "ldp", "Q", "ldq", "M", "N", "K", "beta", "dW", "dbias", "gscale", "nonfinite"]
    assert _lib.struct_dtype("pvrl_ra_desc").fields["c"][0].shape == (6,) and _lib.struct_dtype("pvrl_ra_desc").fields["iarg"][0].shape == (2,)


def test_struct_classes_refuse_names_the_header_does_not_have():
    """a misspelt or dropped field must not become a silent Python attribute next to a null C field"""
    import pytest
    c = _lib.CastProblem()
    setattr(c, "in", 16)
    c.out, c.out_t, c.R, c.C = 32, None, 3, 5
    assert getattr(c, "in") == 16 and (c.out, c.out_t, c.R, c.C) == (32, None, 3, 5)
    for cls in (_lib.CastProblem, _lib.TnProblem, _lib.NtProblem, _lib.LnReduce, _lib.Rows):
        with pytest.raises(AttributeError):
            cls().inp = 16
        with pytest.raises(AttributeError):
            (cls * 2)()[1].inp = 16


def test_limits_come_from_the_header():
    from procedurevrl_amd import ops, ops_mvit, mvit
    hc = _lib.header_constants()
    assert ops.ATTN_MAX_S == 416 == hc["PVRL_ATTN_MAX_S"]
    assert ops.ATTN_CLS_MAX_S == 4096 == hc["PVRL_ATTN_CLS_MAX_S"]
    assert ops.TN_GROUP_MAX == 8 == hc["PVRL_TN_GROUP_MAX"]
    assert (ops.NT_SKINNY_MAX_M, ops.NT_SKINNY_K) == (192, 256) == (hc["PVRL_NT_SKINNY_MAX_M"], hc["PVRL_NT_SKINNY_K"])
    assert ops.HEAD_DIM == 64 == hc["PVRL_HEAD_DIM"] and ops_mvit.HD == mvit.HD == 96 == hc["PVRL_MVIT_HEAD_DIM"]
    assert hc is _lib.header_constants()                      # parsed once


def test_call_refuses_a_wrong_argument_count():
    """ctypes alone passes surplus arguments silently; L.call compares with the prototype.  A pure host query: nothing is launched."""
    import pytest
    L = _lib.lib()
    for args in ((768, 768, 8, 1), (768, 768)):
        with pytest.raises(_lib.PvrlError, match=rf"pvrl_gemm_tn_workspace_bytes takes 3 arguments .* {len(args)} given"):
            L.call("pvrl_gemm_tn_workspace_bytes", *args)


def test_struct_parser_refuses_what_it_does_not_understand():
    import pytest
    ok = "typedef struct s {\n  const float* a; int64_t m, n;\n  double c[6];\n} s;"
    assert _lib.parse_structs(ok) == {"s": [("a", "const float*", None), ("m", "int64_t", None), ("n", "int64_t", None), ("c", "double", 6)]}
    for body in ("int a : 3;",                                  # bit-field
                 "struct { int a; } inner;",                    # nested struct
                 "int (*fn)(int);",                             # function pointer
                 "unsigned int a;", "size_t a;", "pvrl_rows r;", "int a[N];", "float *a, *b;"):
        with pytest.raises(_lib.PvrlError):
            _lib.parse_structs("typedef struct s { int64_t n; %s } s;" % body)
    for txt in ("typedef struct { int a; } s;", "typedef struct t { int a; } s;", "struct s { int a; };"):
        with pytest.raises(_lib.PvrlError):
            _lib.parse_structs(txt)
