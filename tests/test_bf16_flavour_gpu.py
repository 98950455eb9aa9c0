"""The bf16-operand flavour of the library (libpvrl_hip.so, PVRL_OPERAND=bf16): the side flavour since round 5.

The default library rounds GEMM / attention operands to fp16 and is held to north_star's 1e-3 on logits and losses by the
default `-m gpu` suite (e2e_checks.TOL_ACT / TOL_LOSS).  The same kernels built with bf16 operands (the type BASELINE's configs
name; 8 exponent bits, no gradient scaling, ~3 % faster) carry an 8x larger unit roundoff: 2e-3 on logits after 12 blocks with
the cls rows' chain in fp32.  That flavour must keep passing its own (looser, e2e_checks / kernel_checks) bounds: one library
flavour per process, so its kernel, end-to-end, optimiser, MViT and per-row attention, pooling-attention, pooling-operator, row-kernel, optimiser-kernel, gradient-scale and MViT rounding-model checks (whose
bounds follow the bf16 rounding model by themselves) run in a child process."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bf16_operand_flavour():
    env = dict(os.environ, PVRL_OPERAND="bf16")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_e2e_gpu.py"),
                        os.path.join(ROOT, "tests", "test_kernels_gpu.py"), os.path.join(ROOT, "tests", "test_optimizer_gpu.py"),
                        os.path.join(ROOT, "tests", "test_mvit_gpu.py"), os.path.join(ROOT, "tests", "test_attention_gpu.py"),
                        os.path.join(ROOT, "tests", "test_pool_attention_gpu.py"), os.path.join(ROOT, "tests", "test_mvit_pool_gpu.py"),
                        os.path.join(ROOT, "tests", "test_row_kernels_gpu.py"), os.path.join(ROOT, "tests", "test_optim_kernels_gpu.py"),
                        os.path.join(ROOT, "tests", "test_grad_scale_gpu.py"), os.path.join(ROOT, "tests", "test_mvit_rounding_gpu.py"),
                        "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=1800)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-1000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "failed" not in r.stdout, tail
