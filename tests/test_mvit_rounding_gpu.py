"""MViTEngine's step held to the rounding model oracle/mvit_rounded_oracle.py (tests/mvit_rounding_checks.py: cases and rule), pytest -m gpu.
The flavour under test is the library's (fp16 operands by default, PVRL_OPERAND=bf16 the other); `-s` prints the ratios recorded in
mvit_rounding_checks' docstring."""
import pytest
import torch

import mvit_rounding_checks as rc


@pytest.fixture(scope="module")
def engine_model():
    return rc.build_engine_model()


def _operand():
    import e2e_checks as ec
    return ec.OPERAND_DTYPE


@pytest.mark.gpu
@pytest.mark.parametrize("case", rc.CASES)
def test_mvit_step_vs_rounding_model(engine_model, case):
    got = rc.hip_case(engine_model, case)          # the case's own input and the draws the small tensors are judged over
    findings, table = rc.judge(case, _operand(), got)
    rc.report(f"{case} {_operand()}", findings, table)
    bad = rc.failures(findings)
    assert not bad, "\n".join(f"{label}: {v:.3f} > {b:g}" for label, v, b in bad)


@pytest.mark.gpu
def test_mvit_graph_replay_gradients_equal_eager(engine_model):
    """the `fixture` step replayed from HIP graphs (second call with use_graphs): features and all 105 gradients bit-equal to the eager step's"""
    eager = rc.hip_step(engine_model, "fixture")
    try:
        for _ in range(engine_model.model.engine.GRAPH_WARMUP + 1):
            rc.hip_step(engine_model, "fixture", graphs=True)
        assert len(engine_model.model.engine._graphs) >= 1, "the step was not captured"
        replay = rc.hip_step(engine_model, "fixture", graphs=True)
    finally:
        engine_model.model.engine.use_graphs = False
    assert torch.equal(replay["feat"], eager["feat"])
    assert len(replay["grads"]) == rc.N_PARAMS
    bad = [k for k in eager["grads"] if not torch.equal(replay["grads"][k], eager["grads"][k])]
    assert not bad, f"gradients that differ between graph replay and eager launches: {bad}"
