"""The engines' backward passes under a changing gradient magnitude (tests/grad_scale_checks.py; pytest -m gpu).  Both library
flavours: the fp16-operand default scales its internal gradients by a device-chosen power of two S, the bf16 flavour does not -- the
rule "2^k x the loss gives 2^k x every gradient, bit for bit" holds for both, the oracle bars switch with PVRL_OPERAND (e2e_checks).

Measured on MI355X (the tables are in DESIGN.md section 4; each test prints its figures, `-s`):
  * covariance, replay at another scale, the all-zero gradient: bit-exact on every path in both flavours;
  * accumulation across two scales: worst element 0.25 x the bound -- after `temporal_fc.weight`, written by a GEMM and a rank-1 term
    that may cancel, missed it by up to 8,176 x on 2 % of its elements and the engine was changed to add the finished gradient once;
  * regimes: worst-gradient error / rounding model's 0.97 .. 1.38 (fp16), 1.00 .. 1.38 (bf16), bar 1.6;
  * headroom of the 16-bit row sums, fp16, 65,504 / max: dW_e 57 x / 8.0 x at 288 rows (randn / mean_pool), 4.8 x / 0.27 x at 50,176 rows --
    the mean-pooled all-token gradient overflowed; the engine now gives the dW_e copies a power of two of their own (2.2 x after it)."""

import pytest
import torch

import e2e_checks as ec
import grad_scale_checks as gc
import tokens_checks as tc

DEV = ec.DEV


@pytest.fixture(scope="module")
def gold():
    return tc.load()


# ------------------------------------------------------------------------------------------------------ 1. covariance
ENCODER_PATHS = {
    "divided": dict(),
    "divided_unpruned": dict(prune=(False, False)),
    "divided_fp32_stream": dict(resid16=False),
    "joint_space_time": dict(att="joint_space_time", crop=32, B=3),
    "space_only": dict(att="space_only", crop=32, B=3),
    "act_checkpoint": dict(ckpt=True),
    "width_1024": dict(large=True, crop=32, B=2),
    "streamed_336": dict(crop=336, frames=2, B=2, K=64),
}


@pytest.mark.gpu
@pytest.mark.parametrize("path", sorted(ENCODER_PATHS))
def test_encoder_step_is_covariant_under_a_power_of_two(path):
    gc.assert_covariant(gc.encoder_case(**ENCODER_PATHS[path]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tok_div", "tok_space", "tok_stream"])
def test_all_token_step_is_covariant_under_a_power_of_two(gold, name):
    """tok_div / tok_space: below begin_scaled's seam (one launch); tok_stream, 2 clips of 2 x 336^2 = 1.36 M elements: the torch branch"""
    f = gold[name]
    n = f["B"] * tc.n_tokens(f) * f["width"]
    assert (n > gc.SEAM) == (name == "tok_stream")
    gc.assert_covariant(gc.token_case(f))


@pytest.mark.gpu
def test_mvit_step_is_covariant_under_a_power_of_two():
    gc.assert_covariant(gc.mvit_case())


@pytest.mark.gpu
@pytest.mark.parametrize("head", ["head_engine", "stack_fn"])
def test_pretraining_step_is_covariant_under_a_power_of_two(head, monkeypatch):
    """PretrainHeadEngine, and the same head through autograd and functional.StackFn (its returned dx feeds the parameters upstream)"""
    monkeypatch.setenv("PVRL_HEAD_ENGINE", "1" if head == "head_engine" else "0")
    gc.assert_covariant(gc.pretrain_case())


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["divided", "tokens"])
def test_graph_captured_at_one_scale_replays_at_another(gold, path):
    gc.assert_replay_covariant(gc.encoder_case(graphs=True) if path == "divided" else gc.token_case(gold["tok_div"], graphs=True))


@pytest.mark.gpu
@pytest.mark.parametrize("hook", [False, True])
@pytest.mark.parametrize("path", ["divided", "tokens"])
def test_accumulation_across_two_scales(gold, path, hook):
    gc.assert_accumulates(gc.encoder_case() if path == "divided" else gc.token_case(gold["tok_div"]), hook_unscale=hook)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["divided", "tokens"])
def test_an_all_zero_incoming_gradient_gives_exact_zeros(gold, path):
    if path == "divided":
        model, _ = gc.encoder_case()
        x = torch.randn(2, 3, 8, 48, 48, generator=torch.Generator().manual_seed(1)).to(DEV)
        out = model.model.forward_features(x)
    else:
        f = gold["tok_div"]
        model, _ = gc.token_case(f)
        out = model.model.forward_features(tc.inputs(f)[0].to(DEV), cls=False)
    model.zero_grad(set_to_none=True)
    model.model.grad_store().bad.zero_()
    out.backward(torch.zeros_like(out))
    grads = gc.grads_of(model)
    assert grads
    gc.assert_finite(grads)
    nz = [k for k, g in grads.items() if bool((g != 0).any())]
    assert not nz, nz
    assert gc.skip_flag(model) == 0.0


# ------------------------------------------------------------------------------------------------------ 2. begin_scaled's two branches
@pytest.mark.gpu
@pytest.mark.parametrize("n", [gc.SEAM - 768, gc.SEAM, gc.SEAM + 768])
def test_begin_scaled_branches_agree_across_the_seam(n):
    g = gc.seam_gradient(n).to(DEV) * 3e-5
    bad, S = gc.check_branches(g)
    print(f"[n = {n}] S = {S}")
    assert not bad, bad
    # the product took the branch the size says
    gs = gc.new_store()
    gs.begin_scaled(g)
    assert (gs.inv.data_ptr() == gs.inv_row.data_ptr()) == (n <= gc.SEAM)


@pytest.mark.gpu
@pytest.mark.parametrize("j", [-20, 0, 8])
@pytest.mark.parametrize("nb", [-1, 0, 1])
def test_begin_scaled_branches_at_a_power_of_two_maximum(j, nb):
    for n in (gc.SEAM, 4099):
        g = gc.seam_gradient(n, j, nb).to(DEV)
        bad, S = gc.check_branches(g)
        print(f"[max|g| = 2^{j} {'+-'[nb < 0] + '1 ulp' if nb else ''}, n = {n}] S = {S}")
        assert not bad, bad


@pytest.mark.gpu
def test_begin_scaled_takes_a_non_contiguous_gradient():
    base = gc.seam_gradient(2 * 70001, seed=3).to(DEV).view(70001, 2)
    g = base.t()[1]
    assert not g.is_contiguous()
    gs = gc.new_store()
    out = gs.begin_scaled(g)
    import optim_checks as oc
    s = float(gs.scale)
    assert s in oc.gsb_allowed(float(g.abs().max()), True, gc.SCALE_TARGET)
    assert torch.equal(out, g * s) and bool((gs.inv_row == 1.0 / s).all()) and gs.inv_row.numel() == 4096
    out_k, s_k, _ = gc.begin_scaled_kernel(g.contiguous())
    assert float(s_k) == s and torch.equal(out_k, out.contiguous())


# ------------------------------------------------------------------------------------------------------ 3. regimes against the oracle
@pytest.fixture(scope="module")
def cls_setup():
    """e2e_checks._hip_vs_oracle's small step with the forward fixed: model on the device, its features, the oracle's inputs"""
    c = gc.CLS_GEOM
    label, sd, x = gc.cls_oracle_inputs()
    cfg = ec.make_cfg(c["depth"], c["crop"], c["K"], frames=c["frames"])
    model = ec.build(cfg, label.clone())
    vt = model.model
    vt.load_state_dict({**sd, **{k: v for k, v in vt.state_dict().items() if k.startswith("order_tfm.")}}, strict=True)
    model.to(DEV).train()
    vt.engine.use_graphs = False
    return model, sd, x


def _regime(tag, regime, hip_step, oracle, g, zeros):
    ref, mod = oracle(g, None), oracle(g, ec.OPERAND_DTYPE)
    hip = hip_step(g)
    bad, table, worst = gc.judge(regime, hip, ref, mod, zeros)
    gc.print_table(tag, table, worst)
    if regime == "outlier":         # a measurement for DESIGN, not a threshold: what the small clips keep next to a 2^10 outlier
        small = oracle(gc.small_part(regime, g), None)
        rows = []
        for k, r in ref.items():
            if k in hip and float(small[k].norm()) > 0:
                rows.append((float((hip[k].double().cpu() - r.double()).norm() / small[k].double().norm()), k))
        rows.sort(reverse=True)
        print(f"[{tag}] error relative to the small clips' own gradient: worst {rows[0][0]:.3e} ({rows[0][1]}), "
              f"median {rows[len(rows) // 2][0]:.3e}")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("regime", gc.CLS_REGIMES)
def test_cls_path_gradient_regimes_against_the_oracle(cls_setup, regime):
    model, sd, x = cls_setup
    vt = model.model
    g = gc.cls_gradient(regime, gc.CLS_GEOM["B"], 768)

    def hip_step(g):
        model.zero_grad(set_to_none=True)
        vt.forward_features(x.to(DEV)).backward(g.to(DEV))
        return {k: p.grad.detach().cpu() for k, p in vt.named_parameters() if p.grad is not None and k in sd}

    _regime(f"cls, {regime}", regime, hip_step, lambda g, r: gc.cls_oracle_grads(sd, x, g, r), g, gc.STRUCTURAL_ZEROS.get(("cls", regime), ()))


@pytest.fixture(scope="module")
def tok_setup(gold):
    out = {}
    for name in ("tok_div", "tok_space"):
        f = gold[name]
        model, sd = tc.make_model(f, drop_path=0.0)
        model = model.to(DEV).train()
        model.model.engine.use_graphs = False
        out[name] = (f, model, sd, tc.inputs(f)[0])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("regime", gc.TOK_REGIMES)
@pytest.mark.parametrize("name", ["tok_div", "tok_space"])
def test_all_token_gradient_regimes_against_the_oracle(tok_setup, name, regime):
    f, model, sd, x = tok_setup[name]
    vt = model.model
    g = gc.tok_gradient(regime, f["B"], tc.n_tokens(f), f["width"])

    def hip_step(g):
        model.zero_grad(set_to_none=True)
        vt.forward_features(x.to(DEV), cls=False).backward(g.to(DEV))
        return {k: p.grad.detach().cpu() for k, p in vt.named_parameters() if p.grad is not None and k in sd}

    _regime(f"{name}, {regime}", regime, hip_step, lambda g, r: gc.tok_oracle_grads(f, sd, x, g, r), g,
            gc.STRUCTURAL_ZEROS.get((name, regime), ()))


# ------------------------------------------------------------------------------------------------------ 4. headroom of the 16-bit row sums
@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["randn", "mean_pool"])
def test_row_sum_headroom_at_288_rows(regime):
    """depth 1, 4 clips of 8 x 48^2: 288 patch rows"""
    model = gc.headroom_model(4, 48)
    x = torch.randn(4, 3, 8, 48, 48, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    maxima, _ = gc.headroom_run(model, x, gc.headroom_dtok(regime, 4, 1 + 9 * 8, 768), ks=gc.KS_REPLAY)
    print(f"[288 rows, {regime}, {ec.OPERAND}] max|value| into the 16-bit casts: {maxima}; headroom below 65504: "
          + ", ".join(f"{k} {gc.FP16_MAX / v:.1f}x" for k, v in maxima.items() if v))
    assert maxima["dW_e"] is not None, "the probe saw no dW_e cast"


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["randn", "mean_pool"])
def test_row_sum_headroom_at_the_production_row_count(regime):
    """depth 1, 32 clips of 8 x 224^2, ViT-B: 50,176 patch rows -- the row count is the variable under test (no oracle, one step + two for
    the covariance at k = +-9)"""
    model = gc.headroom_model(32, 224)
    x = torch.randn(32, 3, 8, 224, 224, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    maxima, _ = gc.headroom_run(model, x, gc.headroom_dtok(regime, 32, 1 + 196 * 8, 768), ks=gc.KS_REPLAY)
    print(f"[50176 rows, {regime}, {ec.OPERAND}] max|value| into the 16-bit casts: {maxima}; headroom below 65504: "
          + ", ".join(f"{k} {gc.FP16_MAX / v:.1f}x" for k, v in maxima.items() if v))
    assert maxima["dW_e"] is not None, "the probe saw no dW_e cast"


@pytest.mark.gpu
def test_the_row_sum_copies_own_power_of_two_costs_no_accuracy():
    """288 rows, mean_pool, with the engine's limit lowered to 64 so that e = 7 or 8 where the default has e = 0: every gradient but the two the
    chain GEMMs write is bit-equal; those two differ by what falls into fp16's subnormals after the shift, far below one 16-bit rounding
    (2^-11) of the copies themselves.  The bf16 flavour has fp32's exponent range and takes no such power of two: every gradient bit-equal."""
    model = gc.headroom_model(4, 48)
    x = torch.randn(4, 3, 8, 48, 48, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    dtok = gc.headroom_dtok("mean_pool", 4, 1 + 9 * 8, 768)
    eng = model.model.engine
    m0, g0 = gc.headroom_run(model, x, dtok)
    eng.DWE_LIMIT = 64.0
    try:
        m1, g1 = gc.headroom_run(model, x, dtok, ks=gc.KS_REPLAY)
    finally:
        del eng.DWE_LIMIT
    chain = [k for k in g0 if k.endswith("temporal_fc.weight") or k.endswith("temporal_attn.proj.weight")]
    assert len(chain) == 2
    if gc.SCALED:
        assert m0["dW_e"] == m0["dW_e_sum"] == m1["dW_e_sum"] > 64.0 >= m1["dW_e"] > 16.0, (m0, m1)
    else:
        assert m0 == m1, (m0, m1)
        chain = []
    for k in g0:
        if k in chain:
            e = ec.rel(g1[k], g0[k])
            print(f"{k}: {e:.3e}")
            assert e <= 2.0 ** -11, (k, e)
        else:
            assert torch.equal(g0[k], g1[k]), k
