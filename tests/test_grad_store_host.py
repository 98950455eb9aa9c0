"""grads.GradStore on the CPU: the flat layout, the two gradient protocols ("fused", and "touched then unscale()"), the foreign
.grad tensor, the sets that decide what the optimiser scans, prezero's fills and accumulate.  `begin_scaled` takes its torch branch
here (its one-launch branch is tests/kernel_checks.check_grad_scale_begin's)."""
import math

import pytest
import torch

from procedurevrl_amd.grads import GradStore

SHAPES = [(5, 7), (100,), (3,)]          # 35, 100, 3 elements -> 64, 128, 64 with the padding


def make():
    g = torch.Generator().manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]
    return GradStore([(f"p{i}", p) for i, p in enumerate(ps)], "cpu"), ps


def incoming(amax=1.3e-5, n=24):
    """a gradient entering an engine: max |g| = amax"""
    g = torch.linspace(-0.7, 1.0, n) * amax
    assert float(g.abs().max()) == pytest.approx(amax)
    return g


def is_pow2(v):
    return math.isfinite(v) and v > 0.0 and math.frexp(v)[0] == 0.5


def test_layout():
    gs, ps = make()
    assert gs.offsets == [0, 64, 192] and gs.end == 256
    assert [gs.span(i) for i in range(3)] == [(0, 64), (64, 192), (192, 256)]            # padding included
    base = gs.flat.data_ptr()
    assert gs.used.data_ptr() == base + 4 * 256 and gs.used.numel() == 3                    # the tail sits behind `end`
    assert gs.ctl.data_ptr() == base + 4 * 259 and gs.ctl.numel() == 1
    assert gs.bad.data_ptr() == base + 4 * 260 and gs.bad.numel() == 1
    assert gs.flat.numel() >= 261 and gs.flat.numel() % 64 == 0
    for i, (v, p) in enumerate(zip(gs.views, ps)):
        assert v.shape == p.shape and v.data_ptr() == base + 4 * gs.offsets[i]
        v.fill_(i + 1.0)
        a = gs.offsets[i]
        assert bool((gs.flat[a:a + p.numel()] == i + 1.0).all())                           # a view of `flat`, not a copy
    assert float(gs.flat.sum()) == 35 * 1.0 + 100 * 2.0 + 3 * 3.0                           # ... and nothing else was written


def test_target_first_second_and_foreign():
    gs, ps = make()
    t, beta = gs.target(ps[0])
    assert beta == 0.0 and t is gs.views[0] and ps[0].grad is gs.views[0]                  # first touch installs the view
    t, beta = gs.target(ps[0])
    assert beta == 1.0 and t is gs.views[0]
    foreign = torch.ones(100)
    ps[1].grad = foreign
    t, beta = gs.target(ps[1])
    assert t is foreign and beta == 1.0 and ps[1].grad is foreign


def test_scaled_protocol_returns_true_units():
    gs, ps = make()
    g = incoming()
    out = gs.begin_scaled(g)
    S = float(gs.scale)
    assert is_pow2(S) and 128.0 < S * float(g.abs().max()) <= 256.0
    assert float(gs.inv) == 1.0 / S and torch.equal(out, g * S)
    true0 = torch.arange(35.0).view(5, 7) * 1e-6
    foreign = torch.full((100,), 0.25)
    delta = torch.arange(100.0) * 1e-3
    ps[1].grad = foreign
    t0, b0 = gs.target(ps[0])
    t0.copy_(true0 * S)                                         # an engine writes S-scaled values
    t1, b1 = gs.target(ps[1])
    assert b0 == 0.0 and t1 is foreign and b1 == 1.0
    assert torch.equal(foreign, torch.full((100,), 0.25 * S))   # what was there joins the S-scaled units at the first touch ...
    assert gs.target(ps[1])[0] is foreign
    assert torch.equal(foreign, torch.full((100,), 0.25 * S))   # ... and only then
    t1.add_(delta * S)
    inv = gs.end_scaled()
    assert float(inv) == 1.0 / S and gs.scale is None and gs.inv is None
    assert torch.equal(ps[0].grad, true0)                       # scaling by a power of two is exact
    assert torch.equal(foreign, 0.25 + delta)                   # multiplied by 1 / S exactly once


def test_unscale_between_blocks_then_second_write():
    gs, ps = make()
    gs.begin_scaled(incoming())
    S = float(gs.scale)
    a = torch.arange(100.0) * 1e-4
    b = torch.arange(100.0, 0.0, -1.0) * 1e-5
    foreign = torch.zeros(3)
    ps[2].grad = foreign
    gs.target(ps[1])[0].copy_(a * S)
    gs.target(ps[2])[0].add_(a[:3] * S)
    gs.unscale()                                                # a block is done: its gradients are in true units
    assert torch.equal(ps[1].grad, a) and torch.equal(foreign, a[:3])
    gs.unscale()                                                # nothing touched since: no second multiply
    assert torch.equal(ps[1].grad, a) and torch.equal(foreign, a[:3])
    t, beta = gs.target(ps[1])                                  # the same parameters again, now accumulating
    assert beta == 1.0
    t.add_(b * S)
    gs.target(ps[2])[0].add_(b[:3] * S)
    gs.end_scaled()
    assert torch.allclose(ps[1].grad, a + b, rtol=1e-6, atol=0.0)      # (a / S + b if the first write were unscaled twice)
    assert torch.allclose(foreign, a[:3] + b[:3], rtol=1e-6, atol=0.0)


def test_fused_protocol_and_the_optimiser_scan_sets():
    gs, ps = make()
    gs.begin_scaled(incoming())
    t, beta = gs.target(ps[0], fused=True)
    t.fill_(3.0)                                                # a fused kernel writes true units itself
    assert beta == 0.0 and gs._touched == [] and gs.fused_checked == {0}
    t, beta = gs.target(ps[0], fused=True)
    assert t is gs.views[0] and beta == 1.0 and gs._touched == []
    gs.end_scaled()
    assert bool((ps[0].grad == 3.0).all())                      # nothing was registered for unscale()
    # one unchecked writer keeps the parameter in the scan, whichever order the writers come in
    gs.target(ps[0], fused=True, checks=False)
    assert 0 not in gs.fused_checked
    gs.target(ps[0], fused=True)
    assert 0 not in gs.fused_checked
    gs.target(ps[1], fused=True, checks=False)
    gs.target(ps[1], fused=True)
    assert 1 not in gs.fused_checked
    # a foreign .grad is not the optimiser's flat buffer: never marked as checked
    foreign = torch.zeros(3)
    ps[2].grad = foreign
    t, beta = gs.target(ps[2], fused=True)
    assert t is foreign and beta == 1.0 and gs.fused_checked == set()


def test_prezero_one_fill_per_contiguous_run(monkeypatch):
    fills = []
    zero_ = torch.Tensor.zero_
    monkeypatch.setattr(torch.Tensor, "zero_", lambda t: (fills.append(t.numel()), zero_(t))[1])
    gs, ps = make()
    gs.flat.fill_(7.0)                                          # stale sentinels, padding included
    gs.prezero([ps[1], ps[0]])                                  # adjacent spans [0, 64) + [64, 192)
    assert fills == [192]
    assert bool((gs.flat[:192] == 0.0).all()) and bool((gs.flat[192:] == 7.0).all())
    assert ps[0].grad is gs.views[0] and ps[1].grad is gs.views[1] and ps[2].grad is None
    assert gs.target(ps[0])[1] == 1.0                           # .grad is installed: the next writer accumulates
    gs.prezero(ps)                                              # only the one without a gradient is cleared
    assert fills == [192, 64] and ps[2].grad is gs.views[2]

    fills.clear()
    gs, ps = make()
    gs.flat.fill_(7.0)
    gs.prezero([ps[0], ps[2]])                                  # not adjacent: two runs, p1's span stays as it is
    assert fills == [64, 64] and bool((gs.flat[64:192] == 7.0).all()) and float(gs.flat[:64].abs().sum() + gs.flat[192:256].abs().sum()) == 0.0


def test_prezero_inside_a_scaled_region_is_unscaled_with_the_rest():
    gs, ps = make()
    gs.begin_scaled(incoming())
    S = float(gs.scale)
    gs.prezero([ps[0], ps[1]])
    w = torch.arange(35.0).view(5, 7) * 1e-6
    ps[0].grad.add_(w * S)                                      # atomics / beta = 1 kernels: S-scaled sums onto the zeros
    ps[0].grad.add_(w * S)
    gs.unscale()                                                # a block is done; p1 is a later block's, still zeros
    assert torch.equal(ps[0].grad, 2 * w)
    v = torch.arange(100.0) * 1e-6
    t, beta = gs.target(ps[1])
    t.add_(v * S)
    gs.end_scaled()
    assert beta == 1.0 and torch.equal(ps[0].grad, 2 * w) and torch.equal(ps[1].grad, v)


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_begin_scaled_with_a_nonfinite_gradient(value):
    gs, _ = make()
    g = incoming()
    g[5] = value
    out = gs.begin_scaled(g)
    S, inv = float(gs.scale), float(gs.inv)
    assert is_pow2(S) and is_pow2(inv) and S * inv == 1.0
    assert not bool(torch.isfinite(out[5])) and bool(torch.isfinite(out[:5]).all())     # the bad value flows on, the rest stays usable
    gs.end_scaled()


@pytest.mark.parametrize("fused", [False, True])
def test_accumulate_copies_then_adds(fused):
    gs, ps = make()
    kw = dict(fused=True, checks=False) if fused else {}
    g = torch.arange(35.0)
    gs.flat.fill_(7.0)                                          # beta = 0 must overwrite what is there
    gs.accumulate(ps[0], g, **kw)                               # (a [35] gradient for a [5, 7] parameter: view_as)
    assert ps[0].grad is gs.views[0] and torch.equal(ps[0].grad, g.view(5, 7))
    gs.accumulate(ps[0], g.view(5, 7), **kw)
    assert torch.equal(gs.views[0], 2 * g.view(5, 7)) and bool((gs.flat[35:64] == 7.0).all())
    foreign = torch.full((100,), 0.5)
    ps[1].grad = foreign
    gs.accumulate(ps[1], torch.ones(100), **kw)
    assert ps[1].grad is foreign and torch.equal(foreign, torch.full((100,), 1.5)) and bool((gs.flat[64:192] == 7.0).all())
    assert gs.fused_checked == set() and gs._touched == []      # (fused here says checks=False; outside a scaled region nothing is registered)
    if fused:
        assert gs._unchecked == {0, 1}
