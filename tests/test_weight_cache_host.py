"""weights.WeightCache on the CPU: when a 16-bit operand copy is re-cast and when it is not.  The three cast entry points of `ops`
are replaced by torch restatements that record their calls, so every scenario asserts the casts issued and the tensors returned."""
import types

import pytest
import torch

from procedurevrl_amd import ops, weights

OP16 = ops.OP16


@pytest.fixture
def casts(monkeypatch):
    """-> list of recorded calls: ("one", w, need_t), ("multi", [(w, wants_t), ...]), ("pad", w)"""
    log = []

    def cast_weight(w, out=None, out_t=None, need_t=True):
        log.append(("one", w, need_t))
        out = torch.empty(w.shape, dtype=OP16) if out is None else out
        out.copy_(w)
        if need_t:
            out_t = torch.empty((w.shape[1], w.shape[0]), dtype=OP16) if out_t is None else out_t
            out_t.copy_(w.t())
        return out, (out_t if need_t else None)

    def cast_weights_multi(items):
        log.append(("multi", [(w, t is not None) for w, _, t in items]))
        for w, out, out_t in items:
            out.copy_(w)
            if out_t is not None:
                out_t.copy_(w.t())

    def cast_weight_pad(w, out, out_t, bias=None, out_b=None):
        log.append(("pad", w))
        N, K = w.shape
        out[:N, :K].copy_(w)
        out_t[:K, :N].copy_(w.t())
        if bias is not None:
            out_b[:N].copy_(bias.detach())

    monkeypatch.setattr(ops, "cast_weight", cast_weight)
    monkeypatch.setattr(ops, "cast_weights_multi", cast_weights_multi)
    monkeypatch.setattr(ops, "cast_weight_pad", cast_weight_pad)
    return log


def make(n=6, k=10, seed=0, requires_grad=True):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.Parameter(torch.randn(n, k, generator=g), requires_grad=requires_grad)


def cache():
    owner = types.SimpleNamespace(weights_epoch=0)
    return weights.WeightCache(owner), owner


def same(w, p):
    """the operands one recorded cast was given are the parameter's values"""
    return w.shape == (p.shape[0], p[0].numel()) and torch.equal(w, p.detach().reshape(p.shape[0], -1))


def check_values(e, p):
    w2 = p.detach().reshape(p.shape[0], -1)
    assert e.w.dtype == OP16 and torch.equal(e.w, w2.to(OP16))
    assert e.t.dtype == OP16 and torch.equal(e.t, w2.to(OP16).t())


def test_first_use_casts_once_then_nothing(casts):
    wc, _ = cache()
    p = make()
    e = wc.get(p)
    assert [c[0] for c in casts] == ["one"] and same(casts[0][1], p) and casts[0][2] is True
    check_values(e, p)
    assert wc.get(p) is e and wc.get(p, need_t=False) is e
    assert len(casts) == 1


def test_conv_weight_is_viewed_as_rows(casts):
    wc, _ = cache()
    p = torch.nn.Parameter(torch.randn(4, 3, 2, 2))
    e = wc.get(p, need_t=False)
    assert e.w.shape == (4, 12) and e.t is None and casts[0][2] is False
    assert torch.equal(e.w, p.detach().reshape(4, 12).to(OP16))


@pytest.mark.parametrize("change", ["version", "epoch", "data_ptr"])
def test_recast_keeps_the_buffers(casts, change):
    wc, owner = cache()
    p = make()
    e = wc.get(p)
    ptrs = (e.w.data_ptr(), e.t.data_ptr())
    with torch.no_grad():
        if change == "version":
            p.add_(0)
            p.data.mul_(2)          # (.data: new values under the version that add_ just advanced)
        elif change == "epoch":
            p.data.mul_(2)          # the fused optimiser's kind of update: no _version change
            assert wc.get(p) is e and len(casts) == 1
            owner.weights_epoch += 1
        else:
            p.data = p.data * 2
    e2 = wc.get(p)
    assert e2 is e and len(casts) == 2 and casts[1][0] == "one" and same(casts[1][1], p)
    assert (e.w.data_ptr(), e.t.data_ptr()) == ptrs
    check_values(e, p)
    wc.get(p)
    assert len(casts) == 2


def test_epoch_does_not_recast_a_frozen_parameter(casts):
    wc, owner = cache()
    p = make(requires_grad=False)
    wc.get(p)
    owner.weights_epoch += 1
    wc.get(p)
    wc.refresh([(p, True)])
    assert len(casts) == 1
    with torch.no_grad():
        p.add_(1)               # frozen parameters change through versioned in-place copies
    check_values(wc.get(p), p)
    assert len(casts) == 2


def test_refresh_casts_the_stale_ones_in_one_launch(casts):
    wc, owner = cache()
    ps = [make(seed=i) for i in range(4)]
    frozen = make(seed=9, requires_grad=False)
    plist = [(ps[0], True), (ps[1], False), (ps[2], True), (ps[3], True), (frozen, True)]
    wc.refresh(plist)
    assert len(casts) == 1 and casts[0][0] == "multi" and len(casts[0][1]) == 5
    assert [t for _, t in casts[0][1]] == [True, False, True, True, True]
    for p, need_t in plist:
        e = wc.peek(p)
        assert torch.equal(e.w, p.detach().to(OP16)) and ((e.t is None) if not need_t else torch.equal(e.t, p.detach().to(OP16).t()))
    wc.refresh(plist)
    assert len(casts) == 1                                  # all fresh: no launch
    ptrs = [(wc.peek(p).w.data_ptr(), wc.peek(p).t.data_ptr() if n else None) for p, n in plist]
    with torch.no_grad():
        ps[0].add_(1)
        ps[2].data = ps[2].data + 1
    wc.refresh(plist)
    assert len(casts) == 2 and casts[1][0] == "multi"
    assert len(casts[1][1]) == 2 and same(casts[1][1][0][0], ps[0]) and same(casts[1][1][1][0], ps[2])
    owner.weights_epoch += 1
    wc.refresh(plist)                                       # every trainable one, not the frozen one
    assert len(casts) == 3 and len(casts[2][1]) == 4 and not any(same(w, frozen) for w, _ in casts[2][1])
    wc.refresh(plist, force=True)
    assert len(casts) == 4 and len(casts[3][1]) == 5
    assert ptrs == [(wc.peek(p).w.data_ptr(), wc.peek(p).t.data_ptr() if n else None) for p, n in plist]
    for p, _ in plist:                                      # get() agrees that everything is current
        wc.get(p, need_t=wc.peek(p).t is not None)
    assert len(casts) == 4
    check_values(wc.get(ps[0]), ps[0])
    check_values(wc.get(ps[2]), ps[2])


def test_refresh_leaves_a_non_contiguous_view_to_get(casts):
    wc, _ = cache()
    base = make(10, 6)
    view = base.detach().t()                 # [6, 10], strides (1, 6)
    assert not view.is_contiguous()
    p = make()
    wc.refresh([(view, True), (p, True)])
    assert len(casts) == 1 and len(casts[0][1]) == 1 and same(casts[0][1][0][0], p)
    assert wc.peek(view).w is None
    e = wc.get(view)
    assert len(casts) == 2 and casts[1][0] == "one" and casts[1][1].is_contiguous()
    check_values(e, view)


def test_forward_capture_recasts_unless_just_refreshed(casts):
    wc, _ = cache()
    p = make()
    e = wc.get(p)
    ptrs = (e.w.data_ptr(), e.t.data_ptr())
    wc.get(p, force=True)                    # forward capture: a current entry is cast again, into the same tensors
    assert len(casts) == 2 and (e.w.data_ptr(), e.t.data_ptr()) == ptrs
    wc.refresh([(p, True)], force=True)      # forward capture behind the bulk refresh: the engine passes force=False
    wc.get(p, force=False)
    assert [c[0] for c in casts] == ["one", "one", "multi"]
    assert (e.w.data_ptr(), e.t.data_ptr()) == ptrs


def test_backward_capture_casts_nothing_and_needs_the_entry(casts):
    wc, owner = cache()
    p = make()
    e = wc.get(p)
    owner.weights_epoch += 1                 # stale by version: a backward capture still reuses what the forward graph cast
    assert wc.get(p, frozen=True) is e and len(casts) == 1
    with pytest.raises(AssertionError):
        wc.get(make(seed=3), frozen=True)
    q = make(seed=4)
    wc.get(q, need_t=False)
    with pytest.raises(AssertionError):
        wc.get(q, need_t=True, frozen=True)  # ... and the transposed copy, if it is what the backward reads
    assert wc.get(q, need_t=False, frozen=True) is wc.peek(q)


def test_transpose_asked_for_later_is_cast(casts):
    wc, _ = cache()
    p = make()
    e = wc.get(p, need_t=False)
    assert e.t is None
    ptr = e.w.data_ptr()
    assert wc.get(p, need_t=True) is e and len(casts) == 2 and casts[1][2] is True
    assert e.w.data_ptr() == ptr
    check_values(e, p)
    q = make(seed=5)
    wc.refresh([(q, False)])
    wc.refresh([(q, True)])
    assert [c[0] for c in casts[2:]] == ["multi", "multi"]
    check_values(wc.peek(q), q)


def test_derived_entries(casts):
    wc, _ = cache()
    p = make()
    assert wc.peek(p) is None and wc.peek(p, "fused_t") is None
    d = wc.entry(p, "fused_t")
    assert d.w is None and d.ver == -1 and wc.entry(p, "fused_t") is d and wc.peek(p, "fused_t") is d
    assert wc.peek(p) is None                # the derived entry is not the parameter's own
    assert wc.get(p) is not d and not any(c[0] != "one" for c in casts)


def test_padded(casts):
    wc, owner = cache()
    w, b = make(6, 10), torch.nn.Parameter(torch.randn(6))
    e = wc.padded(w, b)
    assert [c[0] for c in casts] == ["pad"] and same(casts[0][1], w)
    assert e.w.shape == (128, 128) and e.t.shape == (128, 128) and e.b.shape == (128,) and (e.N, e.K) == (6, 10)

    def check():
        want = torch.zeros(128, 128, dtype=OP16)
        want[:6, :10] = w.detach().to(OP16)
        wb = torch.zeros(128)
        wb[:6] = b.detach()
        assert torch.equal(e.w, want) and torch.equal(e.t, want.t()) and torch.equal(e.b, wb)
    check()
    assert wc.padded(w, b) is e and len(casts) == 1
    ptrs = (e.w.data_ptr(), e.t.data_ptr(), e.b.data_ptr())
    with torch.no_grad():
        b.add_(1)                            # the bias travels with the weight: its version counts
    assert wc.padded(w, b) is e and len(casts) == 2
    check()
    with torch.no_grad():
        w.add_(1)
    wc.padded(w, b)
    w.data.mul_(2)
    owner.weights_epoch += 1
    wc.padded(w, b)
    w.data = w.data * 2
    wc.padded(w, b)
    wc.padded(w, b, force=True)              # forward capture
    assert len(casts) == 6 and wc.padded(w, b) is e
    assert (e.w.data_ptr(), e.t.data_ptr(), e.b.data_ptr()) == ptrs
    check()
    assert wc.padded(w, b, frozen=True) is e and len(casts) == 6     # backward capture
    with pytest.raises(AssertionError):
        wc.padded(make(seed=2), frozen=True)
    e2 = wc.padded(w, b, Np=256, Kp=512, force=True)     # a re-cast at another padding: new buffers
    assert e2 is not e and e2.w.shape == (256, 512) and e2.t.shape == (512, 256) and len(casts) == 7
    assert torch.equal(e2.w[:6, :10], w.detach().to(OP16)) and float(e2.w.float().abs().sum()) == float(e2.w[:6, :10].float().abs().sum())
    nb = wc.padded(make(seed=7))             # no bias
    assert float(nb.b.abs().sum()) == 0.0


def test_engines_turn_their_capture_state_into_the_arguments(casts):
    """the capture policy lives in the engines: what each passes for its `_capturing` / `_refreshed`, `_cap` / `_cap_seen`"""
    from procedurevrl_amd.engine import EncoderEngine
    from procedurevrl_amd.head_engine import PretrainHeadEngine
    from procedurevrl_amd.mvit import MViTEngine
    wc, owner = cache()
    owner.weights = wc
    p = make()
    eng = EncoderEngine.__new__(EncoderEngine)
    eng.weights = wc
    e = eng._weight(p)
    eng._weight(p)
    assert len(casts) == 1
    eng._capturing = "fwd"                   # forward capture: re-cast a current entry ...
    eng._weight(p)
    assert len(casts) == 2
    eng._refreshed = True                    # ... unless the bulk refresh of this forward has just run
    eng._weight(p)
    assert len(casts) == 2
    eng._capturing, eng._refreshed = "bwd", False
    owner.weights_epoch += 1
    assert eng._weight(p) is e and len(casts) == 2
    with pytest.raises(AssertionError):
        eng._weight(make(seed=1))

    head = PretrainHeadEngine(owner)
    q = make(seed=2)
    head._wc(q)
    head._wc(q)
    assert len(casts) == 3
    head._cap, head._cap_seen = "fwd", set()
    assert head._wc(q) is wc.peek(q) and len(casts) == 4         # forced once per parameter per forward capture
    head._wc(q)
    assert len(casts) == 4
    head._cap = "bwd"                        # the head's backward capture finds the versions current
    head._wc(q)
    assert len(casts) == 4

    mv = MViTEngine.__new__(MViTEngine)
    mv.weights = wc
    w = make(seed=3)
    pe = mv._wpad(w)
    mv._wpad(w)
    assert [c[0] for c in casts[4:]] == ["pad"]
    mv._capturing = "fwd"
    mv._wpad(w)
    mv._wpad(w)                              # every use inside a forward capture
    assert [c[0] for c in casts[4:]] == ["pad"] * 3
    mv._capturing = "bwd"
    owner.weights_epoch += 1
    assert mv._wpad(w) is pe and len(casts) == 7
    with pytest.raises(AssertionError):
        mv._wpad(make(seed=4))
