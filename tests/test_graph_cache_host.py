"""graphs.GraphCache on the host: its capture primitive `_capture` -- the one seam that touches torch.cuda -- is replaced by a stub that
runs the function and hands back a fake graph with a replay counter."""
import warnings

import pytest
import torch

from procedurevrl_amd.graphs import GraphCache, GraphOwner


class FakeGraph:
    def __init__(self):
        self.replays = 0

    def replay(self):
        self.replays += 1


class Owner(GraphOwner):
    """the protocol of every user: look the key up, replay the entry or run eagerly"""

    def __init__(self, **kw):
        self._gcache = GraphCache(self, "the test owner", **kw)
        self._gcache._capture = self.stub
        self.pools, self.markers, self.resets = [], [], 0
        self.fail = None

    def stub(self, fn):
        gc = self._gcache
        if gc.shared_pool and gc.pool is None:
            gc.pool = object()
        self.pools.append(gc.pool)
        return FakeGraph(), fn()

    def body(self, what):
        self.markers.append(self._capturing)
        if self.fail is not None:
            raise self.fail
        return what

    def _graph_reset_host_state(self):
        self.resets += 1

    def call(self, key):
        """-> "eager" / "capture" / "replay": what this call of `key` did"""
        made = []

        def make():
            made.append(1)
            graph, out = self._gcache.capture("fwd", lambda: self.body("out"))
            return dict(fwd=graph, out=out)
        g = self._gcache.entry(key, make)
        if g is None:
            return "capture failed" if made else "eager"
        g["fwd"].replay()
        return "capture" if made else "replay"


@pytest.mark.parametrize("max_keys", [1, 2])
def test_policy_table(max_keys):
    o = Owner(warmup=2, max_keys=max_keys)
    assert [o.call("a") for _ in range(5)] == ["eager", "eager", "capture", "replay", "replay"]
    assert o._gseen == {"a": 3} and list(o._graphs) == ["a"] and o._graphs["a"]["fwd"].replays == 3
    seen = dict(o._gseen)
    o.call("a")
    assert o._gseen == seen                  # a sighting is counted only while there is no entry
    second = [o.call("b") for _ in range(5)]
    if max_keys == 1:                        # the cap is reached: eager for ever, whatever the count says
        assert second == ["eager"] * 5 and list(o._graphs) == ["a"] and o._gseen["b"] == 5
    else:
        assert second == ["eager", "eager", "capture", "replay", "replay"] and len(o._graphs) == 2
        assert [o.call("c") for _ in range(4)] == ["eager"] * 4
    assert o.call("a") == "replay"
    assert o.markers == ["fwd"] * len(o._graphs) and o._capturing is None


def test_defaults_are_todays_values():
    from procedurevrl_amd.engine import GraphReplay
    from procedurevrl_amd.head_engine import PretrainHeadEngine
    gc = GraphCache(Owner(), "x")
    assert (gc.warmup, gc.max_keys, gc.shared_pool) == (2, 4, True)
    assert (GraphReplay.GRAPH_WARMUP, GraphReplay.GRAPH_MAX_KEYS) == (2, 4)
    assert (PretrainHeadEngine.GRAPH_WARMUP, PretrainHeadEngine.GRAPH_MAX_KEYS) == (2, 2)


def test_switch_off(monkeypatch):
    monkeypatch.delenv("PVRL_HIP_GRAPHS", raising=False)
    o = Owner()
    assert o.use_graphs
    o.use_graphs = False                     # the attribute every engine forwards to its cache
    assert not o._gcache.enabled
    assert [o.call("a") for _ in range(4)] == ["eager"] * 4
    assert o._gseen == {} and o._graphs == {} and o.markers == []
    monkeypatch.setenv("PVRL_HIP_GRAPHS", "0")
    o = Owner()
    assert not o.use_graphs
    assert [o.call("a") for _ in range(4)] == ["eager"] * 4
    assert o._gseen == {} and o._graphs == {} and o.markers == []
    monkeypatch.setenv("PVRL_HIP_GRAPHS", "1")
    assert Owner().use_graphs


def test_failed_capture():
    o = Owner(warmup=1)
    assert [o.call("a"), o.call("a"), o.call("b")] == ["eager", "capture", "eager"]
    o.fail = RuntimeError("injected")
    o._gkey = "a"
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        assert o.call("b") == "capture failed"
        assert o.call("b") == "eager" and o.call("a") == "eager"
    assert len(wlist) == 1
    text = str(wlist[0].message)
    assert "capture" in text and "the test owner" in text and "forward" in text and "injected" in text
    assert not o.use_graphs and o._graphs == {} and o.resets == 1 and o._capturing is None
    assert o._gkey is None and o._gcache.pool is None
    assert o.markers == ["fwd", "fwd"]       # nothing was captured after the failure


def test_failed_backward_capture_names_the_pass():
    o = Owner()
    o.fail = ValueError("no")
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        assert o._gcache.attempt("backward", lambda: o._gcache.capture("bwd", lambda: o.body(1))) is None
    assert len(wlist) == 1 and "capture" in str(wlist[0].message) and "backward" in str(wlist[0].message)
    assert o.markers == ["bwd"] and o._capturing is None and not o.use_graphs and o.resets == 1


@pytest.mark.parametrize("what", ["fwd", "bwd"])
def test_marker(what):
    o = Owner()
    graph, out = o._gcache.capture(what, lambda: o.body(7))
    assert isinstance(graph, FakeGraph) and out == 7
    assert o.markers == [what] and o._capturing is None
    o.fail = KeyError("x")
    with pytest.raises(KeyError):
        o._gcache.capture(what, lambda: o.body(7))
    assert o.markers == [what, what] and o._capturing is None
    assert Owner._capturing is None          # the class-level default: engines built with __new__ read it


def test_pool_is_lazy_and_shared_unless_switched_off():
    o = Owner(warmup=0)
    assert o._gcache.pool is None
    o.call("a"), o.call("b")
    assert o.pools[0] is not None and o.pools[0] is o.pools[1] is o._gcache.pool
    o = Owner(warmup=0, shared_pool=False)   # the text tower: captured on a side stream, no `pool=`
    o.call("a"), o.call("b")
    assert o.pools == [None, None] and o._gcache.pool is None


def test_grad_undo_and_install():
    ps = [torch.nn.Parameter(torch.zeros(3)) for _ in range(3)]
    o = Owner()
    g0, g2 = torch.ones(3), torch.full((3,), 2.0)

    def backward():
        ps[0].grad, ps[2].grad = g0, g2
    o._gcache.capture("bwd", backward)
    grads = o._gcache.take_grads(ps)
    assert all(p.grad is None for p in ps)
    o._gcache.install_grads(grads)
    assert ps[0].grad is g0 and ps[1].grad is None and ps[2].grad is g2


def test_release():
    o = Owner(warmup=0)
    o.release_graphs()                       # never captured
    assert o._graphs == {} and o._gkey is None and o._gcache.pool is None
    o.call("a")
    o._gkey = "a"
    entries = o._graphs
    assert len(entries) == 1 and o._gcache.pool is not None
    o.release_graphs()
    assert entries == {} and o._graphs is entries and o._gkey is None and o._gcache.pool is None
    o.release_graphs()
    assert o._graphs == {} and o.use_graphs
    assert o.call("a") == "capture"          # a released cache is still switched on and keeps its sighting counts


def test_engine_names_stay_importable():
    from procedurevrl_amd import engine, graphs
    assert engine.GraphReplay is graphs.GraphReplay and engine.drop_graphs_quietly is graphs.drop_graphs_quietly
    held = {1: FakeGraph()}
    graphs.drop_graphs_quietly(held)
    assert held == {}
