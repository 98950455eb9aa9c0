"""HIP-graph capture and replay, once for every user (`GraphReplay`: EncoderEngine and MViTEngine; head_engine.PretrainHeadEngine;
tfm_model.ClipTextModel).  `GraphCache` is the generic protocol -- when a key is captured, how a capture is made on this runtime, what a
failed capture does, how graphs are let go; a user keeps its key, its static input / output buffers and what a replay hands back."""
import os
import warnings

import torch


def _idle(empty_cache=False):
    try:
        if torch.cuda.is_available():
            torch.cuda.synchronize()
            if empty_cache:
                torch.cuda.empty_cache()
    except Exception:
        pass


def drop_graphs_quietly(graphs):
    """clear a dict / list that holds captured HIP graphs, with the device idle (see GraphCache.release)"""
    if graphs:
        _idle()
        graphs.clear()
        _idle(empty_cache=True)     # their memory pool goes back NOW, still with the device idle, not whenever the allocator next trims


class GraphCache:
    """The captured graphs of one owner: `entries[key]` is whatever the owner's capture built (graphs, static buffers).

    Policy: a key runs eagerly while it has been seen fewer than `warmup` times (lazy workspaces / caches settle) or while `max_keys`
    entries exist; a sighting is counted only while the key has no entry.  `enabled` is the switch (PVRL_HIP_GRAPHS=0: off).
    While a capture runs, `owner._capturing` is "fwd" / "bwd" (the owner's weight-copy policy reads it).  Graphs of one cache share a
    memory pool -- the activations a forward graph saves are its backward graph's inputs -- unless `shared_pool` is off."""

    def __init__(self, owner, name, warmup=2, max_keys=4, shared_pool=True):
        self.owner, self.name = owner, name       # a GraphOwner; `name`: the owner in a warning's words
        self.enabled = os.environ.get("PVRL_HIP_GRAPHS", "1") == "1"
        self.warmup, self.max_keys = warmup, max_keys
        self.shared_pool = shared_pool
        self.entries, self.seen = {}, {}
        self.key = None             # the entry the owner's last forward replayed (its backward replays the same one)
        self.pool = None

    def entry(self, key, make):
        """-> the entry to replay -- captured now by `make()` when this is the call for it -- or None: run eagerly this time"""
        if not self.enabled:
            return None
        g = self.entries.get(key)
        if g is None:
            n = self.seen.get(key, 0)
            self.seen[key] = n + 1
            if n < self.warmup or len(self.entries) >= self.max_keys:
                return None
            g = self.attempt("forward", make)
            if g is not None:
                self.entries[key] = g
        return g

    def attempt(self, what, make):
        """-> make(), or None after it raised: a failed capture is never fatal, the eager launch sequence is the same kernels"""
        try:
            return make()
        except Exception as e:
            self.failed(what, e)
            return None

    def failed(self, what, e):
        warnings.warn(f"HIP graph capture of {self.name} {what} failed ({type(e).__name__}: {e}); continuing with eager launches")
        self.enabled = False
        self.owner._capturing = None
        self.release()
        self.owner._graph_reset_host_state()
        _idle()

    def capture(self, what, fn):
        """-> (graph, fn()): the launches of fn() as one HIP graph; `what`: "fwd" / "bwd" """
        self.owner._capturing = what
        try:
            return self._capture(fn)
        finally:
            self.owner._capturing = None

    def _capture(self, fn):
        if self.shared_pool and self.pool is None:
            self.pool = torch.cuda.graph_pool_handle()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, pool=self.pool, capture_error_mode="thread_local"):
            out = fn()
        return graph, out

    # A backward capture runs no kernel but leaves `p.grad` set on the host: taken off after the capture, put back at every replay.
    @staticmethod
    def take_grads(params):
        grads = [(p, p.grad) for p in params if p.grad is not None]
        for p, _ in grads:
            p.grad = None
        return grads

    @staticmethod
    def install_grads(grads):
        for p, v in grads:
            p.grad = v

    def release(self):
        """Drop every captured graph (and give their memory pool back) WITH THE DEVICE IDLE -- call it, then `gc.collect()`, before a
        long-lived process lets go of a model it has trained.  Round 6: with the MViT tests in front, the train-loop tests aborted or
        hung inside the HIP runtime (ROCm 7.2, no message) in 3 of 4 runs: the dead models' ~20 captured graphs and their pools were
        being torn down by Python's cyclic garbage collector at arbitrary points of the NEXT model's steps.  Releasing every test's GPU
        objects at a quiet point between tests (tests/conftest.py) removed it (5 of 5); doing the same from a `__del__` did not (3 of 6
        still failed: the collector still picks the moment), so there is no destructor hook."""
        drop_graphs_quietly(self.entries)
        self.key = None
        self.pool = None


def _cached(name):
    return property(lambda self: getattr(self._gcache, name), lambda self, v: setattr(self._gcache, name, v))


class GraphOwner:
    """What callers reach for on anything that replays graphs, forwarded to its GraphCache `self._gcache`."""
    _capturing = None           # "fwd" / "bwd" while a HIP graph of that pass is being captured (GraphCache.capture)
    use_graphs = _cached("enabled")
    _graphs = _cached("entries")
    _gseen = _cached("seen")
    _gkey = _cached("key")

    def release_graphs(self):       # (GraphCache.release)
        self._gcache.release()

    def _graph_reset_host_state(self):
        """a capture failed, possibly half way through a step: forget what the owner keeps on the host between launches"""


class GraphReplay(GraphOwner):
    """HIP-graph replay of an encoder engine's training / inference step.

    One training step of the encoder is ~1,400 kernel launches (~7 ms of Python on an idle host, several times that
    when the node's cores are contended -- measured up to 95 ms, more than the 57 ms the GPU needs).  The launch
    sequence of a given (shape, mode) never changes, so it is captured once and replayed: forward and backward are one
    graph each (backward: one per group of blocks when a data-parallel gradient hook is installed and the engine has staged
    backward).  What a replay cannot express falls back to the eager path: pinned DropPath draws, DecodedClips inputs,
    gradient accumulation into existing .grad tensors.

    The engine provides: _eager_forward(frames, training, save), _eager_backward(dfeat), _graph_key(frames, training,
    save), _enc_params() (the parameters whose gradients backward writes), `saved`, `grad_hook`, and consults
    `self._capturing` ("fwd": refresh every weight copy inside the graph, "bwd": reuse them).  Optional: _bwd_begin /
    _bwd_block / _bwd_end for staged capture.
    """
    GRAPH_WARMUP = 2      # eager calls of a key before it is captured
    GRAPH_MAX_KEYS = 4    # captured (shape, mode) combinations kept; others run eagerly
    _staged = False       # ... the backward as one graph per block (a gradient hook runs between the replays)
    _refreshed = False    # EncoderEngine: every weight copy was just rebuilt by _refresh_weights()

    def _graph_init(self):
        self._gcache = GraphCache(self, "the encoder", self.GRAPH_WARMUP, self.GRAPH_MAX_KEYS)

    grad_hook_group = None      # optional: the hook for a list of blocks at once (distributed.GradReducer merges their all-reduces)

    def _group_of(self, i, nb):
        """-> (lo, hi): the blocks [lo, hi] whose gradient hook runs together with block i's (`hook_group` blocks per group: fewer,
        larger collectives).  The LAST group of a backward -- blocks 0 .. hook_group - 1 -- runs per block (PVRL_HOOK_TAIL_SPLIT=0:
        A/B): nothing is left to overlap its collective with but the embedding stage, so the exposed tail round stays one block's
        ~45 MB instead of three blocks' ~135 MB."""
        grp = max(1, int(getattr(self, "hook_group", 1)))
        if i < grp and getattr(self, "hook_tail_split", True):
            return i, i
        lo = (i // grp) * grp
        return lo, min(lo + grp, nb) - 1

    def _run_hooks(self, blocks):
        if not blocks or self.grad_hook is None:
            return
        if self.grad_hook_group is not None and len(blocks) > 1:
            self.grad_hook_group(list(blocks))
        else:
            for j in blocks:
                self.grad_hook(j)

    def _bwd_group_end(self, state):
        """staged backward: a group of blocks is done -- an engine that defers work of its blocks finishes it here (default: nothing)"""

    def join_side_stream(self):
        """Callers that drive a backward stage by stage call this before reading its results.  Every engine issues all of its
        work on the current stream, so there is nothing to wait for."""

    @staticmethod
    def _saved_copy(saved):
        """backward() consumes its `saved` dict (frees block entries as it goes): replays hand it a shallow copy"""
        sv = dict(saved)
        sv["blocks"] = list(saved["blocks"])
        return sv

    def _graph_forward(self, frames, training, save):
        key = self._graph_key(frames, training, save)
        g = self._gcache.entry(key, lambda: self._capture_forward(frames, training, save))
        if g is None:
            self._gkey = None
            return self._eager_forward(frames, training, save)
        g["frames"].copy_(frames)
        g["fwd"].replay()
        self.saved = g["saved"]
        self._gkey = key if save else None
        return g["feat"].clone()        # the graph's own output buffer is overwritten by the next replay

    def _capture_forward(self, frames, training, save):
        st = torch.empty_like(frames)
        st.copy_(frames)
        graph, feat = self._gcache.capture("fwd", lambda: self._eager_forward(st, training, save))
        return dict(fwd=graph, frames=st, feat=feat, saved=self.saved if save else None)

    def _grads_fresh(self):
        return all(p.grad is None for p in self._enc_params())

    def _graph_backward(self, dfeat):
        g = self._graphs[self._gkey]
        gb = None
        if self._grads_fresh() and (self.grad_hook is None or hasattr(self, "_bwd_begin")):
            staged = self.grad_hook is not None         # cut the graph where the data-parallel reducer hooks in
            slot = "bwd_staged" if staged else "bwd"
            if g.get(slot) is None:
                g[slot] = self._capture_backward(g, staged, dfeat)
            gb = g[slot]
        if gb is None:
            # accumulation into existing gradients (beta = 1 launches), a hook this engine cannot stage, or a capture that just failed
            # (graphs are off now): eager launches
            self.saved = self._saved_copy(g["saved"])
            self._gkey = None
            return self._eager_backward(dfeat)
        gb["dfeat"].copy_(dfeat)
        self._gcache.install_grads(gb["touched"])     # before the hooks run: the reducer treats a parameter without .grad as unused
        for graph, blocks in gb["graphs"]:
            graph.replay()
            self._run_hooks(blocks)     # (staged: the blocks this graph finished, last block first)
        self.saved = None
        self._gkey = None

    def _capture_backward(self, g, staged, dfeat):
        """-> the captured graph(s) of g's backward with their static input, or None after a failed capture"""
        gc = self._gcache
        st_in = torch.empty_like(dfeat.contiguous())
        st_in.copy_(dfeat)
        nb = len(g["saved"]["blocks"])
        graphs = []

        def group(i, lo, state):
            if state is None:
                state = self._bwd_begin(st_in)
            for j in range(i, lo - 1, -1):
                self._bwd_block(state, j)
            self._bwd_group_end(state)
            if lo == 0:
                self._bwd_end(state)
            return state

        def capture():
            self.saved = self._saved_copy(g["saved"])
            if not staged:
                graphs.append((gc.capture("bwd", lambda: self._eager_backward(st_in))[0], []))
                return True
            # one graph per GROUP of `hook_group` blocks (the first also holds the final-norm stage, the last the embedding stage):
            # the hook runs for a group's blocks after its replay
            state, i = None, nb - 1
            while i >= 0:
                lo = self._group_of(i, nb)[0]
                graph, state = gc.capture("bwd", lambda: group(i, lo, state))
                graphs.append((graph, list(range(i, lo - 1, -1))))
                i = lo - 1
            return True

        hook, self.grad_hook = self.grad_hook, None
        self._staged = staged          # the hook is detached while capturing: a stage must still finish its block's gradients itself
        try:
            ok = gc.attempt("backward", capture)
        finally:
            self._staged = False
            self.grad_hook = hook
        touched = gc.take_grads(self._enc_params())       # all were None (_grads_fresh)
        return dict(graphs=graphs, dfeat=st_in, touched=touched) if ok else None
