"""16-bit operand copies of the fp32 master weights and the ONE rule for when a copy is current.  One WeightCache
per model wrapper (`model.weights`, next to `weights_epoch`), handed to the engines.  It knows nothing of HIP graphs; a capturing engine
passes `force` (forward capture: re-cast whatever the version says, so that a replay refreshes the copies after an optimiser step) or
`frozen` (backward capture: hand back, untouched, what the forward graph of the same step cast)."""
import torch

from . import ops


class _W:
    """bf16 operand copies of one weight matrix: `w` = [N, K] for forward, `t` = [K, N] for the data gradient
    (`be`, fused temporal map only: fp32 [N] bias W_fc b_proj)."""
    __slots__ = ("w", "t", "ver", "be")

    def __init__(self):
        self.w = self.t = self.be = None
        self.ver = -1


class _PW:
    """zero-padded bf16 operand copies of one weight: w [Np, Kp] (forward), t [Kp, Np] (data gradient), bias [Np] fp32"""
    __slots__ = ("w", "t", "b", "ver", "N", "K")


def _fresh(e, p, ver, need_t):
    return e.ver == ver and e.w is not None and e.w.device == p.device and (e.t is not None or not need_t)


class WeightCache:
    def __init__(self, owner):
        self.owner = owner      # the model wrapper: `weights_epoch`
        self._w = {}
        self._pw = {}

    def _version(self, p):
        # the fused optimiser updates trainable parameters through its flat buffer (no _version bump) and advances weights_epoch
        # instead; frozen parameters (text tower) only change through versioned in-place copies; a new data_ptr(): the parameter moved
        return (p._version, getattr(self.owner, "weights_epoch", 0) if p.requires_grad else 0, p.data_ptr())

    def peek(self, p, tag=None):
        """the entry of parameter `p`, or None; `tag`: an entry DERIVED from `p` that its user fills and versions (fused temporal map)"""
        return self._w.get(id(p) if tag is None else (tag, id(p)))

    def entry(self, p, tag=None):
        """... created empty on first use"""
        e = self.peek(p, tag)
        if e is None:
            e = self._w[id(p) if tag is None else (tag, id(p))] = _W()
        return e

    def get(self, p, need_t=True, force=False, frozen=False):
        """-> the current copies of `p` viewed as [shape[0], -1]: `.w` and, with `need_t`, `.t`.  A re-cast on the same device writes
        into the tensors the entry already has: captured graphs have those addresses baked in."""
        if frozen:
            e = self.peek(p)
            assert e is not None and e.w is not None and (e.t is not None or not need_t)
            return e
        e, ver = self.entry(p), self._version(p)
        if force or not _fresh(e, p, ver, need_t):
            w2 = p.detach().reshape(p.shape[0], -1).contiguous()
            same = e.w is not None and e.w.device == p.device
            e.w, t = ops.cast_weight(w2, out=e.w if same else None, out_t=e.t if same else None, need_t=need_t)
            if need_t:
                e.t = t
            e.ver = ver
        return e

    def refresh(self, plist, force=False):
        """the stale ones -- with `force`, all -- of the (parameter, transposed copy wanted) pairs in ONE launch instead of one per matrix
        on first use; none when nothing is stale.  Non-contiguous views are left to get()."""
        todo = []
        for p, need_t in plist:
            e, ver = self.entry(p), self._version(p)
            if _fresh(e, p, ver, need_t) and not force:
                continue
            w2 = p.detach().reshape(p.shape[0], -1)
            if not w2.is_contiguous():
                continue
            if e.w is None or e.w.device != p.device:
                e.w, e.t = torch.empty(w2.shape, device=p.device, dtype=ops.OP16), None
            if need_t and e.t is None:
                e.t = torch.empty((w2.shape[1], w2.shape[0]), device=p.device, dtype=ops.OP16)
            todo.append((w2, e.w, e.t if need_t else None, e, ver))
        if todo:
            ops.cast_weights_multi([(w2, w, t) for w2, w, t, _, _ in todo])
            for _, _, _, e, ver in todo:
                e.ver = ver

    def padded(self, weight, bias=None, Np=None, Kp=None, force=False, frozen=False):
        """-> _PW: `weight` [N, K] / `bias` [N] zero-padded to [Np, Kp] / [Np] (default: multiples of 128; MViT's widths are no tile
        multiples).  The version covers the bias too, and `weights_epoch` whether or not the weight is trainable."""
        e = self._pw.get(id(weight))
        if frozen:
            assert e is not None
            return e
        ver = (weight._version, bias._version if bias is not None else -1, getattr(self.owner, "weights_epoch", 0), weight.data_ptr())
        if force or e is None or e.ver != ver or e.w.device != weight.device:
            w2 = weight.detach().reshape(weight.shape[0], -1).contiguous()
            N, K = w2.shape
            Np, Kp = -(-N // 128) * 128 if Np is None else Np, -(-K // 128) * 128 if Kp is None else Kp
            if e is None or e.w.device != weight.device or tuple(e.w.shape) != (Np, Kp):
                e = self._pw[id(weight)] = _PW()
                e.w, e.t = (torch.zeros(s, device=weight.device, dtype=ops.OP16) for s in ((Np, Kp), (Kp, Np)))
                e.b = torch.zeros(Np, device=weight.device, dtype=torch.float32)
            ops.cast_weight_pad(w2, e.w, e.t, bias, e.b)
            e.N, e.K, e.ver = N, K, ver
        return e
