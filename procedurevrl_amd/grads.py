"""The flat gradient buffer every engine writes into (`GradStore`) and the switch that says whether engines scale their internal
gradients (`SCALED_GRADS`): the third service the engines share, next to graphs.GraphCache and weights.WeightCache.  Runs on the
CPU as well (tests/test_grad_store_host.py): only `begin_scaled`'s one-launch branch needs the HIP library."""
import torch

from . import ops
from ._lib import lib

F32 = torch.float32
SCALED_GRADS = ops.OP16 == torch.float16     # fp16-operand flavour: engines scale their internal gradients (GradStore.begin_scaled)


class GradStore:
    """Flat fp32 gradient buffer; every trainable parameter's .grad is a view into it so the
    data-parallel all-reduce works on large contiguous chunks (reference: DDP buckets,
    lib/models/build.py:49-53)."""

    def __init__(self, named_params, device):
        self.names = [n for n, _ in named_params]
        self.params = [p for _, p in named_params]
        sizes = [p.numel() for p in self.params]
        # 64-element alignment keeps every view 256-byte aligned
        self.offsets = []
        off = 0
        for s in sizes:
            self.offsets.append(off)
            off += (s + 63) // 64 * 64
        self.end = off                     # end of the parameter gradients
        # tail: one float per parameter, "this rank produced a gradient for it" -- summed over ranks inside the last
        # chunk of the data-parallel all-reduce (distributed.GradReducer, DDP's find_unused_parameters bookkeeping) -- and one
        # control slot behind them ("a rank asks for a re-synchronisation of the replicas", GradReducer find_unused="cached")
        # ... and behind it `bad`, the optimiser's "skip this step" flag (csrc/optim.hip): raised on the device by the kernels that
        # write parameter gradients when a value is inf / nan and by the training loop when a loss is; summed over ranks with the
        # rest of the tail, so every replica drops the same step (misc.check_nan_losses, tools/train_net.py:174)
        self.flat = torch.zeros(off + (len(sizes) + 2 + 63) // 64 * 64, device=device, dtype=F32)
        self.used = self.flat[off:off + len(sizes)]
        self.ctl = self.flat[off + len(sizes):off + len(sizes) + 1]
        self.bad = self.flat[off + len(sizes) + 1:off + len(sizes) + 2]
        self.fused_checked = set()     # parameters whose gradient producers raise `bad` themselves (target(..., fused=True))
        self._unchecked = set()        # ... parameters with at least one writer that does not (target(..., checks=False))
        self.reduced_over_ranks = False   # set by distributed.GradReducer.finish(): the buffer holds SUMS over ranks (the optimiser then scans all of it)
        self.views = [self.flat[o:o + s].view(p.shape) for o, s, p in zip(self.offsets, sizes, self.params)]
        self.index = {id(p): i for i, p in enumerate(self.params)}
        self.scale = None       # fp16 flavour: device scalar S while an engine's backward runs with S-scaled gradients
        self.inv = None         # ... and 1 / S: the `gscale` of the kernels that write parameter gradients (include/pvrl.h)
        self._touched = []
        self._zeroed = set()    # ... parameters prezero() cleared inside the scaled region and no target() has handed out since

    def span(self, i):
        """[a, b) of parameter i in the flat buffer, padding included"""
        return self.offsets[i], (self.offsets[i + 1] if i + 1 < len(self.offsets) else self.end)

    def _runs(self, idx):
        """sorted parameter indices -> the contiguous [a, b) runs of the flat buffer their spans form"""
        runs = []
        for i in idx:
            a, b = self.span(i)
            if runs and runs[-1][1] == a:
                runs[-1][1] = b
            else:
                runs.append([a, b])
        return runs

    def target(self, p, fused=False, checks=True):
        """-> (grad tensor to write into, beta).  beta = 0 overwrites, 1 accumulates.
        `fused`: the caller's kernel computes  grad = beta * grad + self.inv * (its S-scaled result)  itself (`gscale`): nothing is
        registered for unscale(), what is already there stays in true units.  `checks` (with `fused`): that kernel also raises `self.bad`
        on a non-finite value it writes (`nonfinite`), so the optimiser's scan may skip the parameter (`fused_checked`); a writer that
        takes no `nonfinite` argument says checks=False and its parameter stays in the scan."""
        i = self.index[id(p)]
        v = self.views[i]
        self._zeroed.discard(i)
        if p.grad is None:
            p.grad = v
            t, beta = v, 0.0
        elif p.grad.data_ptr() == v.data_ptr():
            t, beta = v, 1.0
        else:       # a foreign .grad tensor (someone else allocated it): accumulate into it
            t, beta = p.grad, 1.0
        if fused:
            if not checks:                       # one unchecked writer is enough to keep the parameter in the scan, whatever the order
                self._unchecked.add(i)
                self.fused_checked.discard(i)
            elif t is v and i not in self._unchecked:
                self.fused_checked.add(i)
            return t, beta
        if self.scale is not None:
            key = i if t is v else t
            seen = self._seen_idx if t is v else self._seen_ptr
            tag = i if t is v else t.data_ptr()
            if tag not in seen:
                seen.add(tag)
                if beta == 1.0:
                    t.mul_(self.scale)      # what is already there joins the S-scaled units until the engine is done
            self._touched.append(key)
        return t, beta

    def accumulate(self, p, g, fused=False, checks=True):
        """p.grad = g (first touch) or p.grad += g, with torch ops; `fused` / `checks` as in target().  A `fused` caller passes g in
        true units, and says checks=False: copy_ / add_ raise no flag"""
        t, beta = self.target(p, fused, checks)
        if beta == 0.0:
            t.copy_(g.view_as(t))
        else:
            t.add_(g.view_as(t))

    def prezero(self, params):
        """An engine that is about to ACCUMULATE into every one of `params` (atomics / beta = 1 kernels): the ones without a
        gradient yet get their zeroed view now, contiguous runs of the flat buffer in one fill each, instead of one small
        fill per parameter at its first use.  Only for parameters the caller is certain to write: .grad stops being None."""
        idx = sorted(self.index[id(p)] for p in params if p.grad is None and id(p) in self.index)
        for a, b in self._runs(idx):
            self.flat[a:b].zero_()
        for i in idx:
            self.params[i].grad = self.views[i]
            if self.scale is not None:           # zeros need no conversion to S-scaled units, but are unscaled with the rest
                self._seen_idx.add(i)
                self._zeroed.add(i)
                self._touched.append(i)

    # ---- fp16-operand flavour: gradient scaling inside an engine's backward -------------------------------------------
    # fp16 has 5 exponent bits: the 16-bit gradient operands of the backward GEMMs (rms 1e-6 .. 1e-4 at the benchmark
    # shapes) would underflow.  An engine therefore multiplies the gradient it receives by a power of two S, chosen on the
    # DEVICE from that gradient's magnitude (no host sync, capturable in a HIP graph), runs its whole backward in S-scaled
    # units -- exact in fp32, and the 16-bit operands sit mid-range -- and multiplies every parameter gradient it produced
    # by 1/S before anyone outside the engine sees it.  Nothing outside the engine ever holds a scaled value.
    # S * max|incoming gradient|.  The only internal 16-bit operand that can outgrow it is an S-scaled SUM OVER ROWS: dW_e of the encoder's
    # fused temporal map (engine._temporal_chain_all).  Measured headroom below fp16's 65,504 (tests/test_grad_scale_gpu.py):
    # cls path ~100 x; all-token gradients at 288 rows 57 x (N(0,1)) / 8 x (mean-pooled), at 50,176 rows 4.8 x / 0.27 x -- so under an
    # all-token gradient the dW_e copies carry a power of two of their own and enter the cast 2.2 x below.
    SCALE_TARGET = 256.0

    def begin_scaled(self, g):
        """g: the fp32 gradient entering the engine -> g * S; registers S for target() / unscale()"""
        # a non-finite incoming gradient (amax = inf / nan) must not turn S into 0 and 1/S into inf: S stays a finite power
        # of two, so the non-finite values flow through to the loss check (train_epoch) instead of poisoning gradients
        # accumulated by earlier micro-iterations
        self._touched, self._seen_idx, self._seen_ptr, self._zeroed = [], set(), set(), set()
        g = g.detach()
        if g.is_cuda and g.dtype == F32 and g.is_contiguous() and g.numel() <= (1 << 20):      # one launch (csrc/optim.hip)
            out = torch.empty_like(g)
            self.scale = torch.empty(1, device=g.device, dtype=F32)
            self.inv_row = torch.empty(4096, device=g.device, dtype=F32)       # 1 / S, also as a GEMM epilogue's per-row scale
            self.inv = self.inv_row[:1]
            lib().call("pvrl_grad_scale_begin", ops._ptr(g), g.numel(), float(self.SCALE_TARGET), ops._ptr(out), ops._ptr(self.scale),
                       ops._ptr(self.inv_row), 4096, ops._stream())
            return out
        amax = torch.nan_to_num(g.abs().max(), nan=1.0, posinf=3e38).clamp(1e-30, 3e38)
        self.scale = torch.exp2(torch.floor(torch.log2(self.SCALE_TARGET / amax)).clamp(-100.0, 100.0)).reshape(1)
        self.inv = 1.0 / self.scale
        self.inv_row = self.inv.expand(4096).contiguous()      # 1 / S as a GEMM epilogue's per-row scale (EncoderEngine._temporal_chain_all)
        return g * self.scale

    def unscale(self):
        """multiply every gradient written since the last call by 1/S (contiguous runs of the flat buffer in one op each)"""
        if self.scale is None or not self._touched:
            return
        inv = self.inv
        for a, b in self._runs(sorted(set(k for k in self._touched if isinstance(k, int)))):
            self.flat[a:b].mul_(inv)
        done = set()
        for k in self._touched:
            if not isinstance(k, int) and k.data_ptr() not in done:
                done.add(k.data_ptr())
                k.mul_(inv)
        # they are in true units again: the first touch of a later writer brings what is there back into S-scaled units (target()),
        # except the zeros of prezero() that nobody has written yet
        self._seen_idx -= {k for k in self._touched if isinstance(k, int) and k not in self._zeroed}
        self._seen_ptr -= done
        self._touched = []

    def end_scaled(self):
        """-> 1/S (device scalar) for gradients the engine hands back to autograd (StackEngine's dx)"""
        self.unscale()
        inv = self.inv
        self.scale = self.inv = None
        return inv
