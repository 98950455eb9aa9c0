"""Kernel sequencing for the TimeSformer divided space-time encoder (forward + backward).

This is the host side of the hot path `VisionTransformer.forward_features`
(reference lib/models/vit.py:365-423) and its autograd backward, restated as an explicit
schedule of C-ABI kernel launches (include/pvrl.h) on torch's current HIP stream.

Token layout (the residual stream x has M = B*N*T + B rows of C = embed_dim channels: 768 for ViT-B, 1024 for ViT-L):
    rows [0, R)   patch tokens ordered (b, n, t), t innermost      R = B*N*T     16-bit operand type since round 6 (`_X`, resid16)
    rows [R, M)   the cls token of clip b                                        fp32
The reference keeps [B, 1 + N*T, C] and re-gathers it with einops for every branch
(vit.py:130-151); here temporal sequences are 8 consecutive rows, spatial sequences are
addressed in place by the attention kernel, and the cls rows are a small suffix, so the
three residual branches of a block are 3 LayerNorms + 7 GEMMs + 2 attention launches and no
copy kernels.  Activations are GEMM operands in the library's 16-bit type (fp16 by default); the cls rows of the residual stream,
LayerNorm statistics, softmax statistics and all parameter gradients are fp32.

TIMESFORMER.ATTENTION_TYPE 'joint_space_time' / 'space_only' (vit.py:124-127) take ONE undivided block path on the same row layout
(`_block_fwd_undivided` / `_block_bwd_undivided`): a sample's sequence is its cls row plus its N*T patch rows (the attention kernels'
mode 1 with T = 1); `space_only` runs it on B*T one-frame pseudo-clips and averages a clip's cls rows in front of the final norm.
"""
import math
import os

import torch

from . import ops
from ._lib import lib
from .grads import SCALED_GRADS, GradStore                # (re-exported: `from procedurevrl_amd.engine import GradStore` keeps working)
from .graphs import GraphReplay, drop_graphs_quietly      # (their home; re-exported like the two above)
from .transform import DecodedClips

OP16 = ops.OP16
F32 = torch.float32


class _X:
    """One stage of the encoder's residual stream (or of its gradient): patch rows `p` [R, C], cls rows `c` [B, C] fp32.
    Split stream (EncoderEngine.resid16, round 6): `p` is its own tensor in the 16-bit operand type -- GEMM residual epilogues
    (PVRL_EPI_RESID_16) read and write it, the LayerNorm kernels take the two parts as one matrix (ops.SplitRows / pvrl_rows).
    Otherwise `p` and `c` are views of ONE fp32 buffer `full` [R + B, C] (rounds 1-5)."""
    __slots__ = ("p", "c", "full")

    def __init__(self, p, c, full=None):
        self.p, self.c, self.full = p, c, full

    @staticmethod
    def new(R, B, C, device, split, zero=False, zero_p=True):
        mk = torch.zeros if zero else torch.empty
        if split:
            return _X((mk if zero_p else torch.empty)((R, C), device=device, dtype=OP16), mk((B, C), device=device, dtype=F32))
        full = mk((R + B, C), device=device, dtype=F32)
        return _X(full[:R], full[R:], full)

    def all(self, p_zero=False):
        """every row, as the LayerNorm entry points take it (`p_zero`: the patch rows are known to be zero and are not read)"""
        if self.full is not None:
            return self.full
        return ops.SplitRows(None if p_zero else self.p, self.c, n_lo=self.p.shape[0])

    def patch(self):
        return self.p if self.full is not None else ops.SplitRows(self.p, None)


def storage_nbytes(obj, seen=None):
    """bytes of the distinct storages under `obj` (tensors, `_X` stages, dicts, lists, tuples); views of one storage -- and a tensor two
    entries share, like the cls rows `x1.c is x0.c` of the split stream -- count once.  `seen`: storages already counted elsewhere."""
    seen = set() if seen is None else seen
    if isinstance(obj, torch.Tensor):
        st = obj.untyped_storage()
        if st.data_ptr() in seen:
            return 0
        seen.add(st.data_ptr())
        return st.nbytes()
    if isinstance(obj, _X):
        obj = (obj.p, obj.c, obj.full)
    elif isinstance(obj, dict):
        obj = obj.values()
    elif not isinstance(obj, (list, tuple)):
        return 0
    return sum(storage_nbytes(v, seen) for v in obj)


class EncoderEngine(GraphReplay):
    DWE_LIMIT = 32768.0     # fp16 flavour: the largest |S-scaled dW_e| its 16-bit copies are allowed to hold, 2 x below 65,504 (_temporal_chain_all)

    def __init__(self, model):
        """`model` is a procedurevrl_amd.vit.VisionTransformer (same parameter names as the reference)."""
        self.m = model
        # 'space_only' / 'joint_space_time' (vit.py:124-127): ONE attention over each sample's tokens and an MLP per block -- the undivided
        # block path below (_block_fwd_undivided / _block_bwd_undivided); `space_only` runs it on B * T one-frame pseudo-clips
        self.undivided = getattr(model, "attention_type", "divided_space_time") != "divided_space_time"
        self.space_only = getattr(model, "attention_type", "") == "space_only"
        self.C = model.embed_dim
        self.H = model.num_heads
        self.scale = (self.C // self.H) ** -0.5
        self.eps = model.ln_eps
        self.weights = model.weights      # weights.WeightCache: the 16-bit operand copies, shared with the head and the text tower
        self._grads = None
        self.saved = None
        self.grad_hook = None
        self._dwe_rescale = False
        # ONE STREAM since round 5.  Until round 4 the weight-gradient GEMMs ran on a side stream next to the dgrad chain and the
        # fused temporal maps W_e were built on it at the start of the forward.  Measured (profiles/r5_hw_queues.txt, two passes):
        # single stream 636.5 clips/s, W_e prefetch only 632.3, both 622.7 -- and only the single-stream step is independent of how
        # HIP maps streams to hardware queues: with the side stream it is 58 ms instead of 51 at GPU_MAX_HW_QUEUES=6 (the branches of
        # its graph truly co-run), the capture segfaults inside ROCm 7 at 1-2 queues, and under a foreign stream's long kernel (RCCL)
        # it stalls behind whatever shares its queue (tools/probe/comm_cus_ab.py).  Grouped weight-gradient launches fill the chip on
        # their own; there is nothing to overlap.
        # the C^3 GEMMs of the fused temporal branch (W_e per block in forward; dW_fc, dW_proj per block in backward) are batched into
        # one launch per dozen (ops.gemm_nt_batched): 36 tiles apiece cannot fill 256 CUs
        # with a gradient hook (data parallel): blocks per group -- the hook runs (and the deferred launches go out, batched) once per
        # group of this many blocks instead of per block: four all-reduce rounds of ~135 MB per backward instead of twelve of 45
        self.hook_group = max(1, int(os.environ.get("PVRL_HOOK_GROUP", "3")))
        self.hook_tail_split = os.environ.get("PVRL_HOOK_TAIL_SPLIT", "1") == "1"      # the backward's last group per block (_group_of)
        self._fused_fresh = set()
        self._chain = []
        self._ln_defer = []
        self.group_wgrad = True       # one grouped launch for a block's seven weight gradients
        # the B cls rows' projection + MLP in fp32 on the master weights (csrc/cls_chain.hip; PVRL_CLS_FP32=0: A/B runs)
        self.cls_fp32 = os.environ.get("PVRL_CLS_FP32", "1") == "1"
        # Only the cls row of the LAST block's output is read (final norm + `x[:, 0]`, vit.py:418-421): that block's spatial projection
        # and MLP touch the cls rows alone, forward and backward -- the reference computes (and back-propagates zeros through) all 1,569
        # tokens of every clip there.  Same features, loss and gradients; PVRL_PRUNE_LAST=0: A/B runs.
        self.prune_last = os.environ.get("PVRL_PRUNE_LAST", "1") == "1"
        self.prune_attn = os.environ.get("PVRL_PRUNE_ATTN", "1") == "1"     # ... and its spatial attention the cls query only (attn_cls.hip)
        # SPLIT residual stream (round 6): the patch rows of x and of its gradient dx live in the 16-bit operand type between kernels,
        # the B cls rows stay fp32 -- per block 18 passes over the 50k token rows move 77 instead of 154 MB.  What it costs in error is
        # what the rounding-model oracle says (profiles/r6_resid16_rounding.txt: logits 2.84e-4 -> 2.96e-4, worst gradient 1.09e-3 ->
        # 1.16e-3 at 12 blocks, fp16 operands).  PVRL_RESID16=0: the fp32 stream of rounds 1-5 (A/B runs).
        self.resid16 = os.environ.get("PVRL_RESID16", "1") == "1"
        # Debug aid (VERDICT r5 weak #11 / ADVICE): with the last block pruned, the patch rows of its x2 / x3, the patch queries of its qkv,
        # o_s[:R], the patch rows of the gradient stream ahead of its norm1 backward and the query third of its dqkv are never written --
        # correct only while nothing reads them.  PVRL_DEBUG_NAN_UNDEFINED=1 fills every such region with NaN, so a reader that should
        # not exist turns the loss / gradients NaN (tests/e2e_checks.check_train_step_undefined_rows_nan_filled runs the suite's steps so).
        self.debug_nan_undefined = os.environ.get("PVRL_DEBUG_NAN_UNDEFINED", "0") == "1"
        # MODEL.ACT_CHECKPOINT (the reference's defaults.py:413): a training forward keeps, of every block but the last, its input stage
        # and its DropPath scales alone; the backward runs that block's forward again (_recompute) in front of its own kernels.  No
        # training kernel uses atomics, so the recomputed activations -- hence features and gradients -- are the plain path's bit for
        # bit.  The last block is kept whole: its activations are the first the backward frees, the peak would be the same.
        self.act_checkpoint = bool(model.cfg.MODEL.ACT_CHECKPOINT)
        self._wq = []
        self._keep = None
        self._graph_init()            # HIP-graph replay of the step (GraphReplay)
        self._refreshed = False
        self._tok = False             # the running forward() returns every token (part of the graph key)
        # the sizes the kernels serve, ViT-B (768, 12) and ViT-L (1024, 16): a clear error here for any other pair
        ops.check_encoder_width(self.C, self.H)
        # the geometry the model was built for (DATA.TRAIN_CROP_SIZE, DATA.NUM_FRAMES) against the attention kernels' limits: a clear
        # error here instead of PVRL_EINVAL from inside the first block (a forward checks its input's own geometry again)
        self._check_geometry(model.patch_embed.num_patches, model.time_embed.shape[1] if hasattr(model, "time_embed") else 1)

    def _check_geometry(self, N, T, prune=True, **keys):
        """`prune` False: a call whose last block runs unpruned whatever the switches say (forward(tokens=True))"""
        scheme = getattr(self.m, "attention_type", "divided_space_time")
        ops.check_attn_geometry(N, T, scheme, prune and self.prune_last and self.prune_attn, **keys)

    # ------------------------------------------------------------------ weights
    def _weight(self, p, need_t=True):
        """operand copies of `p`; re-cast inside a forward capture unless _refresh_weights() has just done it (weights.WeightCache.get)"""
        return self.weights.get(p, need_t, force=self._capturing == "fwd" and not self._refreshed, frozen=self._capturing == "bwd")

    def _refresh_weights(self):
        """Bring the bf16 operand copies of every encoder weight up to date in ONE launch (pvrl_cast_weights_multi_bf16)
        instead of one 6-us launch per matrix on first use; afterwards _weight() finds every version current."""
        m = self.m
        plist = [(m.patch_embed.proj.weight, False)]
        for blk in m.blocks:
            if not self.undivided:
                plist += [(blk.temporal_attn.qkv.weight, True), (blk.temporal_attn.proj.weight, True), (blk.temporal_fc.weight, True)]
            plist += [(blk.attn.qkv.weight, True), (blk.attn.proj.weight, True),
                      (blk.mlp.fc1.weight, True), (blk.mlp.fc2.weight, True)]
        self.weights.refresh(plist, force=self._capturing == "fwd")

    def _fused_temporal(self, blk):
        """The temporal branch applies two linear maps back to back (vit.py:131-134: temporal_attn.proj, DropPath, then
        temporal_fc), so  x + fc(rs * proj(o)) = x + rs * (o W_e^T + b_e) + b_fc  with  W_e = W_fc W_proj,  b_e = W_fc b_proj:
        ONE 50k-row GEMM forward (and one data-gradient / one weight-gradient GEMM backward) instead of two each.
        W_e is rebuilt from the bf16 operand copies whenever either weight changed (a C^3 MFMA GEMM); the parameter
        gradients are recovered from dW_e in backward (`_temporal_chain_all`)."""
        wf, wp = blk.temporal_fc.weight, blk.temporal_attn.proj.weight
        e = self.weights.entry(wf, "fused_t")
        ef, ep = self._weight(wf), self._weight(wp)
        ver = (ef.ver, ep.ver, blk.temporal_attn.proj.bias._version)
        if self._capturing == "bwd" or id(blk) in self._fused_fresh:     # (built a moment ago by _build_fused_all)
            return e
        if self._capturing == "fwd" or e.ver != ver or e.w is None:
            L = lib()
            we = ops.gemm_nt(ef.w, ep.t, L.PVRL_EPI_F32)                    # [out, in] = W_fc [out, mid] . W_proj [mid, in]
            e.w, e.t = ops.cast_weight(we, out=e.w, out_t=e.t)
            e.be = ops.gemv_rows(wf.detach(), blk.temporal_attn.proj.bias.detach(), out=e.be)                 # [out]
            e.ver = ver
        return e

    def _fused_temporal_stale(self, blk):
        if self._capturing == "fwd":
            return True
        e = self.weights.peek(blk.temporal_fc.weight, "fused_t")
        if e is None or e.w is None:
            return True
        ef = self.weights.peek(blk.temporal_fc.weight)
        ep = self.weights.peek(blk.temporal_attn.proj.weight)
        return ef is None or ep is None or e.ver != (ef.ver, ep.ver, blk.temporal_attn.proj.bias._version)

    def _build_fused_all(self):
        """W_e = W_fc W_proj (and b_e) of every block whose weights changed, at the start of a forward: ONE batched launch of the blocks'
        C^3 GEMMs and one of their casts instead of a GEMM (16.6 us at C = 768) + a cast in front of every block's temporal GEMM."""
        self._fused_fresh = set()
        if self.undivided:
            return
        stale = [blk for blk in self.m.blocks if self._fused_temporal_stale(blk)]
        if len(stale) < 2:
            return
        L = lib()
        ents, probs = [], []
        for blk in stale:
            wf, wp = blk.temporal_fc.weight, blk.temporal_attn.proj.weight
            e = self.weights.entry(wf, "fused_t")
            ef, ep = self._weight(wf), self._weight(wp)
            ents.append((blk, e, ef, ep))
            probs.append(dict(A=ef.w, W=ep.t))                              # [out, in] = W_fc [out, mid] . W_proj [mid, in]
        wes = ops.gemm_nt_batched(probs, L.PVRL_EPI_F32)
        items = []
        for we, (blk, e, ef, ep) in zip(wes, ents):
            if e.w is None or e.w.device != we.device:
                e.w = torch.empty(we.shape, device=we.device, dtype=OP16)
                e.t = torch.empty((we.shape[1], we.shape[0]), device=we.device, dtype=OP16)
            items.append((we, e.w, e.t))
        ops.cast_weights_multi(items)
        for blk, e, ef, ep in ents:
            if e.be is None or e.be.device != wes[0].device:
                e.be = torch.empty(self.C, device=wes[0].device, dtype=F32)
        ops.gemv_rows_batched([blk.temporal_fc.weight.detach() for blk, _, _, _ in ents],
                              [blk.temporal_attn.proj.bias.detach() for blk, _, _, _ in ents], [e.be for _, e, _, _ in ents],
                              [0.0] * len(ents))                               # b_e = W_fc b_proj
        for blk, e, ef, ep in ents:
            e.ver = (ef.ver, ep.ver, blk.temporal_attn.proj.bias._version)
            self._fused_fresh.add(id(blk))

    def _temporal_chain_all(self, gs):
        """dW_e [out, in], db_e [out] (fp32, from the weight-gradient GEMM of each fused map the backward queued) -> gradients of the
        four parameters:  dW_fc = dW_e W_proj^T + db_e b_proj^T,  dW_proj = W_fc^T dW_e,  db_proj = W_fc^T db_e  (db_fc comes from the
        LayerNorm backward's column sums).  Nobody needs a block's gradients before the end of the backward (of its group, under a
        gradient hook): the two GEMMs per block as batched launches, the blocks' casts as one."""
        chain, self._chain = self._chain, []
        if not chain:
            return
        L = lib()
        # dW_e / db_e are in the backward's S-scaled units (fp16 flavour; their 16-bit copies must stay mid-range); the scale is taken
        # out where the four parameter gradients are written: a row scale of 1 / S in the GEMM epilogues, `gscale` below
        rs = gs.inv_row if gs.inv is not None else None
        dev = chain[0][1].device
        C = self.C
        rss = [rs] * len(chain)
        if rs is not None and self._dwe_rescale:
            # dW_e is the one S-scaled SUM OVER ALL PATCH ROWS that is rounded to 16 bits.  Under an all-token gradient (forward(tokens=True):
            # up to 256 in S units on EVERY row, not on one row per clip) it grows with the row count and passes fp16's 65,504 (mean-pooled
            # tokens, 32 clips of 8 x 224^2: 2.4e5).  There its copies get a power of two of their own, 2^-e with the
            # smallest e >= 0 that brings max|dW_e| under DWE_LIMIT, chosen on the device; 2^e goes into the row scale of the two GEMMs
            # (db_e is used in fp32).  Exact, and e = 0 -- nothing changes, not a bit -- below the limit.  The cls path (measured 100 x
            # below 65,504 at the same row count) keeps its launches as they are.
            amax = torch.nan_to_num(torch.stack(torch._foreach_norm([dwe for _, dwe, _ in chain], float("inf"))), nan=1.0, posinf=3e38)
            e = torch.ceil(torch.log2(amax.clamp_min(1e-30) / self.DWE_LIMIT)).clamp(0.0, 100.0)
            for (_, dwe, _), f in zip(chain, torch.exp2(-e).unbind(0)):
                dwe.mul_(f)
            rss = list((torch.exp2(e).unsqueeze(1) * rs.unsqueeze(0)).unbind(0))
        items = []
        for blk, dwe, dbe in chain:
            items.append((dwe, torch.empty((C, C), device=dev, dtype=OP16), torch.empty((C, C), device=dev, dtype=OP16)))
        ops.cast_weights_multi(items)
        groups = {0.0: [], 1.0: []}
        fresh = {}      # id(blk) -> (temporal_fc.weight gradient that is already there, the new one): see below
        for (blk, dwe, dbe), (_, dwe_b, dwe_t), rsi in zip(chain, items, rss):
            wf, wp = blk.temporal_fc.weight, blk.temporal_attn.proj.weight
            ef, ep = self._weight(wf), self._weight(wp)
            for lin_w, A, W in ((wf, dwe_b, ep.w), (wp, ef.t, dwe_t)):       # [out,mid] = dW_e.W_p^T ; [mid,in] = W_f^T.dW_e
                # (gemm_nt_batched / rank1_add / gemv_rows take no `nonfinite` argument: checks=False keeps these parameters in the optimiser's scan)
                g, beta = gs.target(lin_w, fused=True, checks=False)
                if beta and lin_w is wf:
                    # dW_fc is written in two steps (this GEMM, then the rank-1 term db_e b_proj^T) that may cancel: added one after the
                    # other to a gradient that is already there, each rounds at ITS OWN size, not the sum's.  An accumulating step
                    # (eager launches, never captured) forms the new gradient first and adds it once: one rounding of the sum.
                    fresh[id(blk)] = (g, torch.empty_like(g))
                    g, beta = fresh[id(blk)][1], 0.0
                groups[beta].append(dict(A=A, W=W, rowscale=rsi, out0=g, aux=g if beta else None))
        if groups[0.0]:
            ops.gemm_nt_batched(groups[0.0], L.PVRL_EPI_F32)
        if groups[1.0]:
            ops.gemm_nt_batched(groups[1.0], L.PVRL_EPI_RESID_F32)
        ops.rank1_add_batched([fresh[id(blk)][1] if id(blk) in fresh else gs.target(blk.temporal_fc.weight, fused=True, checks=False)[0]
                               for blk, _, _ in chain],
                              [dbe for _, _, dbe in chain], [blk.temporal_attn.proj.bias.detach() for blk, _, _ in chain], gscale=gs.inv)
        for g, new in fresh.values():
            g.add_(new)
        tb = [gs.target(blk.temporal_attn.proj.bias, fused=True, checks=False) for blk, _, _ in chain]
        ops.gemv_rows_batched([self._weight(blk.temporal_fc.weight).t for blk, _, _ in chain], [dbe for _, _, dbe in chain],
                              [t for t, _ in tb], [b for _, b in tb], gscale=gs.inv)

    def _finish_deferred(self, gs):
        """what the blocks' backward left for the end (no gradient hook): the fused temporal chains and the LayerNorm partial reduces"""
        self._temporal_chain_all(gs)
        items, self._ln_defer = self._ln_defer, []
        ops.layernorm_bwd_reduce_batched(items, gscale=gs.inv, nonfinite=gs.bad)

    def grad_store(self):
        return self.m.grad_store()

    # ------------------------------------------------------------------ weight gradients
    def _wgrad(self, dy, xin, dw, dbias, beta, gscale=None, nonfinite=None):
        """queue dW = beta*dW + gscale * dy^T xin (and dbias); `flush_wgrads` issues what is queued."""
        self._wq.append((dy, xin, dw, dbias, beta, gscale, nonfinite))
        if not self.group_wgrad:
            self.flush_wgrads()

    def flush_wgrads(self):
        """Issue the queued weight gradients as one grouped launch (ops.gemm_tn_grouped)."""
        q, self._wq = self._wq, []
        if q:
            ops.gemm_tn_grouped(q, ws_tag="tn")

    # every parameter gradient of a block is written by a kernel that takes the backward's scale out itself (`gscale` = 1 / S,
    # fp16 flavour) and raises the optimiser's skip flag on a non-finite value (`nonfinite`): no pass over the gradient buffer
    def _lin_wgrad(self, gs, dy, xin, lin, queue=True):
        """the weight / bias gradient of the linear layer `lin` from dy^T xin: queued for the block's grouped launch, or
        (queue=False) returned as an item for a launch of the caller's own"""
        (dw, bw), (dbias, _) = gs.target(lin.weight, fused=True), gs.target(lin.bias, fused=True)
        item = (dy, xin, dw, dbias, bw, gs.inv, gs.bad)
        if not queue:
            return item
        self._wgrad(*item)

    # (the 7-us reduces of the LayerNorm partials are deferred: one launch for the whole backward, or per group of blocks under a gradient hook)
    def _lnbwd(self, gs, dh, x, st, ln, dx_in, dx_out, **sums):
        """backward of the LayerNorm `ln` on the gradient stream (dx_out = dx_in + ...); `sums`: ops.layernorm_bwd's dxs / dxsum arguments"""
        (dg, bg), (db, _) = gs.target(ln.weight, fused=True), gs.target(ln.bias, fused=True)
        ops.layernorm_bwd(dh, x, st[0], st[1], ln.weight.detach(), dg, db, dx_in=dx_in, dx_out=dx_out, beta_acc=bg,
                          gscale=gs.inv, nonfinite=gs.bad, defer=self._ln_defer, **sums)

    # ------------------------------------------------------------------ drop path
    def _droppath_keep(self, device, training):
        """-> (the blocks' DropPath rates, keep = 1 - rate as fp32 [nb, 1] on the device -- None when this pass draws nothing)"""
        rates = [float(r) for r in self.m.drop_path_rates]
        if not training or all(r == 0.0 for r in rates):
            return rates, None
        if self._keep is None or self._keep[0] != (tuple(rates), device):   # cached: a host->device copy blocks the host
            self._keep = ((tuple(rates), device), torch.tensor([1.0 - r for r in rates], device=device, dtype=F32).view(len(rates), 1))
        return rates, self._keep[1]

    def _droppath_all(self, B, N, T, device, training):
        """DropPath row scales of every block, lib/models/vit_utils.py:140-155: floor(keep + U[0,1)) / keep per dim-0 row
        of each branch (temporal: per (b h w); spatial: per (b t); mlp: per b).  All blocks are drawn and expanded to
        token rows with ONE set of launches (a per-block version costs ~20 tiny kernels x depth on the critical path)."""
        rates, keep = self._droppath_keep(device, training)
        nb = len(rates)
        if keep is None:
            return [None] * nb
        n1, n2, n3 = B * N, B * T, B
        sc = torch.floor(keep + torch.rand((nb, n1 + n2 + n3), device=device)) / keep
        s1, s2, s3 = sc[:, :n1], sc[:, n1:n1 + n2], sc[:, n1 + n2:]
        s1_tok = s1.repeat_interleave(T, dim=1)                                       # [nb, B*N*T]
        s2_seq = s2.contiguous()
        s2_tok = s2.reshape(nb, B, 1, T).expand(nb, B, N, T).reshape(nb, -1)          # [nb, B*N*T]
        s3_all = torch.cat([s3.repeat_interleave(N * T, dim=1), s3], 1)               # [nb, B*N*T + B]
        s2_mean = s2.reshape(nb, B, T).mean(2)                                        # [nb, B]: the cls rows' bias factor
        return [None if rates[i] == 0.0 else dict(s1_tok=s1_tok[i], s2_seq=s2_seq[i], s2_tok=s2_tok[i], s3_all=s3_all[i],
                                                  s2_mean=s2_mean[i])
                for i in range(nb)]

    def _droppath_undivided(self, B, N, T, device, training):
        """DropPath of the undivided schemes: one draw per dim-0 sample and branch (vit.py:125-126 through vit_utils.py:140-155) -- per
        clip for `joint_space_time`, per (clip, frame) for `space_only`, whose pseudo-clips are the B here"""
        rates, keep = self._droppath_keep(device, training)
        nb = len(rates)
        if keep is None:
            return [None] * nb
        sc = torch.floor(keep + torch.rand((nb, 2 * B), device=device)) / keep
        s2, s3 = sc[:, :B], sc[:, B:]
        s2_all = torch.cat([s2.repeat_interleave(N * T, dim=1), s2], 1)               # [nb, B*N*T + B]
        s3_all = torch.cat([s3.repeat_interleave(N * T, dim=1), s3], 1)
        return [None if rates[i] == 0.0 else dict(s2_all=s2_all[i], s3_all=s3_all[i]) for i in range(nb)]

    @staticmethod
    def expand_droppath_undivided(s_attn, s_mlp, B, N, T):
        """pinned draws of one undivided block: s_attn / s_mlp fp32 [B] = floor(keep + u) / keep of its two DropPath calls (B: clips
        for `joint_space_time`, (clip, frame) pairs for `space_only` with T = 1) -> the dict forward(..., droppath=[...]) takes"""
        exp = lambda v: torch.cat([v.repeat_interleave(N * T), v]).contiguous()
        return dict(s2_all=exp(s_attn), s3_all=exp(s_mlp))

    @staticmethod
    def expand_droppath(s1, s2, s3, B, N, T):
        s1_tok = s1.repeat_interleave(T).contiguous()
        s2_tok = s2.view(B, 1, T).expand(B, N, T).reshape(-1).contiguous()
        s3_all = torch.cat([s3.repeat_interleave(N * T), s3]).contiguous()
        return dict(s1_tok=s1_tok, s2_seq=s2.contiguous(), s2_tok=s2_tok, s3_all=s3_all, s2_mean=s2.view(B, T).mean(1))

    # ------------------------------------------------------------------ embeddings
    def _pos_time(self, N, T, Wp):
        """nearest-neighbour resize of pos/time embeddings when the input differs (vit.py:375-386,398-402)."""
        m = self.m
        pos = m.pos_embed[0]
        if pos.shape[0] != N + 1:
            P = int(math.isqrt(pos.shape[0] - 1))
            Hn = N // Wp
            other = pos[1:].t().reshape(1, self.C, P, P)
            other = torch.nn.functional.interpolate(other, size=(Hn, Wp), mode="nearest").flatten(2)[0].t()
            pos = torch.cat([pos[:1], other], 0)
        if self.space_only:         # no time embedding (vit.py:393): a zero row for the embedding table
            return pos.contiguous(), torch.zeros((1, self.C), device=pos.device, dtype=pos.dtype)
        tim = m.time_embed[0]
        if tim.shape[0] != T:
            tim = torch.nn.functional.interpolate(tim.t().unsqueeze(0), size=T, mode="nearest")[0].t()
        return pos.contiguous(), tim.contiguous()

    # ------------------------------------------------------------------ forward
    def forward(self, frames, training, droppath=None, save=True, tokens=False):
        """frames fp32 [B, 3, T, H, W] on the GPU (or transform.DecodedClips) -> (feat fp32 [B, C] = norm(x)[:, 0]).
        `droppath`: optional list (per block) of dicts from expand_droppath, to pin the RNG draws.
        `tokens`: norm(x) of every token instead, fp32 [B, 1 + N*T, C] in the reference's order (forward_features(cls=False),
        vit.py:418-423; [B, 1 + N, C] for `space_only`): the last block then runs unpruned and the final norm covers all rows.
        With `use_graphs` the launch sequence of a (shape, mode) is captured once into a HIP graph and replayed."""
        self._tok = bool(tokens)            # (read by _graph_key / _eager_forward: the replay core passes frames, training, save)
        try:
            if self.use_graphs and droppath is None and isinstance(frames, torch.Tensor) and frames.is_cuda:
                return self._graph_forward(frames, training, save)
            self._gkey = None
            return self._forward(frames, training, droppath, save, tokens=self._tok)
        finally:
            self._tok = False

    def _forward(self, frames, training, droppath=None, save=True, tokens=False):
        # the input's own geometry (a test crop may differ from the model's) against the kernels' limits, before the first launch
        self._check_geometry((frames.shape[3] // 16) * (frames.shape[4] // 16), frames.shape[2], prune=not tokens,
                             crop_key="input crop (DATA.TRAIN_CROP_SIZE / DATA.TEST_CROP_SIZE)", frames_key="input frames (DATA.NUM_FRAMES)")
        L = lib()
        m = self.m
        self._refresh_weights()
        self._refreshed = True
        self._build_fused_all()
        frames_per_clip = 0
        if self.space_only:
            # every frame is a sample of its own (vit.py:174-180: PatchEmbed folds T into the batch, and nothing unfolds it before the
            # mean over the frames' cls rows, vit.py:414-416): B * T pseudo-clips of one frame, rows (b * T + t, n)
            if isinstance(frames, DecodedClips):
                frames = ops.frames_u8_to_f32(frames)
            frames_per_clip = frames.shape[2]
            frames = frames.permute(0, 2, 1, 3, 4).reshape(-1, frames.shape[1], 1, frames.shape[3], frames.shape[4])
        B, _, T, HI, WI = frames.shape
        Wp = WI // 16
        N = (HI // 16) * Wp
        R = B * N * T
        M = R + B
        C = self.C
        dev = frames.device
        sv = dict(B=B, T=T, N=N, R=R, M=M, Wp=Wp, blocks=[], ckpt=bool(save and self.act_checkpoint))
        if tokens:
            sv["tokens"] = True

        if isinstance(frames, DecodedClips):     # decoded uint8 clips: GPU-side normalise/rescale/crop/flip + im2col
            a_pe = ops.frames_u8_patchify(frames)
        else:
            a_pe = ops.patchify(frames.contiguous())
        pos, tim = self._pos_time(N, T, Wp)
        E = ops.embed_table(pos, tim, m.patch_embed.proj.bias.detach(), N, T)
        x = _X.new(R, B, C, dev, self.resid16)
        sv["split"] = self.resid16
        wpe = self._weight(m.patch_embed.proj.weight, need_t=False)
        ops.gemm_nt(a_pe, wpe.w, self._epi_resid(), aux=E, aux_rowmod=N * T, out0=x.p)
        x.c[:] = (m.cls_token.detach()[0, 0] + pos[0]).unsqueeze(0)
        sv["a_pe"] = a_pe if save else None

        if droppath is None:
            droppath = (self._droppath_undivided if self.undivided else self._droppath_all)(B, N, T, dev, training)
        for i, blk in enumerate(m.blocks):
            last = i == len(m.blocks) - 1
            ckpt = save and self.act_checkpoint and not last
            if self.undivided:
                x = self._block_fwd_undivided(blk, x, sv, droppath[i], save, ckpt=ckpt)
            else:
                x = self._block_fwd(blk, x, sv, droppath[i], save, last=last, ckpt=ckpt, tokens=tokens)

        if tokens:
            return self._final_norm_tokens(x, sv, frames_per_clip, save)
        if frames_per_clip:         # vit.py:414-416: the mean over the frames, in front of the final norm (only x[:, 0] is read)
            sv["frames_per_clip"] = frames_per_clip
            x = _X(x.p, x.c.view(-1, frames_per_clip, C).mean(1))
        feat, mean, rstd = ops.layernorm_fwd(x.c, m.norm.weight.detach(), m.norm.bias.detach(), self.eps,
                                             out_dtype=F32)
        self._refreshed = False
        if save:
            sv["x_final"] = x
            sv["norm_stats"] = (mean, rstd)
            self.saved = sv
            if SCALED_GRADS:
                # fp16 operands: a 16-bit forward activation past 65504 (qkv, the MLP's u / g, attention outputs) is an inf that reaches
                # every later block's cls row through the attention, i.e. these B x C features: one few-microsecond check raises the
                # optimiser's skip flag on the device, in the step that overflowed, whatever the caller does with its loss
                gs = self.grad_store()
                lib().call("pvrl_nonfinite_flag_f32", ops._ptr(feat), feat.numel(), ops._ptr(gs.bad), ops._stream())
        return feat

    def _final_norm_tokens(self, x, sv, frames_per_clip, save):
        """the tail of a tokens forward: norm(x) of every row, written by ONE launch straight into the reference's token order
        (pvrl_layernorm_fwd_tokens) -> fp32 [B, 1 + P, C]"""
        m = self.m
        B, N, T, R, C = sv["B"], sv["N"], sv["T"], sv["R"], self.C
        P = N * T
        if frames_per_clip:
            # `space_only` (vit.py:414-416): the mean over a clip's frames covers every token.  The rows are (b, t, n): as a matrix
            # [B * T, N * C] the patch rows are groups of T consecutive rows, which is pvrl_group_reduce's grouping -- it reads the
            # stream's values and accumulates in fp32; the B * T cls rows with torch ops, as in the cls path.  The mean stays fp32.
            sv["frames_per_clip"] = frames_per_clip
            B, P = B // frames_per_clip, N
            full = torch.empty((B * N + B, C), device=x.c.device, dtype=F32)
            ops.group_reduce(x.p.view(B * frames_per_clip, N * C), B, frames_per_clip, alpha=1.0 / frames_per_clip,
                             out=full[:B * N].view(B, N * C))
            full[B * N:] = x.c.view(B, frames_per_clip, C).mean(1)
            x = _X(full[:B * N], full[B * N:], full)
        tok, mean, rstd = ops.layernorm_fwd_tokens(x.all(), m.norm.weight.detach(), m.norm.bias.detach(), self.eps, P)
        self._refreshed = False
        if save:
            sv["x_final"] = x
            sv["norm_stats"] = (mean, rstd)
            self.saved = sv
            if SCALED_GRADS:        # (see _forward: an overflowed 16-bit activation raises the optimiser's skip flag)
                gs = self.grad_store()
                lib().call("pvrl_nonfinite_flag_f32", ops._ptr(tok), tok.numel(), ops._ptr(gs.bad), ops._stream())
        return tok.view(B, P + 1, C)

    def saved_nbytes(self):
        """bytes the last training forward keeps for its backward: the distinct storages under `self.saved` (storage_nbytes)"""
        return storage_nbytes(self.saved)

    def stream_from_rows(self, x_rows, B):
        """fp32 [B*N*T + B, C] (patch rows, then cls rows) -> a stage of the residual stream as this engine keeps it (tests / probes)"""
        R = x_rows.shape[0] - B
        if not self.resid16:
            full = x_rows.contiguous()
            return _X(full[:R], full[R:], full)
        return _X(x_rows[:R].to(OP16).contiguous(), x_rows[R:].contiguous())

    @staticmethod
    def stream_to_rows(x):
        return x.full if x.full is not None else torch.cat([x.p.float(), x.c], 0)

    def _undef(self, t):
        """`t` is deliberately left unwritten (see debug_nan_undefined)"""
        if self.debug_nan_undefined and t is not None and t.numel():
            t.fill_(float("nan"))
        return t

    def _epi_resid(self):
        L = lib()
        return L.PVRL_EPI_RESID_16 if self.resid16 else L.PVRL_EPI_RESID_F32

    def _cls_mlp_fp32(self, blk, xc, s3c, out):
        """out = xc + s3c * mlp(norm2(xc)) for the B cls rows in fp32 on the master weights (csrc/cls_chain.hip)"""
        P = lambda t: t.detach()
        hc, _, _ = ops.layernorm_fwd(xc, P(blk.norm2.weight), P(blk.norm2.bias), self.eps, out_dtype=F32, save_stats=False)
        gc = ops.cls_linear(hc, P(blk.mlp.fc1.weight), P(blk.mlp.fc1.bias), gelu=True)
        ops.cls_linear(gc, P(blk.mlp.fc2.weight), P(blk.mlp.fc2.bias), rowscale=s3c, biasscale=s3c, aux=xc, out=out)

    def _fc1(self, blk, h_m, keep_u):
        """-> (u, g) = (fc1(h_m), GELU(u)) in the 16-bit operand type; u is None unless `keep_u` (only the backward's PVRL_EPI_DGELU reads
        it: without it the GEMM's largest output of the block is not written)"""
        L = lib()
        w1, b1 = self._weight(blk.mlp.fc1.weight).w, blk.mlp.fc1.bias.detach()
        if keep_u:
            return ops.gemm_nt(h_m, w1, L.PVRL_EPI_GELU, bias=b1)
        return None, ops.gemm_nt(h_m, w1, L.PVRL_EPI_GELU_ONLY, bias=b1)

    def _mlp_fwd(self, blk, x, s3_all, sv, whole=False, keep_u=True, recompute=False):
        """x + s3 * mlp(norm2(x)) on every row (vit.py:155-157) -> (the next stage, h_m, (mean_m, rstd_m), u, g): what the block saves.
        `whole`: the one-buffer fp32 stream of the divided path, fc2 as ONE GEMM over all rows.  `keep_u` False: nobody will read the
        pre-activation u (it is None; PVRL_EPI_GELU_ONLY writes the same g).  `recompute`: a checkpointed block's second pass -- the
        next stage exists already, so fc2, the cls rows' fp32 chain and the stage's allocation are skipped (it is None)"""
        L = lib()
        B, R = sv["B"], sv["R"]
        P = lambda t: t.detach()
        h_m, mean_m, rstd_m = ops.layernorm_fwd(x.all(), P(blk.norm2.weight), P(blk.norm2.bias), self.eps)
        u, g = self._fc1(blk, h_m, keep_u)
        if recompute:
            return None, h_m, (mean_m, rstd_m), u, g
        y = _X.new(R, B, self.C, x.c.device, sv["split"])
        s3c = s3_all[R:] if s3_all is not None else None
        w2 = self._weight(blk.mlp.fc2.weight).w
        if whole:
            ops.gemm_nt(g, w2, L.PVRL_EPI_RESID_F32, bias=P(blk.mlp.fc2.bias), rowscale=s3_all, aux=x.full, out0=y.full)
        else:           # the patch rows with the stream's residual epilogue; the cls rows are the fp32 chain's below (or their own GEMM)
            ops.gemm_nt(g[:R], w2, self._epi_resid(), bias=P(blk.mlp.fc2.bias), rowscale=s3_all[:R] if s3_all is not None else None,
                        aux=x.p, out0=y.p)
            if not self.cls_fp32:
                ops.gemm_nt(g[R:], w2, L.PVRL_EPI_RESID_F32, bias=P(blk.mlp.fc2.bias), rowscale=s3c, aux=x.c, out0=y.c)
        if self.cls_fp32:       # (the 16-bit path's cls rows of h_m / u / g stay what the backward reads; y's are replaced)
            self._cls_mlp_fp32(blk, x.c, s3c, y.c)
        return y, h_m, (mean_m, rstd_m), u, g

    def _mlp_bwd(self, blk, s, dy, gs):
        """backward of the MLP's two linear layers from dy = 16-bit(s3 * dx): queues their weight gradients -> dh, the gradient of norm2's output"""
        L = lib()
        self._lin_wgrad(gs, dy, s["g"], blk.mlp.fc2)
        du = ops.gemm_nt(dy, self._weight(blk.mlp.fc2.weight).t, L.PVRL_EPI_DGELU, aux=s["u"])
        self._lin_wgrad(gs, du, s["h_m"], blk.mlp.fc1)
        return ops.gemm_nt(du, self._weight(blk.mlp.fc1.weight).t, L.PVRL_EPI_BF16)

    def _block_fwd(self, blk, x0, sv, dp, save, last=False, ckpt=False, recompute=False, tokens=False):
        """`last`: the encoder's last block (with prune_last: the patch rows of x2 / x3 are neither computed nor defined).
        `ckpt` (act_checkpoint, never the last block): the entry saved is x0 and dp alone.  `recompute`: the backward's second pass over
        such a block from that entry -- the full entry again, without the next stage (_mlp_fwd) -> None"""
        prune = last and self.prune_last and not tokens     # (tokens: every row of the last block's output is read)
        keep_u = save and not ckpt
        L = lib()
        B, T, N, R, M = sv["B"], sv["T"], sv["N"], sv["R"], sv["M"]
        C, H = self.C, self.H
        dev = x0.c.device
        split, epi_res = sv["split"], self._epi_resid()
        s1_tok = dp["s1_tok"] if dp else None
        s2_seq = dp["s2_seq"] if dp else None
        s2_tok = dp["s2_tok"] if dp else None
        s3_all = dp["s3_all"] if dp else None
        P = lambda t: t.detach()

        # ---- temporal branch (vit.py:129-135), rows [0, R) ----
        h_t, mean_t, rstd_t = ops.layernorm_fwd(x0.patch(), P(blk.temporal_norm1.weight), P(blk.temporal_norm1.bias), self.eps)
        qkv_t = ops.gemm_nt(h_t, self._weight(blk.temporal_attn.qkv.weight).w, L.PVRL_EPI_BF16,
                            bias=P(blk.temporal_attn.qkv.bias))
        lse_t = None
        if T == 8:
            o_t = ops.attn_t8_fwd(qkv_t, B * N, H, self.scale)
        else:
            o_t, _, lse_t = ops.attn_fwd(qkv_t, B * N, T, H, self.scale, mode=0)
        if split:       # the cls rows pass the temporal branch unchanged: the same tensor (nothing writes a stage's rows twice)
            x1 = _X(torch.empty_like(x0.p), x0.c)
        else:
            x1 = _X.new(R, B, C, dev, False)
        fe = self._fused_temporal(blk)          # proj then temporal_fc as one linear map
        ops.gemm_nt(o_t, fe.w, epi_res, bias=fe.be, rowscale=s1_tok, bias2=P(blk.temporal_fc.bias),
                    aux=x0.p, out0=x1.p)
        if not split:
            x1.c[:] = x0.c

        # ---- spatial branch (vit.py:137-151), all rows; cls of clip b is token 0 of its T sequences ----
        h_s, mean_s, rstd_s = ops.layernorm_fwd(x1.all(), P(blk.norm1.weight), P(blk.norm1.bias), self.eps)
        o_s = torch.empty((R + B * T, C), device=dev, dtype=OP16)
        cls_attn = prune and self.prune_attn
        wqkv = self._weight(blk.attn.qkv.weight).w
        if cls_attn:
            # the last block: only the cls query's output is read (csrc/attn_cls.hip) -- keys and values of every token, queries of the
            # B cls rows; the patch rows' query third of qkv_s and o_s[:R] stay undefined and are never read
            qkv_s = torch.empty((M, 3 * C), device=dev, dtype=OP16)
            self._undef(qkv_s[:R, :C])
            self._undef(o_s[:R])
            bq = P(blk.attn.qkv.bias)
            ops.gemm_nt(h_s, wqkv[C:], L.PVRL_EPI_BF16, bias=bq[C:], out0=qkv_s[:, C:])
            ops.gemm_nt(h_s[R:], wqkv[:C], L.PVRL_EPI_BF16, bias=bq[:C], out0=qkv_s[R:, :C])
            _, lse_s = ops.attn_cls_fwd(qkv_s, B * T, N + 1, H, self.scale, T, R, o_cls=o_s[R:])
        else:
            qkv_s = ops.gemm_nt(h_s, wqkv, L.PVRL_EPI_BF16, bias=P(blk.attn.qkv.bias))
            # (N + 1 tokens per frame: the whole-sequence kernels up to ops.ATTN_MAX_S, the streamed ones for crops above 320^2)
            _, _, lse_s = ops.attn_seq_fwd(qkv_s, B * T, N + 1, H, self.scale, mode=1, T=T, cls_base=R, o=o_s[:R], o_cls=o_s[R:])
        x2 = _X.new(R, B, C, dev, split)      # (pruned last block: its patch rows are neither computed nor defined)
        if prune:
            self._undef(x2.p)
        wproj = self._weight(blk.attn.proj.weight).w
        if not prune:
            ops.gemm_nt(o_s[:R], wproj, epi_res, bias=P(blk.attn.proj.bias), rowscale=s2_tok, aux=x1.p, out0=x2.p)
        if self.cls_fp32:
            # the cls rows' own chain in fp32 on the master weights (csrc/cls_chain.hip): the projection is linear, so the mean over
            # the T frames (vit.py:147-149) is taken first -- B rows instead of B * T
            om = ops.group_reduce(o_s[R:], B, T, scale=s2_seq, alpha=1.0 / T)
            ops.cls_linear(om, P(blk.attn.proj.weight), P(blk.attn.proj.bias), biasscale=dp["s2_mean"] if dp else None,
                           aux=x1.c, out=x2.c)
        else:
            pc = ops.gemm_nt(o_s[R:], wproj, L.PVRL_EPI_F32, bias=P(blk.attn.proj.bias))
            ops.group_reduce(pc, B, T, scale=s2_seq, alpha=1.0 / T, resid=x1.c, out=x2.c)

        # ---- MLP (vit.py:155-157) ----
        if prune:
            # the B cls rows only; h_m / st_m / u / g are then [B, .] tensors (what the backward of this block reads, _block_bwd)
            x3 = _X.new(R, B, C, dev, split)
            self._undef(x3.p)
            s3c = s3_all[R:] if s3_all is not None else None
            h_m = mean_m = rstd_m = u = g = None
            if save or not self.cls_fp32:
                h_m, mean_m, rstd_m = ops.layernorm_fwd(x2.c, P(blk.norm2.weight), P(blk.norm2.bias), self.eps)
                u, g = self._fc1(blk, h_m, keep_u)
            if self.cls_fp32:
                self._cls_mlp_fp32(blk, x2.c, s3c, x3.c)
            else:
                ops.gemm_nt(g, self._weight(blk.mlp.fc2.weight).w, L.PVRL_EPI_RESID_F32, bias=P(blk.mlp.fc2.bias), rowscale=s3c,
                            aux=x2.c, out0=x3.c)
        else:
            x3, h_m, (mean_m, rstd_m), u, g = self._mlp_fwd(blk, x2, s3_all, sv, whole=not split, keep_u=keep_u, recompute=recompute)
        if ckpt:
            sv["blocks"].append(dict(ckpt=True, x0=x0, dp=dp))
        elif save:
            sv["blocks"].append(dict(x0=x0, x1=x1, x2=x2, h_t=h_t, st_t=(mean_t, rstd_t), qkv_t=qkv_t, o_t=o_t,
                                     lse_t=lse_t, h_s=h_s, st_s=(mean_s, rstd_s), qkv_s=qkv_s, o_s=o_s,
                                     lse_s=lse_s, h_m=h_m, st_m=(mean_m, rstd_m), u=u, g=g, dp=dp, pruned=prune, cls_attn=cls_attn))
        return x3

    # ------------------------------------------------------------------ undivided schemes (space_only / joint_space_time)
    def _attn_undivided(self, qkv, B, S, R, o):
        """one sequence per sample: its cls row R + b, then its S - 1 patch rows -- the kernels' mode 1 with T = 1, whose token-0 side
        buffers are then the cls rows of the same matrices.  Up to ops.ATTN_MAX_S tokens the whole-sequence kernels, beyond them the
        streamed ones (ops.attn_family, the one dispatch rule of every scheme)."""
        return ops.attn_seq_fwd(qkv, B, S, self.H, self.scale, mode=1, T=1, cls_base=R, o=o[:R], o_cls=o[R:])[2]

    def _block_fwd_undivided(self, blk, x0, sv, dp, save, ckpt=False, recompute=False):
        """x += dp * proj(attn(norm1(x))); x += dp * mlp(norm2(x))   (Block.forward, vit.py:124-127) on the rows of `_X`.  No pruning of
        the last block; the cls rows' projection and MLP run in fp32 (cls_fp32) as in the divided path.  `ckpt` / `recompute`: _block_fwd"""
        L = lib()
        B, T, N, R, M = sv["B"], sv["T"], sv["N"], sv["R"], sv["M"]
        C = self.C
        dev = x0.c.device
        split, epi_res = sv["split"], self._epi_resid()
        s2_all = dp["s2_all"] if dp else None
        row = lambda s, a, b: s[a:b] if s is not None else None
        P = lambda t: t.detach()

        # ---- attention over all 1 + N * T tokens of a sample ----
        h_s, mean_s, rstd_s = ops.layernorm_fwd(x0.all(), P(blk.norm1.weight), P(blk.norm1.bias), self.eps)
        qkv_s = ops.gemm_nt(h_s, self._weight(blk.attn.qkv.weight).w, L.PVRL_EPI_BF16, bias=P(blk.attn.qkv.bias))
        o_s = torch.empty((M, C), device=dev, dtype=OP16)
        lse_s = self._attn_undivided(qkv_s, B, N * T + 1, R, o_s)
        x1 = _X.new(R, B, C, dev, split)
        wproj = self._weight(blk.attn.proj.weight).w
        ops.gemm_nt(o_s[:R], wproj, epi_res, bias=P(blk.attn.proj.bias), rowscale=row(s2_all, 0, R), aux=x0.p, out0=x1.p)
        if self.cls_fp32:
            ops.cls_linear(o_s[R:].float(), P(blk.attn.proj.weight), P(blk.attn.proj.bias), rowscale=row(s2_all, R, M),
                           biasscale=row(s2_all, R, M), aux=x0.c, out=x1.c)
        else:
            ops.gemm_nt(o_s[R:], wproj, L.PVRL_EPI_RESID_F32, bias=P(blk.attn.proj.bias), rowscale=row(s2_all, R, M), aux=x0.c, out0=x1.c)

        # ---- MLP ----
        x2, h_m, st_m, u, g = self._mlp_fwd(blk, x1, dp["s3_all"] if dp else None, sv, keep_u=save and not ckpt, recompute=recompute)
        if ckpt:
            sv["blocks"].append(dict(ckpt=True, x0=x0, dp=dp))
        elif save:
            sv["blocks"].append(dict(undivided=True, x0=x0, x1=x1, h_s=h_s, st_s=(mean_s, rstd_s), qkv_s=qkv_s, o_s=o_s, lse_s=lse_s,
                                     h_m=h_m, st_m=st_m, u=u, g=g, dp=dp))
        return x2

    def _block_bwd_undivided(self, blk, s, sv, dx, gs, dy, has_prev, prev_dp):
        """backward of _block_fwd_undivided; dy = 16-bit(s3 * dx) [M, C] arrives from the caller, the return value is the same for the
        block in front (or, for block 0, the unscaled 16-bit copy of dx's patch rows for the patch-embedding weight gradient)"""
        L = lib()
        B, T, N, R, M = sv["B"], sv["T"], sv["N"], sv["R"], sv["M"]
        C, H = self.C, self.H
        dev = dx.c.device
        dp = s["dp"]
        s2_all = dp["s2_all"] if dp else None
        row = lambda v, a, b: v[a:b] if v is not None else None

        # ---- MLP ----
        dh = self._mlp_bwd(blk, s, dy, gs)
        dps = torch.empty((M, C), device=dev, dtype=OP16)
        self._lnbwd(gs, dh, s["x1"].all(), s["st_m"], blk.norm2, dx.all(), dx.all(), dxs=dps[:R],
                    dxs_scale=row(s2_all, 0, R))       # also emits 16-bit(s2 * dx[:R])
        ops.cast_scale(dx.c, row(s2_all, R, M), out=dps[R:])

        # ---- attention ----
        self._lin_wgrad(gs, dps, s["o_s"], blk.attn.proj)
        do = ops.gemm_nt(dps, self._weight(blk.attn.proj.weight).t, L.PVRL_EPI_BF16)
        del dps
        S = N * T + 1
        dqkv = torch.empty((M, 3 * C), device=dev, dtype=OP16)
        ops.attn_seq_bwd(s["qkv_s"], s["o_s"][:R], s["o_s"][R:], do[:R], do[R:], s["lse_s"], B, S, H, self.scale, mode=1, T=1, cls_base=R,
                         dqkv=dqkv, dqkv_cls=dqkv[R:])
        self._lin_wgrad(gs, dqkv, s["h_s"], blk.attn.qkv)
        dh = ops.gemm_nt(dqkv, self._weight(blk.attn.qkv.weight).t, L.PVRL_EPI_BF16)
        del dqkv, do
        s3p = prev_dp["s3_all"] if (has_prev and prev_dp) else None
        dy_next = torch.empty((M if has_prev else R, C), device=dev, dtype=OP16)
        self._lnbwd(gs, dh, s["x0"].all(), s["st_s"], blk.norm1, dx.all(), dx.all(), dxs=dy_next[:R], dxs_scale=row(s3p, 0, R))
        if has_prev:
            ops.cast_scale(dx.c, row(s3p, R, M), out=dy_next[R:])
        self.flush_wgrads()
        return dy_next

    # ------------------------------------------------------------------ HIP graphs (GraphReplay)
    def _eager_forward(self, frames, training, save):
        return self._forward(frames, training, None, save, tokens=self._tok)

    def _eager_backward(self, dfeat):
        return self._backward(dfeat)          # (what the saved forward returned decides: sv["tokens"], _bwd_begin)

    def _graph_key(self, frames, training, save):
        m = self.m
        # parameter / gradient storage is baked into a graph: a re-homed parameter (optimizer flat buffer, .to()) is a new key
        return (tuple(frames.shape), frames.dtype, bool(training), bool(save), bool(self.act_checkpoint), frames.device.index, tuple(m.drop_path_rates),
                m.blocks[0].attn.qkv.weight.data_ptr(), m.norm.weight.data_ptr(), self.grad_store().flat.data_ptr(), bool(self._tok))

    def _graph_reset_host_state(self):
        self._wq = []
        self._chain = []
        self._ln_defer = []
        self._fused_fresh = set()

    def _enc_params(self):
        """the parameters whose gradients backward() writes"""
        m = self.m
        ps = [m.cls_token, m.pos_embed] + ([] if self.space_only else [m.time_embed])
        ps += list(m.patch_embed.parameters()) + list(m.norm.parameters())
        for blk in m.blocks:
            ps += list(blk.parameters())
        return [p for p in ps if p.requires_grad]

    # ------------------------------------------------------------------ backward
    def backward(self, dfeat, tokens=False):
        """dfeat fp32 [B, C]: gradient of the loss w.r.t. forward()'s output ([B, 1 + N*T, C] after forward(tokens=True): `tokens` must
        say what the saved forward was).  Writes every encoder parameter gradient into the GradStore views (p.grad) and returns nothing."""
        assert self.saved is not None and bool(self.saved.get("tokens")) == bool(tokens), "backward(tokens=...) does not match the saved forward"
        if self._gkey is not None:
            return self._graph_backward(dfeat)
        return self._backward(dfeat)

    def _backward(self, dfeat):
        st = self._bwd_begin(dfeat)
        nb = len(self.m.blocks)
        for i in range(nb - 1, -1, -1):
            self._bwd_block(st, i)
            lo, hi = self._group_of(i, nb)
            if self.grad_hook is not None and i == lo:
                self._bwd_group_end(st)      # the group's deferred chains / reduces: its blocks' parameter gradients are final now,
                self._run_hooks(range(hi, lo - 1, -1))      # the reducer may start their all-reduce
        self._bwd_end(st)

    def _bwd_group_end(self, st):
        self._finish_deferred(st["gs"])

    # the three stages of backward(); a stage boundary is where the gradient hook may run (and where a staged HIP-graph
    # capture is cut, see _graph_backward)
    def _bwd_begin(self, dfeat):
        m = self.m
        sv = self.saved
        assert sv is not None, "backward() without a saved forward()"
        gs = self.grad_store()
        R, M = sv["R"], sv["M"]
        self._chain = []
        self._ln_defer = []
        self._dwe_rescale = bool(sv.get("tokens"))        # (_temporal_chain_all)
        if SCALED_GRADS:
            dfeat = gs.begin_scaled(dfeat)
        last = len(m.blocks) - 1
        if sv.get("tokens"):
            return self._bwd_begin_tokens(dfeat, sv, gs)
        pruned = bool(sv["blocks"][last].get("pruned"))
        split = sv["split"]
        # the residual gradient stream: zero outside the cls rows until the last block's spatial branch.  Split stream + pruned last
        # block: the patch rows are not even cleared -- the first kernel that would read them (that block's norm1 backward) takes them
        # as zeros (`dxp_zero`)
        dxp_zero = split and pruned
        dx = _X.new(R, M - R, self.C, dfeat.device, split, zero=True, zero_p=not dxp_zero)
        if dxp_zero:
            self._undef(dx.p)
        mean, rstd = sv["norm_stats"]
        (dg, bg), (db, bb) = gs.target(m.norm.weight, fused=True), gs.target(m.norm.bias, fused=True)
        fpc = sv.get("frames_per_clip", 0)
        dxm = torch.empty_like(sv["x_final"].c) if fpc else dx.c
        ops.layernorm_bwd(dfeat.contiguous(), sv["x_final"].c, mean, rstd, m.norm.weight.detach(), dg, db,
                          dx_out=dxm, beta_acc=bg, gscale=gs.inv, nonfinite=gs.bad)
        if fpc:                     # `space_only`: the final norm saw the mean of a clip's frames (vit.py:414-416)
            dx.c.view(-1, fpc, self.C).copy_((dxm / fpc).unsqueeze(1).expand(-1, fpc, -1))
        # dy = bf16(DropPath-scale * dx) is the operand of each block's first backward GEMMs; after the first block it is
        # emitted by the previous block's last LayerNorm-backward kernel instead of a separate cast pass.
        s3 = sv["blocks"][last]["dp"]["s3_all"] if sv["blocks"][last]["dp"] else None
        if pruned:                                # dx is zero outside the cls rows here: the last block's MLP / projection backward
            dy = ops.cast_scale(dx.c, s3[R:] if s3 is not None else None)       # runs on those rows alone (_block_bwd)
        elif split:
            dy = torch.zeros((M, self.C), device=dfeat.device, dtype=OP16)
            ops.cast_scale(dx.c, s3[R:] if s3 is not None else None, out=dy[R:])
        else:
            dy = ops.cast_scale(dx.full, s3)
        return dict(sv=sv, gs=gs, dx=dx, dy=dy, dxp_zero=dxp_zero)

    def _bwd_begin_tokens(self, dtok, sv, gs):
        """_bwd_begin after forward(tokens=True): dtok fp32 [B, 1 + P, C] (in S-scaled units already).  ONE launch
        (pvrl_layernorm_bwd_tokens) reads it in the reference's token order and writes the gradient of every row of the stream and,
        from the same registers, the last block's first operand dy = 16-bit(s3 * dx); norm.weight / norm.bias are sums over all rows."""
        m = self.m
        R, M, C = sv["R"], sv["M"], self.C
        Bp = M - R                      # the stream's cls rows (`space_only`: one per frame)
        dev = dtok.device
        split = sv["split"]
        last = len(m.blocks) - 1
        s3 = sv["blocks"][last]["dp"]["s3_all"] if sv["blocks"][last]["dp"] else None
        mean, rstd = sv["norm_stats"]
        xf = sv["x_final"]
        (dg, bg), (db, _) = gs.target(m.norm.weight, fused=True), gs.target(m.norm.bias, fused=True)
        dtok = dtok.contiguous().view(-1, C)
        dy = torch.empty((M, C), device=dev, dtype=OP16)
        dx = _X.new(R, Bp, C, dev, split)
        fpc = sv.get("frames_per_clip", 0)
        if not fpc:
            ops.layernorm_bwd(dtok, xf.all(), mean, rstd, m.norm.weight.detach(), dg, db, dx_out=dx.all(), beta_acc=bg, gscale=gs.inv,
                              nonfinite=gs.bad, defer=self._ln_defer, dxs=dy, dxs_scale=s3, rows_per_clip=sv["N"] * sv["T"])
            return dict(sv=sv, gs=gs, dx=dx, dy=dy, dxp_zero=False)
        # `space_only`: the norm saw the mean over a clip's frames of every token (vit.py:414-416) -- its gradient, then 1 / T of it to
        # each frame's rows: pvrl_group_bcast_bf16 on the [B * T, N * C] view of the (b, t, n) patch rows, once for the stream's gradient
        # and once with the last block's DropPath factor (one per frame) for dy; the B * T cls rows with torch ops
        B, N = Bp // fpc, sv["N"]
        dxm = torch.empty_like(xf.full)
        ops.layernorm_bwd(dtok, xf.full, mean, rstd, m.norm.weight.detach(), dg, db, dx_out=dxm, beta_acc=bg, gscale=gs.inv,
                          nonfinite=gs.bad, defer=self._ln_defer, rows_per_clip=N)
        dpm = dxm[:B * N].view(B, N * C)
        s3c = s3[R:] if s3 is not None else None
        ops.group_bcast(dpm, B, fpc, scale=s3c, alpha=1.0 / fpc, out=dy[:R].view(Bp, N * C))
        if split:
            ops.group_bcast(dpm, B, fpc, alpha=1.0 / fpc, out=dx.p.view(Bp, N * C))
        else:       # (the fp32 stream of PVRL_RESID16=0, an A/B switch: no fp32 broadcast kernel is kept for it)
            dx.p.view(B, fpc, N * C).copy_((dpm / fpc).unsqueeze(1).expand(-1, fpc, -1))
        dx.c.view(B, fpc, C).copy_((dxm[B * N:] / fpc).unsqueeze(1).expand(-1, fpc, -1))
        ops.cast_scale(dx.c, s3c, out=dy[R:])
        return dict(sv=sv, gs=gs, dx=dx, dy=dy, dxp_zero=False)

    def _recompute(self, blk, s, sv):
        """a checkpointed block's entry (x0, dp) -> the entry a plain forward would have saved: the block's forward once more (the same
        launches on the same operands -- the weight copies and the fused temporal map W_e are the forward's, _weight / _fused_temporal
        -- less what no backward reads, _mlp_fwd).  Inside _bwd_block: stage boundaries and the hook order are the plain backward's."""
        one = dict(sv, blocks=[])
        fwd = self._block_fwd_undivided if self.undivided else self._block_fwd
        fwd(blk, s["x0"], one, s["dp"], True, recompute=True)
        return one["blocks"][0]

    def _bwd_block(self, st, i):
        sv = st["sv"]
        nxt = sv["blocks"][i - 1]["dp"] if i > 0 else None
        s = sv["blocks"][i]
        if s.get("ckpt"):
            s = self._recompute(self.m.blocks[i], s, sv)
        st["dy"] = self._block_bwd(self.m.blocks[i], s, sv, st["dx"], st["gs"], st["dy"], i > 0, nxt,
                                   dxp_zero=st.get("dxp_zero", False))
        del s
        if sv["ckpt"]:
            # What the blocks defer to the end of the backward -- a LayerNorm partial-sum workspace per norm (sized by the grid: 1.8 MB
            # at 784 rows, 4.7 MB at 50k), dW_e / db_e per block -- grows while the saved stages go.  With few rows per step it outweighs
            # them and moves the peak to block 0 (2 clips of 2 x 224^2, depth 4: 82.8 MB instead of 69.0).  This mode pays time for
            # memory: finish the deferred work per block -- the same per-item arithmetic; at the headline shape neither the peak (it is
            # at the first recomputed block) nor the step time moves measurably.
            self._finish_deferred(st["gs"])
        st["dxp_zero"] = False
        sv["blocks"][i] = None  # free activations as we go

    def _bwd_end(self, st):
        # ---- embedding prologue + patch embed (vit.py:174-180, 370-407) ----
        m = self.m
        sv, gs, dx, dy = st["sv"], st["gs"], st["dx"], st["dy"]
        B, T, N, R, C = sv["B"], sv["T"], sv["N"], sv["R"], self.C
        dz = dy[:R]     # block 0's last LayerNorm backward emitted the unscaled bf16 copy of dx[:R]
        w = m.patch_embed.proj.weight
        (dw, bw), (dbias, _) = gs.target(w, fused=True), gs.target(m.patch_embed.proj.bias, fused=True)
        self._wgrad(dz, sv["a_pe"], dw.view(C, -1), dbias, bw, gscale=gs.inv, nonfinite=gs.bad)
        G = ops.batch_sum(dx.p, B, N * T).view(N, T, C)
        dcls_rows = dx.c.sum(0)
        if gs.inv is not None:       # the three small embedding gradients below are sums of these: the scale is taken out here
            G = G * gs.inv           # (a non-finite value in dx reaches the patch-embed weight gradient above, which raises gs.bad)
            dcls_rows = dcls_rows * gs.inv
        # (the three are in true units already, and torch's copy_ / add_ raise no flag: fused, checks=False)
        gs.accumulate(m.cls_token, dcls_rows.view(1, 1, C), fused=True, checks=False)
        dpos = torch.cat([dcls_rows.unsqueeze(0), G.sum(1)], 0)
        dtime = G.sum(0)
        pos_p, tim_p = m.pos_embed, None if self.space_only else m.time_embed
        if pos_p.shape[1] != N + 1 or (tim_p is not None and tim_p.shape[1] != T):
            raise NotImplementedError("training with resized pos/time embeddings is not supported (reference "
                                      "resizes at inference only, vit.py:374)")
        gs.accumulate(pos_p, dpos.unsqueeze(0), fused=True, checks=False)
        if tim_p is not None:
            gs.accumulate(tim_p, dtime.unsqueeze(0), fused=True, checks=False)
        self.flush_wgrads()
        self._finish_deferred(gs)
        if gs.scale is not None:
            gs.end_scaled()
        self.saved = None

    def _block_bwd(self, blk, s, sv, dx, gs, dy, has_prev, prev_dp, dxp_zero=False):
        L = lib()
        B, T, N, R, M = sv["B"], sv["T"], sv["N"], sv["R"], sv["M"]
        C, H = self.C, self.H
        dev = dx.c.device
        if s.get("undivided"):
            return self._block_bwd_undivided(blk, s, sv, dx, gs, dy, has_prev, prev_dp)
        dp = s["dp"]
        s1_tok = dp["s1_tok"] if dp else None
        s2_seq = dp["s2_seq"] if dp else None
        s2_tok = dp["s2_tok"] if dp else None
        s3_all = dp["s3_all"] if dp else None

        if s.get("pruned"):
            # The encoder's last block under prune_last: dx is zero outside the B cls rows (only `x[:, 0]` of the final norm is read,
            # vit.py:418-421), so the MLP, norm2 and the spatial projection back-propagate those rows alone: dy, h_m, u, g are [B, .]
            # tensors here, the weight gradients sums over B (B * T for the projection) rows -- their own small grouped launch: in the
            # block's grouped launch they would force ONE row slice on its 50k-row problems.
            wq = [self._lin_wgrad(gs, dy, s["g"], blk.mlp.fc2, queue=False)]
            du = ops.gemm_nt(dy, self._weight(blk.mlp.fc2.weight).t, L.PVRL_EPI_DGELU, aux=s["u"])
            wq.append(self._lin_wgrad(gs, du, s["h_m"], blk.mlp.fc1, queue=False))
            dh = ops.gemm_nt(du, self._weight(blk.mlp.fc1.weight).t, L.PVRL_EPI_BF16)
            self._lnbwd(gs, dh, s["x2"].c, s["st_m"], blk.norm2, dx.c, dx.c)
            dpc = ops.group_bcast(dx.c, B, T, scale=s2_seq, alpha=1.0 / T)
            wq.append(self._lin_wgrad(gs, dpc, s["o_s"][R:], blk.attn.proj, queue=False))
            if not s.get("cls_attn"):
                ops.gemm_tn_grouped(wq, ws_tag="tn_cls")
            if s.get("cls_attn"):
                do = ops.gemm_nt(dpc, self._weight(blk.attn.proj.weight).t, L.PVRL_EPI_BF16)      # [B * T, C]: the cls queries' dO
            else:
                do = torch.zeros((R + B * T, C), device=dev, dtype=OP16)        # no gradient reaches the patch queries' outputs
                ops.gemm_nt(dpc, self._weight(blk.attn.proj.weight).t, L.PVRL_EPI_BF16, out0=do[R:])
            del du, dpc
        else:
            # ---- MLP ----   (dy = bf16(s3 * dx) arrives from the caller)
            dh = self._mlp_bwd(blk, s, dy, gs)
            dps = torch.empty((R + B * T, C), device=dev, dtype=OP16)
            self._lnbwd(gs, dh, s["x2"].all(), s["st_m"], blk.norm2, dx.all(), dx.all(), dxs=dps[:R], dxs_scale=s2_tok)   # also emits bf16(s2 * dx[:R])

            # ---- spatial ----
            ops.group_bcast(dx.c, B, T, scale=s2_seq, alpha=1.0 / T, out=dps[R:])
            self._lin_wgrad(gs, dps, s["o_s"], blk.attn.proj)
            do = ops.gemm_nt(dps, self._weight(blk.attn.proj.weight).t, L.PVRL_EPI_BF16)
            del dps
        dqkv = torch.empty((M + B * T, 3 * C), device=dev, dtype=OP16)
        if s.get("cls_attn"):
            self._undef(dqkv[:R, :C])
            # dQ is non-zero for the cls rows alone: the query third of dqkv's patch rows is neither written nor read -- the qkv weight
            # gradient's query rows are sums over the B cls rows (into the block's small grouped launch), the data gradient of the patch
            # rows a K = 2 C product
            ops.attn_cls_bwd(s["qkv_s"], s["o_s"][R:], do, s["lse_s"], B * T, N + 1, H, self.scale, T, R, dqkv[:M], dqkv[M:],
                             zero_patch_dq=False)
            ops.group_reduce(dqkv[M:], B, T, out=dqkv[R:M])
            (dw, bw), (dbias, _) = gs.target(blk.attn.qkv.weight, fused=True), gs.target(blk.attn.qkv.bias, fused=True)
            wq.append((dqkv[R:M, :C], s["h_s"][R:], dw[:C], dbias[:C], bw, gs.inv, gs.bad))
            ops.gemm_tn_grouped(wq, ws_tag="tn_cls")
            self._wgrad(dqkv[:M, C:], s["h_s"], dw[C:], dbias[C:], bw, gscale=gs.inv, nonfinite=gs.bad)
            wt = self._weight(blk.attn.qkv.weight).t
            dh = torch.empty((M, C), device=dev, dtype=OP16)
            ops.gemm_nt(dqkv[:R, C:], wt[:, C:], L.PVRL_EPI_BF16, out0=dh[:R])
            ops.gemm_nt(dqkv[R:M], wt, L.PVRL_EPI_BF16, out0=dh[R:])
            del wq
        else:
            ops.attn_seq_bwd(s["qkv_s"], s["o_s"][:R], s["o_s"][R:], do[:R], do[R:], s["lse_s"], B * T, N + 1, H, self.scale,
                             mode=1, T=T, cls_base=R, dqkv=dqkv[:M], dqkv_cls=dqkv[M:])
            ops.group_reduce(dqkv[M:], B, T, out=dqkv[R:M])
            self._lin_wgrad(gs, dqkv[:M], s["h_s"], blk.attn.qkv)
            dh = ops.gemm_nt(dqkv[:M], self._weight(blk.attn.qkv.weight).t, L.PVRL_EPI_BF16)
        del dqkv, do
        # also emits dz = bf16(s1 * dx[:R]) and, into temporal_fc.bias.grad, the unscaled column sums of dx[:R]
        dz = torch.empty((R, C), device=dev, dtype=OP16)
        dbf, bbf = gs.target(blk.temporal_fc.bias, fused=True)
        self._lnbwd(gs, dh, s["x1"].all(), s["st_s"], blk.norm1, dx.all(p_zero=dxp_zero), dx.all(), dxs=dz, dxs_scale=s1_tok, dxsum=dbf,
                    dxsum_beta=bbf)

        # ---- temporal (rows [0, R); cls rows pass straight through): proj + temporal_fc as ONE map W_e (_fused_temporal)
        fe = self._fused_temporal(blk)
        dwe = torch.empty((C, C), device=dev, dtype=F32)
        dbe = torch.empty(C, device=dev, dtype=F32)
        self._wgrad(dz, s["o_t"], dwe, dbe, 0.0)               # the chain runs batched in _finish_deferred (_temporal_chain_all)
        self._chain.append((blk, dwe, dbe))
        dot = ops.gemm_nt(dz, fe.t, L.PVRL_EPI_BF16)
        if T == 8:
            dqkv_t = ops.attn_t8_bwd(s["qkv_t"], dot, B * N, H, self.scale)
        else:
            dqkv_t, _ = ops.attn_bwd(s["qkv_t"], s["o_t"], None, dot, None, s["lse_t"], B * N, T, H, self.scale, mode=0)
        self._lin_wgrad(gs, dqkv_t, s["h_t"], blk.temporal_attn.qkv)
        dh = ops.gemm_nt(dqkv_t, self._weight(blk.temporal_attn.qkv.weight).t, L.PVRL_EPI_BF16)
        # the block's input gradient is final after this kernel: it also emits the bf16 operand of the next stage
        # (previous block's MLP backward with that block's DropPath scale, or the patch-embed weight gradient)
        s3p = prev_dp["s3_all"] if (has_prev and prev_dp) else None
        dy_next = torch.empty((M if has_prev else R, C), device=dev, dtype=OP16)
        self._lnbwd(gs, dh, s["x0"].patch(), s["st_t"], blk.temporal_norm1, dx.patch(), dx.patch(), dxs=dy_next[:R], dxs_scale=s3p)
        if has_prev:
            ops.cast_scale(dx.c, s3p[R:] if s3p is not None else None, out=dy_next[R:])
        self.flush_wgrads()
        return dy_next
