"""Segment-varlen attention for GPS global attention.

Dense-batch attention (reference hydragnn/globalAtt/gps.py:140) pads
every graph to the largest one in the batch; for molecular batches that
wastes both HBM traffic and FLOPs.  The HIP kernels
(csrc/varlen_attn.hip) run one (graph, head) per workgroup with the
other side staged in LDS tiles, over exactly the graph's nodes, for
fp32 or bf16, head_dim <= 128 and any segment length.

Orders of differentiation:

* forward: ``varlen_attention_fwd`` -> (O, LSE), LSE the row
  log-sum-exp of the scaled logits;
* first order: ``varlen_attention_bwd``, two atomic-free passes that
  recompute P from LSE (``_VarlenAttnBwd.forward``) -- no host sync, no
  dense re-padding;
* second order (force-style training): ``varlen_attention_bwd2``, two
  more atomic-free passes (``_VarlenAttnBwd.backward`` with grad mode
  off, the ordinary ``loss.backward()``) -- no host sync either, so the
  whole step captures into a device graph;
* third order, or ``HYDRAGNN_VARLEN_ATTN_BWD2=0``:
  ``_VarlenAttnBwd.backward`` recomputes the attention through a
  pure-torch reference (dense-batch explicit softmax with a finite mask
  bias, query-chunked above 1024 nodes per segment; syncs on the segment
  sizes) and differentiates that twice.

``HYDRAGNN_VARLEN_ATTN_BWD=0`` restores the first-order recompute
backward (the torch reference differentiated once).  On CPU tensors the
same two autograd Functions run on pure-torch doubles of the three entry
points, which is what the autograd-closure tests check without a GPU.
"""

from __future__ import annotations

import math
import os

import torch

from ._extension import get_extension
from ..data import to_dense_batch

MAX_SEG = None  # r2: K/V tiling removed the segment cap
MAX_DH = 128


def torch_varlen_attention_chunked(q, k, v, batch, chunk=512):
    """Per-graph exact attention in query chunks: O(chunk * N_g)
    transient memory instead of the dense [B, maxN, maxN] logits —
    the recompute backward for LARGE segments (the dense reference
    would materialize maxN^2 per graph)."""
    N, H, dh = q.shape
    out = torch.empty_like(q)
    scale = 1.0 / math.sqrt(dh)
    n_graphs = int(batch.max()) + 1 if batch.numel() else 0
    counts = torch.bincount(batch, minlength=n_graphs)
    starts = torch.zeros(n_graphs, dtype=torch.long,
                         device=batch.device)
    if n_graphs > 1:
        starts[1:] = counts.cumsum(0)[:-1]
    for g in range(n_graphs):
        lo, n = int(starts[g]), int(counts[g])
        if n == 0:
            continue
        kg = k[lo:lo + n].transpose(0, 1)          # [H, n, dh]
        vg = v[lo:lo + n].transpose(0, 1)
        for c0 in range(0, n, chunk):
            qg = q[lo + c0:lo + min(c0 + chunk, n)].transpose(0, 1)
            logits = qg @ kg.transpose(-1, -2) * scale
            o = torch.softmax(logits, dim=-1) @ vg  # [H, c, dh]
            out[lo + c0:lo + c0 + o.shape[1]] = o.transpose(0, 1)
    return out


def torch_varlen_attention(q: torch.Tensor, k: torch.Tensor,
                           v: torch.Tensor, batch: torch.Tensor):
    """Reference path: [N, H, dh] q/k/v + per-node graph index ->
    [N, H, dh] via dense-batch masked SDPA."""
    N, H, dh = q.shape
    x = torch.cat([q, k, v], dim=1).reshape(N, 3 * H * dh)
    xd, mask = to_dense_batch(x, batch)
    B, Nmax = mask.shape
    qd, kd, vd = xd.view(B, Nmax, 3, H, dh).permute(2, 0, 3, 1, 4)
    # explicit softmax attention (not SDPA): double-differentiable on
    # every backend, which the recompute backward relies on; finite
    # mask bias keeps padded rows NaN-free
    bias = torch.where(mask.view(B, 1, 1, Nmax), 0.0, -1e9).to(q.dtype)
    logits = qd @ kd.transpose(-1, -2) / math.sqrt(dh) + bias
    out = torch.softmax(logits, dim=-1) @ vd
    out = out.permute(0, 2, 1, 3)  # [B, Nmax, H, dh]
    return out[mask]


def _segments(ptr):
    p = ptr.tolist()
    return [(lo, hi) for lo, hi in zip(p[:-1], p[1:]) if hi > lo]


def torch_varlen_attention_fwd(q, k, v, ptr):
    """Pure-torch double of the ``varlen_attention_fwd`` entry point:
    (O [N, H, dh], LSE [N, H]) per segment of the rowptr ``ptr``; LSE
    in q's dtype (the kernel's is fp32)."""
    N, H, dh = q.shape
    scale = 1.0 / math.sqrt(dh)
    out = torch.empty_like(q)
    lse = q.new_empty(N, H)
    for lo, hi in _segments(ptr):
        qg, kg, vg = (t[lo:hi].transpose(0, 1) for t in (q, k, v))
        s = qg @ kg.transpose(-1, -2) * scale        # [H, n, n]
        ls = torch.logsumexp(s, dim=-1)              # [H, n]
        out[lo:hi] = (torch.exp(s - ls[..., None]) @ vg).transpose(0, 1)
        lse[lo:hi] = ls.transpose(0, 1)
    return out, lse


def torch_varlen_attention_bwd(q, k, v, out, lse, dout, ptr):
    """Pure-torch double of the ``varlen_attention_bwd`` entry point:
    with s = scale q k^T, P = exp(s - LSE), D = rowsum(dO * O),
    dV = P^T dO, dS = P (dO V^T - D), dQ = scale dS K,
    dK = scale dS^T Q, per segment."""
    N, H, dh = q.shape
    scale = 1.0 / math.sqrt(dh)
    dq, dk, dv = (torch.empty_like(t) for t in (q, k, v))
    for lo, hi in _segments(ptr):
        qg, kg, vg, og, gg = (t[lo:hi].transpose(0, 1)
                              for t in (q, k, v, out, dout))
        p = torch.exp(qg @ kg.transpose(-1, -2) * scale
                      - lse[lo:hi].transpose(0, 1)[..., None])
        d = (gg * og).sum(-1, keepdim=True)          # [H, n, 1]
        ds = p * (gg @ vg.transpose(-1, -2) - d)
        dv[lo:hi] = (p.transpose(-1, -2) @ gg).transpose(0, 1)
        dq[lo:hi] = (ds @ kg).transpose(0, 1) * scale
        dk[lo:hi] = (ds.transpose(-1, -2) @ qg).transpose(0, 1) * scale
    return dq, dk, dv


def torch_varlen_attention_bwd2(q, k, v, out, lse, dout, cq, ck, cv, ptr):
    """Pure-torch double of the ``varlen_attention_bwd2`` entry point:
    the gradients of R = <cq, dQ> + <ck, dK> + <cv, dV> with respect to
    (q, k, v, dO), where (dQ, dK, dV) = varlen_attention_bwd(...) and
    ``out``/``lse`` are functions of (q, k, v) that get no gradient of
    their own.  A cotangent given as None is zero.  Per segment, with
    s = scale q k^T, P = exp(s - LSE), a = dO V^T, D = rowsum(dO * O),
    T = scale (cq k^T + q ck^T), W = dO cv^T:

        t = rowsum(P T), u = rowsum(P T a), w = rowsum(P W),
        e = u - 2 t D + w,
        E = (T - t) a - D T + W,  GS = P (E - e),  dS = P (a - D),
        g_dO = P (T - t) V + P cv,        g_v = (P (T - t))^T dO,
        g_q = scale (GS K + dS ck),       g_k = scale (GS^T Q + dS^T cq).
    """
    N, H, dh = q.shape
    scale = 1.0 / math.sqrt(dh)
    cq, ck, cv = (torch.zeros_like(q) if c is None else c
                  for c in (cq, ck, cv))
    gq, gk, gv, gg = (torch.empty_like(q) for _ in range(4))
    for lo, hi in _segments(ptr):
        qg, kg, vg, og, dg, cqg, ckg, cvg = (
            t[lo:hi].transpose(0, 1)
            for t in (q, k, v, out, dout, cq, ck, cv))
        kt = kg.transpose(-1, -2)
        p = torch.exp(qg @ kt * scale
                      - lse[lo:hi].transpose(0, 1)[..., None].to(q.dtype))
        a = dg @ vg.transpose(-1, -2)
        d = (dg * og).sum(-1, keepdim=True)
        tt = (cqg @ kt + qg @ ckg.transpose(-1, -2)) * scale
        w = dg @ cvg.transpose(-1, -2)
        t = (p * tt).sum(-1, keepdim=True)
        e = (p * tt * a).sum(-1, keepdim=True) - 2 * t * d \
            + (p * w).sum(-1, keepdim=True)
        ptc = p * (tt - t)
        gs = p * ((tt - t) * a - d * tt + w - e)
        ds = p * (a - d)
        gg[lo:hi] = (ptc @ vg + p @ cvg).transpose(0, 1)
        gv[lo:hi] = (ptc.transpose(-1, -2) @ dg).transpose(0, 1)
        gq[lo:hi] = (gs @ kg + ds @ ckg).transpose(0, 1) * scale
        gk[lo:hi] = (gs.transpose(-1, -2) @ qg
                     + ds.transpose(-1, -2) @ cqg).transpose(0, 1) * scale
    return gq, gk, gv, gg


def varlen_tiling(head_dim: int):
    """(tile rows T, rows per workgroup pass B) of the kernel instance
    that serves ``head_dim``."""
    t, b = get_extension(required=True).varlen_attention_tiling(head_dim)
    return t, b


def varlen_tiling2(head_dim: int):
    """The same for the second-order instance that serves ``head_dim``."""
    t, b = get_extension(required=True).varlen_attention_tiling2(head_dim)
    return t, b


def _kernel_backward_enabled() -> bool:
    return os.environ.get("HYDRAGNN_VARLEN_ATTN_BWD", "1") != "0"


def _kernel_second_order_enabled() -> bool:
    return os.environ.get("HYDRAGNN_VARLEN_ATTN_BWD2", "1") != "0"


def _recompute_out(q, k, v, batch):
    """The double-differentiable torch recompute of the attention
    (syncs on the segment sizes to pick the bounded-memory path)."""
    max_seg = int(torch.bincount(batch).max()) if batch.numel() else 0
    if max_seg > 1024:
        # dense recompute would materialize maxN^2 logits per
        # graph; chunked exact path keeps memory bounded
        return torch_varlen_attention_chunked(q, k, v, batch)
    return torch_varlen_attention(q, k, v, batch)


class _VarlenAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, ptr, batch):
        if q.is_cuda:
            ext = get_extension(required=True)
            out, lse = ext.varlen_attention_fwd(
                q.contiguous(), k.contiguous(), v.contiguous(), ptr)
        else:
            out, lse = torch_varlen_attention_fwd(q, k, v, ptr)
        ctx.save_for_backward(q, k, v, out, lse, ptr, batch)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g):
        # the double backward reaches this node a second time through
        # the saved ``out``, which gets no gradient there: without this
        # the engine would hand in zeros and the first-order kernels
        # would run once more for nothing
        if g is None:
            return (None,) * 5
        q, k, v, out, lse, ptr, batch = ctx.saved_tensors
        if _kernel_backward_enabled():
            dq, dk, dv = _VarlenAttnBwd.apply(
                q, k, v, out, lse, g.contiguous(), ptr, batch)
            return dq, dk, dv, None, None
        # recompute through the torch reference, differentiating w.r.t.
        # the SAVED tensors (not detached copies) so the second-order
        # graph stays connected for force-style double backward
        need = ctx.needs_input_grad[:3]
        with torch.enable_grad():
            ref = _recompute_out(q, k, v, batch)
            inputs = [t for t, n in zip((q, k, v), need) if n]
            grads = iter(torch.autograd.grad(
                ref, inputs, g, create_graph=torch.is_grad_enabled(),
                allow_unused=True))
        res = [next(grads) if n else None for n in need]
        return res[0], res[1], res[2], None, None


class _VarlenAttnBwd(torch.autograd.Function):
    """(q, k, v, out, lse, g) -> (dq, dk, dv) on the backward kernels.
    Its own backward (the double backward) runs the second-order
    kernels when no third order is requested (grad mode off, the
    ordinary ``loss.backward()`` of force training), and the torch
    recompute otherwise."""

    @staticmethod
    def forward(ctx, q, k, v, out, lse, g, ptr, batch):
        if q.is_cuda:
            ext = get_extension(required=True)
            dq, dk, dv = ext.varlen_attention_bwd(
                q.contiguous(), k.contiguous(), v.contiguous(),
                out, lse, g, ptr)
        else:
            dq, dk, dv = torch_varlen_attention_bwd(
                q, k, v, out, lse, g, ptr)
        ctx.save_for_backward(q, k, v, g, batch, out, lse, ptr)
        ctx.set_materialize_grads(False)
        return dq, dk, dv

    @staticmethod
    def _kernel_route(q) -> bool:
        if torch.is_grad_enabled() or not _kernel_second_order_enabled():
            return False
        return not q.is_cuda or q.dtype in (torch.float32, torch.bfloat16)

    @staticmethod
    def backward(ctx, *cots):
        if all(c is None for c in cots):
            return (None,) * 8
        if _VarlenAttnBwd._kernel_route(ctx.saved_tensors[0]):
            # out and lse are functions of (q, k, v) and get no gradient
            # of their own, as below; an absent cotangent is a zero
            # tensor, so the kernels carry no optional operands
            q, k, v, g, _, out, lse, ptr = ctx.saved_tensors
            cq, ck, cv = (torch.zeros_like(q) if c is None
                          else c.contiguous() for c in cots)
            if q.is_cuda:
                ext = get_extension(required=True)
                gq, gk, gv, gg = ext.varlen_attention_bwd2(
                    q.contiguous(), k.contiguous(), v.contiguous(), out,
                    lse, g, cq, ck, cv, ptr)
            else:
                gq, gk, gv, gg = torch_varlen_attention_bwd2(
                    q, k, v, out, lse, g, cq, ck, cv, ptr)
            return gq, gk, gv, None, None, gg, None, None
        # out and lse are functions of (q, k, v): the recompute below
        # carries that dependence, so they get no gradient of their own.
        # The cotangent g enters as a fresh leaf -- its own history
        # (e.g. g = 2 * out) is differentiated by the caller's graph
        # from the gradient returned for it here, not a second time
        # inside this recompute.
        *qkv, g, batch = ctx.saved_tensors[:5]
        pairs = [(i, c) for i, c in enumerate(cots) if c is not None]
        with torch.enable_grad():
            g = g.detach().requires_grad_(True)
            # an operand outside the caller's graph still has to be
            # differentiated once to form the first-order gradients
            qkv = [t if t.requires_grad else
                   t.detach().requires_grad_(True) for t in qkv]
            ref = _recompute_out(*qkv, batch)
            first = torch.autograd.grad(
                ref, [qkv[i] for i, _ in pairs], g, create_graph=True)
            gq, gk, gv, gg = torch.autograd.grad(
                first, (*qkv, g), [c for _, c in pairs],
                create_graph=torch.is_grad_enabled(), allow_unused=True)
        return gq, gk, gv, None, None, gg, None, None


def varlen_attention_fn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                        ptr: torch.Tensor, batch: torch.Tensor):
    """Attention through the autograd Function pair on any device:
    HIP kernels for GPU tensors (fp32/bf16 native, other dtypes via
    fp32), their pure-torch doubles for CPU tensors."""
    if q.is_cuda and q.dtype not in (torch.float32, torch.bfloat16):
        orig_dtype = q.dtype
        q, k, v = (t.float() for t in (q, k, v))
        return _VarlenAttn.apply(q, k, v, ptr, batch).to(orig_dtype)
    return _VarlenAttn.apply(q, k, v, ptr, batch)


def varlen_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                     ptr: torch.Tensor, batch: torch.Tensor):
    """[N, H, dh] q/k/v, graph rowptr [G+1] and per-node graph index
    [N] -> [N, H, dh].  HIP kernels on GPU (fp32 or bf16, head_dim <=
    128, forward, first- and second-order backward), torch reference on
    CPU."""
    if not q.is_cuda:
        return torch_varlen_attention(q, k, v, batch)
    return varlen_attention_fn(q, k, v, ptr, batch)


def varlen_eligible(head_dim: int, max_seg: int, device) -> bool:
    if os.environ.get("HYDRAGNN_VARLEN_ATTN", "1") == "0":
        return False
    if not (isinstance(device, torch.device) and device.type == "cuda"):
        return False
    return head_dim <= MAX_DH
