"""Fused PaiNN message: the gated vector message of PaiNN and PNAEq in
one launch, and its first-order gradients in two.

    painn_message(phi[N, 3F], w[E, 3F], v[N, 3, F], u[E, 3], src, dst,
                  scalar=True) -> (ds[N, F] | None, dv[N, 3, F])

With ``j = src.index[e]``, ``i = dst.index[e]`` and blocks 0, 1, 2 of
the 3F axis in the order of the models' ``torch.split`` (gate on the
source vector, gate on the edge direction, scalar message):

    dv[i, d, f] = sum_{e -> i} ((w0[e, f] phi0[j, f]) v[j, d, f]
                                + (w1[e, f] phi1[j, f]) u[e, d])
    ds[i, f]    = sum_{e -> i}   w2[e, f] phi2[j, f]

``src`` and ``dst`` are ``SegmentPlan``s (ops/segment_plan.py).  The
semantics are those of ``gather_mul_sum``: the sum runs in ascending
edge id within a row, from 0, in the accumulator type (fp32 for
bf16/f16/fp32, fp64 for fp64); every product is rounded to the
accumulator type, associates as the parentheses show and is never fused
with an add; the result is rounded once; an empty row gives 0; indices
outside their range are unspecified.  In fp32 and fp64 on a dst-sorted
index the forward equals, bit for bit, the composition of ``gather``,
broadcast products and ``scatter(..., sorted_index=True)`` it replaces.

The kernels (csrc/painn_message.hip) serve device tensors of fp32,
fp64, bf16 and f16 with E < 2^31; E = 0 or N = 0 launches nothing.  CPU
tensors, ``HYDRAGNN_AMD_FORCE_EAGER=1`` and anything outside that
envelope run the pure-torch doubles below, written on ``gather`` and
``scatter`` so that their own autograd stays on the existing kernels.

First order is fused: ``bwd_node`` (dphi, dv, over the src plan's CSR,
built at the first backward) and ``bwd_edge`` (dw, du).  The second
order, which a force loss needs, differentiates the backward double
under ``enable_grad``: unfused, on the gather / scatter kernels, and
counted as ``composition``.
"""

from __future__ import annotations

import torch

from ._extension import get_extension
from .scatter import gather, scatter
from .segment_plan import (PathCounter, SegmentPlan, acc_dtype, check_plans,
                           env_default, kernel_route)

__all__ = ["painn_message", "torch_painn_message",
           "torch_painn_message_bwd", "fused_painn", "path_counts",
           "reset_path_counts"]

_counts = PathCounter("fwd", "bwd_node", "bwd_edge", "composition")


def path_counts() -> dict:
    """Launches of the three kernels, and calls that ran a torch double
    instead (the second order among them)."""
    return _counts.snapshot()


def reset_path_counts() -> None:
    _counts.reset()


def fused_painn(default: bool) -> bool:
    """Whether a model stack takes the fused message:
    HYDRAGNN_PAINN_FUSED=0 restores the composition of generic ops, any
    other value selects the fused route, and unset leaves the stack's
    own default (profiles/README.md).  Read at call time."""
    return env_default("HYDRAGNN_PAINN_FUSED", default)


# ---------------------------------------------------------------------------
# pure-torch doubles
# ---------------------------------------------------------------------------
def _gather(x, plan: SegmentPlan):
    csr = None
    if x.is_cuda and not plan.sorted_index:
        csr = plan.csr()
    return gather(x, plan.index, backward_csr=csr)


def _scatter(x, plan: SegmentPlan):
    if plan.sorted_index or not x.is_cuda:
        return scatter(x, plan.index, plan.size, "sum",
                       sorted_index=plan.sorted_index)
    return scatter(x, plan.index, plan.size, "sum", csr=plan.csr())


def torch_painn_message(phi, w, v, u, src: SegmentPlan, dst: SegmentPlan,
                        scalar: bool = True):
    """(ds | None, dv): the products and sums of the kernel, in the
    accumulator type, one cast."""
    n, _, feat = v.shape
    acc = acc_dtype(phi.dtype)
    gate = w.to(acc) * _gather(phi.to(acc), src)
    g0, g1, g2 = torch.split(gate, feat, dim=1)
    vj = _gather(v.to(acc).reshape(n, 3 * feat), src).view(-1, 3, feat)
    msg = vj * g0.unsqueeze(1) + g1.unsqueeze(1) * u.to(acc).unsqueeze(-1)
    dv = _scatter(msg.reshape(-1, 3 * feat), dst).view(n, 3, feat)
    ds = _scatter(g2, dst).to(phi.dtype) if scalar else None
    return ds, dv.to(phi.dtype)


def torch_painn_message_bwd(phi, w, v, u, gs, gv, src: SegmentPlan,
                            dst: SegmentPlan):
    """(dphi, dw, dv_in, du) for the cotangents gs[N, F] | None and
    gv[N, 3, F]: the formulas of the two backward kernels, differentiable
    in all six tensors."""
    n, _, feat = v.shape
    acc = acc_dtype(phi.dtype)
    w0, w1, w2 = torch.split(w.to(acc), feat, dim=1)
    p0, p1, p2 = torch.split(_gather(phi.to(acc), src), feat, dim=1)
    vj = _gather(v.to(acc).reshape(n, 3 * feat), src).view(-1, 3, feat)
    gi = _gather(gv.to(acc).reshape(n, 3 * feat), dst).view(-1, 3, feat)
    ua = u.to(acc)
    sv = (gi * vj).sum(1)                         # sum_d gv[i, d] v[j, d]
    su = (gi * ua.unsqueeze(-1)).sum(1)           # sum_d gv[i, d] u[e, d]
    gsi = _gather(gs.to(acc), dst) if gs is not None \
        else torch.zeros_like(sv)
    dw = torch.cat([p0 * sv, p1 * su, p2 * gsi], dim=1)
    dphi = _scatter(torch.cat([w0 * sv, w1 * su, w2 * gsi], dim=1), src)
    dv_in = _scatter(((w0 * p0).unsqueeze(1) * gi).reshape(-1, 3 * feat),
                     src).view(n, 3, feat)
    du = (gi * (w1 * p1).unsqueeze(1)).sum(-1)
    return tuple(t.to(phi.dtype) for t in (dphi, dw, dv_in, du))


# ---------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------
def _nothing(phi, w) -> bool:
    return w.shape[0] == 0 or phi.shape[0] == 0 or phi.shape[1] == 0


class _PainnMessage(torch.autograd.Function):
    """Kernel route only; v is [N, 3F] here and dv comes back so."""

    @staticmethod
    def forward(ctx, phi, w, v, u, src, dst, scalar):
        ctx.save_for_backward(phi, w, v, u)
        ctx.plans = (src, dst)
        ctx.set_materialize_grads(False)
        feat = phi.shape[1] // 3
        if _nothing(phi, w):
            dv = phi.new_zeros(phi.shape[0], 3 * feat)
            return (phi.new_zeros(phi.shape[0], feat) if scalar else None), dv
        perm, rowptr = dst.csr()
        _counts.hit("fwd")
        ds, dv = get_extension(required=True).painn_msg_fwd(
            phi, w, v, u, src.index, rowptr, perm, scalar)
        return ds, dv

    @staticmethod
    def backward(ctx, gs, gv):
        if gs is None and gv is None:
            return (None,) * 7
        phi, w, v, u = ctx.saved_tensors
        if gv is None:
            gv = torch.zeros_like(v)
        grads = _PainnMessageBwd.apply(phi, w, v, u, gs, gv, *ctx.plans,
                                       tuple(ctx.needs_input_grad[:4]))
        return grads + (None, None, None)


class _PainnMessageBwd(torch.autograd.Function):
    """(dphi, dw, dv_in, du) from the two backward kernels; `need`
    masks them.  Its own backward differentiates the torch double."""

    @staticmethod
    def forward(ctx, phi, w, v, u, gs, gv, src, dst, need):
        ctx.save_for_backward(phi, w, v, u, gs, gv)
        ctx.plans = (src, dst)
        ctx.need = need
        ctx.set_materialize_grads(False)
        gv = gv.contiguous()
        if gs is not None:
            gs = gs.contiguous()
        dphi = dw = dv_in = du = None
        if _nothing(phi, w):
            outs = (torch.zeros_like(phi), torch.zeros_like(w),
                    torch.zeros_like(v), torch.zeros_like(u))
            return tuple(t if k else None for t, k in zip(outs, need))
        ext = get_extension(required=True)
        if need[0] or need[2]:
            perm, rowptr = src.csr()
            _counts.hit("bwd_node")
            dphi, dv_in = ext.painn_msg_bwd_node(
                phi, w, v, u, gs, gv, dst.index, rowptr, perm, need[0],
                need[2])
        if need[1] or need[3]:
            _counts.hit("bwd_edge")
            dw, du = ext.painn_msg_bwd_edge(
                phi, w, v, u, gs, gv, src.index, dst.index, need[1], need[3])
        return dphi, dw, dv_in, du

    @staticmethod
    def backward(ctx, *cot):
        src, dst = ctx.plans
        saved = ctx.saved_tensors
        feat = saved[0].shape[1] // 3
        picked = [k for k in range(4) if ctx.need[k] and cot[k] is not None]
        wanted = [k for k in range(6)
                  if ctx.needs_input_grad[k] and saved[k] is not None]
        grads = [None] * 6
        if picked and wanted:
            _counts.hit("composition")
            create = torch.is_grad_enabled()
            with torch.enable_grad():
                # aliases: the cotangents are themselves functions of
                # the operands, and the partial derivatives wanted here
                # must stop at this call's own arguments
                saved = [None if t is None else t.view_as(t) for t in saved]
                phi, w, v, u, gs, gv = saved
                outs = torch_painn_message_bwd(
                    phi, w, v.view(-1, 3, feat), u, gs,
                    gv.view(-1, 3, feat), src, dst)
                outs = (outs[0], outs[1], outs[2].reshape(-1, 3 * feat),
                        outs[3])
                got = torch.autograd.grad(
                    [outs[k] for k in picked], [saved[k] for k in wanted],
                    [cot[k] for k in picked], allow_unused=True,
                    create_graph=create)
            for k, g in zip(wanted, got):
                grads[k] = g
        return tuple(grads) + (None, None, None)


def painn_message(phi: torch.Tensor, w: torch.Tensor, v: torch.Tensor,
                  u: torch.Tensor, src: SegmentPlan, dst: SegmentPlan,
                  scalar: bool = True):
    """(ds[N, F] | None, dv[N, 3, F]).  See the module docstring."""
    check_plans(src, dst)
    if v.dim() != 3 or v.shape[1] != 3:
        raise ValueError(f"v must be [N, 3, F], got {tuple(v.shape)}")
    n, _, feat = v.shape
    n_edges = src.n_edges
    for name, t in (("w", w), ("v", v), ("u", u)):
        if t.dtype != phi.dtype:
            raise ValueError(f"phi is {phi.dtype} and {name} is {t.dtype}")
    if tuple(phi.shape) != (n, 3 * feat):
        raise ValueError(f"phi must be [{n}, {3 * feat}], got "
                         f"{tuple(phi.shape)}")
    if tuple(w.shape) != (n_edges, 3 * feat):
        raise ValueError(f"w must be [{n_edges}, {3 * feat}], got "
                         f"{tuple(w.shape)}")
    if tuple(u.shape) != (n_edges, 3):
        raise ValueError(f"u must be [{n_edges}, 3], got {tuple(u.shape)}")
    if src.size != n or dst.size != n:
        raise ValueError(f"the plans have {src.size} and {dst.size} rows "
                         f"for {n} nodes")
    if not kernel_route(phi, n_edges):
        _counts.hit("composition")
        return torch_painn_message(phi, w, v, u, src, dst, scalar)
    ds, dv = _PainnMessage.apply(
        phi.contiguous(), w.contiguous(),
        v.reshape(n, 3 * feat).contiguous(), u.contiguous(), src, dst,
        bool(scalar))
    return ds, dv.view(n, 3, feat)


# `hydragnn_amd.ops.painn_message` names this function once the package
# has exported it, so the counters are reachable through either spelling
painn_message.path_counts = path_counts
painn_message.reset_path_counts = reset_path_counts
