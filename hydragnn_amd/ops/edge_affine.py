"""Pair-affine edge layer: the first layer of EGNN's edge MLP without
the concatenation, closed under differentiation by four primitives.

    edge_pair_affine(P[N, 2H], r2[E], ea[E, D], w_r[H], W_e[H, D], b[H],
                     src, dst) -> z[E, H]
        z[e, f] = P[dst e, f] + P[src e, H + f] + r2[e] w_r[f]
                  + sum_k ea[e, k] W_e[f, k] + b[f]
    pair_affine_node(g[E, H], src, dst) -> dP[N, 2H]
        dP[i, f] = sum_{dst e = i} g[e, f],  dP[j, H + f] = sum_{src e = j} g[e, f]
    pair_affine_edge(g[E, H], w_r[H], W_e[H, D]) -> (dr2[E], dea[E, D])
        dr2[e] = sum_f g[e, f] w_r[f],  dea[e, k] = sum_f g[e, f] W_e[f, k]
    pair_affine_param(g[E, H], r2[E], ea[E, D], bias) -> (dw_r, dW_e, db)
        dw_r[f] = sum_e r2[e] g[e, f],  dW_e[f, k] = sum_e ea[e, k] g[e, f],
        db[f] = sum_e g[e, f]

A layer that is affine in ``cat([h[dst], h[src], r2, ea])`` with weight
``[W_i | W_j | w_r | W_e]`` is ``edge_pair_affine`` of the node-side
product ``P = h [W_i ; W_j]^T``: the per-edge GEMM with K = 2F + 1 + D
becomes a per-node GEMM with K = F, a gather, an add and a rank-(1 + D)
update.

``src`` and ``dst`` are ``SegmentPlan``s (ops/segment_plan.py).  Every
operand group is optional (``P``; ``r2`` with ``w_r``; ``ea`` with
``W_e``; ``b``): an absent group contributes nothing.  Semantics, the
same on the HIP kernels (csrc/edge_affine.hip) and on the pure-torch
doubles below: sums run in the accumulator type (fp32 for
bf16/f16/fp32, fp64 for fp64) in the order written above, k ascending;
every product is rounded to the accumulator type and never fused with
an add; the result is rounded once.  The sums over edges of ``node``
run in ascending edge id; those of ``edge`` and ``param`` in a fixed
order of the kernels' own.

The family is closed under differentiation, so every order stays on
the kernels:

    of fwd,   cotangent g:        node(g), edge(g; w_r, W_e),
                                  param(g; r2, ea)
    of node,  cotangent C:        fwd(P = C)
    of edge,  cotangents c_r, c_e: g: fwd(None, c_r, c_e; w_r, W_e),
                                  parameters: param(g; c_r, c_e), no bias
    of param, cotangents u_r, U_e, u_b:
                                  g: fwd(None, r2, ea; u_r, U_e, u_b),
                                  (r2, ea): edge(g; u_r, U_e)

The kernels serve device tensors of fp32, fp64, bf16 and f16 (all
operands of one dtype) with any H, 0 <= D <= 16 and E < 2^31; E = 0 or
N = 0 launches nothing; nothing syncs with the host.  CPU tensors,
``HYDRAGNN_AMD_FORCE_EAGER=1`` and anything outside that envelope and
the wide one below run the doubles, counted as ``composition``.

Wide edge attributes (csrc/edge_affine_mfma.hip, ``wide_envelope``):
bf16 or f16 with D a multiple of 32 in [32, 128] and H a multiple of 64
in [64, 256] run ``fwd``, ``edge`` and ``param`` on the matrix cores,
the route chosen per call, so the closure table holds for them as well.
Their contract: products of two bf16 or f16 values are exact in fp32;
every sum is in fp32 and rounded once; the order of a D-, H- or E-sum
is the matrix unit's and the tiling's, fixed per (shape, kernel) and
not "k ascending", so results are reproducible run to run and equal the
fp64 result rounded once whenever all partial sums are exact; nothing
syncs with the host, E = 0 launches nothing, every launch is checked.
"""

from __future__ import annotations

import torch

from ._extension import get_extension
from .segment_plan import (PathCounter, SegmentPlan, acc_dtype, check_plans,
                           env_default, kernel_route)

__all__ = ["edge_pair_affine", "pair_affine_node", "pair_affine_edge",
           "pair_affine_param", "torch_edge_pair_affine",
           "torch_pair_affine_node", "torch_pair_affine_edge",
           "torch_pair_affine_param", "fused_egnn", "path_counts",
           "reset_path_counts", "MAX_EDGE_DIM", "wide_envelope"]

MAX_EDGE_DIM = 16

_counts = PathCounter("fwd", "node", "edge", "param", "composition")


def path_counts() -> dict:
    """Launches per primitive (``param`` counts its two kernels as one),
    and calls that ran a torch double instead."""
    return _counts.snapshot()


def reset_path_counts() -> None:
    _counts.reset()


def fused_egnn(default: bool) -> bool:
    """Whether EGNN's edge MLP takes the pair-affine route:
    HYDRAGNN_EGNN_FUSED=0 restores the concatenation, any other value
    selects the fused route, and unset leaves the stack's own default
    (profiles/README.md).  Read at call time."""
    return env_default("HYDRAGNN_EGNN_FUSED", default)


# ---------------------------------------------------------------------------
# pure-torch doubles (differentiable)
# ---------------------------------------------------------------------------
def torch_edge_pair_affine(P, r2, ea, w_r, W_e, b, src=None, dst=None,
                           n_edges=None, like=None):
    ref = next(t for t in (P, r2, ea, b, like) if t is not None)
    acc_t = acc_dtype(ref.dtype)
    acc = None
    if P is not None:
        half = P.shape[1] // 2
        Pa = P.to(acc_t)
        acc = (Pa[:, :half].index_select(0, dst.index)
               + Pa[:, half:].index_select(0, src.index))
    terms = []
    if r2 is not None:
        terms.append(r2.to(acc_t).unsqueeze(1) * w_r.to(acc_t).unsqueeze(0))
    if ea is not None:
        ea_a, We_a = ea.to(acc_t), W_e.to(acc_t)
        terms += [ea_a[:, k:k + 1] * We_a[:, k].unsqueeze(0)
                  for k in range(ea.shape[1])]
    if b is not None:
        terms.append(b.to(acc_t).unsqueeze(0))
    for t in terms:
        acc = t if acc is None else acc + t
    if acc is None or acc.shape[0] != n_edges:
        width = (b if b is not None else w_r if w_r is not None
                 else W_e).shape[0]
        zero = ref.new_zeros(n_edges, width, dtype=acc_t)
        acc = zero if acc is None else acc + zero
    return acc.to(ref.dtype)


def torch_pair_affine_node(g, src: SegmentPlan, dst: SegmentPlan):
    ga = g.to(acc_dtype(g.dtype))
    zero = ga.new_zeros(dst.size, g.shape[1])
    return torch.cat([zero.index_add(0, dst.index, ga),
                      zero.index_add(0, src.index, ga)], dim=1).to(g.dtype)


def torch_pair_affine_edge(g, w_r, W_e):
    acc_t = acc_dtype(g.dtype)
    ga = g.to(acc_t)
    dr2 = None if w_r is None else \
        (ga * w_r.to(acc_t).unsqueeze(0)).sum(1).to(g.dtype)
    dea = None if W_e is None else (ga @ W_e.to(acc_t)).to(g.dtype)
    return dr2, dea


def torch_pair_affine_param(g, r2, ea, bias=True):
    acc_t = acc_dtype(g.dtype)
    ga = g.to(acc_t)
    dwr = None if r2 is None else \
        (r2.to(acc_t).unsqueeze(1) * ga).sum(0).to(g.dtype)
    dWe = None if ea is None else (ga.t() @ ea.to(acc_t)).to(g.dtype)
    db = ga.sum(0).to(g.dtype) if bias else None
    return dwr, dWe, db


# ---------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------
def wide_envelope(dtype: torch.dtype, feat: int, edge_dim: int) -> bool:
    """Whether (dtype, H, D) is served by the MFMA kernels."""
    return (dtype in (torch.bfloat16, torch.float16)
            and edge_dim % 32 == 0 and 32 <= edge_dim <= 128
            and feat % 64 == 0 and 64 <= feat <= 256)


def _kernel_route(t, n_edges, feat, edge_dim) -> bool:
    return kernel_route(t, n_edges) and (
        edge_dim <= MAX_EDGE_DIM or wide_envelope(t.dtype, feat, edge_dim))


def _c(t):
    return None if t is None else t.contiguous()


def _width(t):
    return 0 if t is None else t.shape[1]


class _Fwd(torch.autograd.Function):
    """Kernel route only.  `shape` is (E, H); `like` fixes dtype and
    device when every tensor group but the bias is absent."""

    @staticmethod
    def forward(ctx, P, r2, ea, w_r, W_e, b, src, dst, shape):
        ctx.save_for_backward(r2, ea, w_r, W_e)
        ctx.plans = (src, dst)
        ctx.set_materialize_grads(False)
        like = next(t for t in (P, r2, ea, b) if t is not None)
        _counts.hit("fwd")
        if wide_envelope(like.dtype, shape[1], _width(ea)):
            return get_extension(required=True).pair_affine_wide_fwd(
                P, r2, ea, w_r, W_e, b, None if P is None else dst.index,
                None if P is None else src.index, shape[0], shape[1])
        return get_extension(required=True).pair_affine_fwd(
            P, r2, ea, w_r, None if W_e is None else W_e.t().contiguous(),
            b, None if P is None else dst.index,
            None if P is None else src.index, shape[0], shape[1], like)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 9
        r2, ea, w_r, W_e = ctx.saved_tensors
        src, dst = ctx.plans
        need = ctx.needs_input_grad
        dP = dr2 = dea = dwr = dWe = db = None
        if need[0]:
            dP = pair_affine_node(g, src, dst)
        if need[1] or need[2]:
            dr2, dea = pair_affine_edge(g, w_r if need[1] else None,
                                        W_e if need[2] else None)
        if need[3] or need[4] or need[5]:
            dwr, dWe, db = pair_affine_param(
                g, r2 if need[3] else None, ea if need[4] else None,
                bias=need[5])
        return dP, dr2, dea, dwr, dWe, db, None, None, None


class _Node(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, src, dst):
        ctx.plans = (src, dst)
        ctx.set_materialize_grads(False)
        d_perm, d_rowptr = dst.csr()
        s_perm, s_rowptr = src.csr()
        _counts.hit("node")
        return get_extension(required=True).pair_affine_node(
            g, d_rowptr.contiguous(), _c(d_perm), s_rowptr.contiguous(),
            _c(s_perm), dst.size)

    @staticmethod
    def backward(ctx, C):
        if C is None or not ctx.needs_input_grad[0]:
            return None, None, None
        src, dst = ctx.plans
        return edge_pair_affine(C, None, None, None, None, None, src,
                                dst), None, None


class _Edge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, w_r, W_e):
        ctx.save_for_backward(g, w_r, W_e)
        ctx.set_materialize_grads(False)
        _counts.hit("edge")
        ext = get_extension(required=True)
        call = ext.pair_affine_wide_edge if wide_envelope(
            g.dtype, g.shape[1], _width(W_e)) else ext.pair_affine_edge
        dr2, dea = call(g, w_r,
                        None if W_e is None else W_e.t().contiguous())
        return dr2, dea

    @staticmethod
    def backward(ctx, c_r, c_e):
        g, w_r, W_e = ctx.saved_tensors
        if w_r is None:
            c_r = None
        if W_e is None:
            c_e = None
        if c_r is None and c_e is None:
            return None, None, None
        need = ctx.needs_input_grad
        dg = dwr = dWe = None
        if need[0]:
            dg = edge_pair_affine(
                None, c_r, c_e, None if c_r is None else w_r,
                None if c_e is None else W_e, None, n_edges=g.shape[0])
        if need[1] or need[2]:
            dwr, dWe, _ = pair_affine_param(
                g, c_r if need[1] else None, c_e if need[2] else None,
                bias=False)
        return dg, dwr, dWe


class _Param(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, r2, ea, bias):
        ctx.save_for_backward(g, r2, ea)
        ctx.set_materialize_grads(False)
        _counts.hit("param")
        ext = get_extension(required=True)
        call = ext.pair_affine_wide_param if wide_envelope(
            g.dtype, g.shape[1], _width(ea)) else ext.pair_affine_param
        dwr, dWe, db = call(g, r2, ea, bias)
        return dwr, dWe, db

    @staticmethod
    def backward(ctx, u_r, U_e, u_b):
        g, r2, ea = ctx.saved_tensors
        if r2 is None:
            u_r = None
        if ea is None:
            U_e = None
        if u_r is None and U_e is None and u_b is None:
            return None, None, None, None
        need = ctx.needs_input_grad
        dg = dr2 = dea = None
        if need[0]:
            dg = edge_pair_affine(
                None, None if u_r is None else r2,
                None if U_e is None else ea, u_r, U_e, u_b,
                n_edges=g.shape[0], like=g)
        if (need[1] and u_r is not None) or (need[2] and U_e is not None):
            dr2, dea = pair_affine_edge(g, u_r if need[1] else None,
                                        U_e if need[2] else None)
        return dg, dr2, dea, None


# ---------------------------------------------------------------------------
# public wrappers
# ---------------------------------------------------------------------------
def _same_dtype(ref, **tensors):
    for name, t in tensors.items():
        if t is not None and t.dtype != ref.dtype:
            raise ValueError(f"operands are {ref.dtype} and {name} is "
                             f"{t.dtype}")
        if t is not None and t.device != ref.device:
            raise ValueError(f"operands are on {ref.device} and {name} is "
                             f"on {t.device}")


def _check_g(g):
    if g.dim() != 2:
        raise ValueError(f"g must be [E, H], got {tuple(g.shape)}")
    return g.shape


def _check_edge_groups(n_edges, feat, r2, ea, w_r, W_e):
    """r2 comes back flattened to [E]."""
    if r2 is not None:
        if r2.numel() != n_edges or r2.dim() > 2:
            raise ValueError(f"r2 must be [{n_edges}], got "
                             f"{tuple(r2.shape)}")
        r2 = r2.reshape(n_edges)
        if tuple(w_r.shape) != (feat,):
            raise ValueError(f"w_r must be [{feat}], got "
                             f"{tuple(w_r.shape)}")
    if ea is not None:
        if ea.dim() != 2 or ea.shape[0] != n_edges:
            raise ValueError(f"ea must be [{n_edges}, D], got "
                             f"{tuple(ea.shape)}")
        if tuple(W_e.shape) != (feat, ea.shape[1]):
            raise ValueError(f"W_e must be [{feat}, {ea.shape[1]}], got "
                             f"{tuple(W_e.shape)}")
    return r2


def edge_pair_affine(P, r2, ea, w_r, W_e, b, src: SegmentPlan = None,
                     dst: SegmentPlan = None, n_edges: int = None,
                     like: torch.Tensor = None) -> torch.Tensor:
    """z[E, H].  See the module docstring.  Without ``P`` the plans may
    be left out and ``n_edges`` given instead; ``like`` supplies dtype
    and device when ``b`` is the only operand."""
    ref = next((t for t in (P, r2, ea, b, like) if t is not None), None)
    if ref is None:
        raise ValueError("edge_pair_affine needs at least one operand")
    _same_dtype(ref, P=P, r2=r2, ea=ea, w_r=w_r, W_e=W_e, b=b)
    if (r2 is None) != (w_r is None):
        raise ValueError("r2 and w_r go together")
    if (ea is None) != (W_e is None):
        raise ValueError("ea and W_e go together")
    if P is not None:
        check_plans(src, dst)
        n_edges = src.n_edges
    elif r2 is not None or ea is not None:
        n_edges = (r2 if r2 is not None else ea).shape[0]
    elif n_edges is None:
        raise ValueError("with b alone, n_edges is needed")
    feat = (P.shape[1] // 2 if P is not None else
            next(t for t in (w_r, W_e, b) if t is not None).shape[0])
    if P is not None:
        if P.dim() != 2 or P.shape[1] != 2 * feat:
            raise ValueError(f"P must be [N, 2H], got {tuple(P.shape)}")
        if src.size != P.shape[0] or dst.size != P.shape[0]:
            raise ValueError(f"the plans have {src.size} and {dst.size} "
                             f"rows for {P.shape[0]} nodes")
    r2 = _check_edge_groups(n_edges, feat, r2, ea, w_r, W_e)
    if b is not None and tuple(b.shape) != (feat,):
        raise ValueError(f"b must be [{feat}], got {tuple(b.shape)}")
    if not _kernel_route(ref, n_edges, feat, _width(ea)):
        _counts.hit("composition")
        return torch_edge_pair_affine(P, r2, ea, w_r, W_e, b, src, dst,
                                      n_edges, like)
    if n_edges == 0 or feat == 0 or (P is not None and P.shape[0] == 0) \
            or all(t is None for t in (P, r2, ea, b)):
        return ref.new_zeros(n_edges, feat)
    return _Fwd.apply(_c(P), _c(r2), _c(ea), _c(w_r), _c(W_e), _c(b), src,
                      dst, (n_edges, feat))


def pair_affine_node(g: torch.Tensor, src: SegmentPlan,
                     dst: SegmentPlan) -> torch.Tensor:
    """dP[N, 2H]: the gradient of ``edge_pair_affine`` in ``P``."""
    check_plans(src, dst)
    n_edges, feat = _check_g(g)
    if src.n_edges != n_edges:
        raise ValueError(f"g has {n_edges} rows for {src.n_edges} edges")
    if src.size != dst.size:
        raise ValueError(f"the plans have {src.size} and {dst.size} rows")
    if not _kernel_route(g, n_edges, feat, 0):
        _counts.hit("composition")
        return torch_pair_affine_node(g, src, dst)
    if n_edges == 0 or feat == 0 or dst.size == 0:
        return g.new_zeros(dst.size, 2 * feat)
    return _Node.apply(g.contiguous(), src, dst)


def pair_affine_edge(g: torch.Tensor, w_r, W_e):
    """(dr2[E] | None, dea[E, D] | None): the gradients of
    ``edge_pair_affine`` in ``r2`` and ``ea``; an absent parameter
    leaves its output out."""
    n_edges, feat = _check_g(g)
    _same_dtype(g, w_r=w_r, W_e=W_e)
    if w_r is not None and tuple(w_r.shape) != (feat,):
        raise ValueError(f"w_r must be [{feat}], got {tuple(w_r.shape)}")
    if W_e is not None and (W_e.dim() != 2 or W_e.shape[0] != feat):
        raise ValueError(f"W_e must be [{feat}, D], got "
                         f"{tuple(W_e.shape)}")
    if w_r is None and W_e is None:
        return None, None
    if not _kernel_route(g, n_edges, feat, _width(W_e)):
        _counts.hit("composition")
        return torch_pair_affine_edge(g, w_r, W_e)
    if n_edges == 0 or feat == 0:
        return (None if w_r is None else g.new_zeros(n_edges),
                None if W_e is None else g.new_zeros(n_edges, W_e.shape[1]))
    return _Edge.apply(g.contiguous(), _c(w_r), _c(W_e))


def pair_affine_param(g: torch.Tensor, r2, ea, bias: bool = True):
    """(dw_r[H] | None, dW_e[H, D] | None, db[H] | None): the gradients
    of ``edge_pair_affine`` in its parameters."""
    n_edges, feat = _check_g(g)
    _same_dtype(g, r2=r2, ea=ea)
    if r2 is not None:
        if r2.numel() != n_edges or r2.dim() > 2:
            raise ValueError(f"r2 must be [{n_edges}], got "
                             f"{tuple(r2.shape)}")
        r2 = r2.reshape(n_edges)
    if ea is not None and (ea.dim() != 2 or ea.shape[0] != n_edges):
        raise ValueError(f"ea must be [{n_edges}, D], got "
                         f"{tuple(ea.shape)}")
    if r2 is None and ea is None and not bias:
        return None, None, None
    if not _kernel_route(g, n_edges, feat, _width(ea)):
        _counts.hit("composition")
        return torch_pair_affine_param(g, r2, ea, bias)
    if n_edges == 0 or feat == 0:
        return (None if r2 is None else g.new_zeros(feat),
                None if ea is None else g.new_zeros(feat, ea.shape[1]),
                g.new_zeros(feat) if bias else None)
    return _Param.apply(g.contiguous(), _c(r2), _c(ea), bool(bias))


# `hydragnn_amd.ops.edge_pair_affine` names the function once the
# package has exported it, so the counters are reachable either way
edge_pair_affine.path_counts = path_counts
edge_pair_affine.reset_path_counts = reset_path_counts
