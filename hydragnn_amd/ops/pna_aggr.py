"""Fused PNA aggregation: every aggregator times every degree scaler of
``DegreeScalerAggregation`` in one pass over the CSR rows.

    pna_aggregate(msg[E, F], rowptr[N+1], scale[N, S], aggregators,
                  perm=None) -> out[N, S*A*F]
    pna_scale(rowptr, scalers, avg_deg_lin, avg_deg_log, dtype)
                  -> scale[N, S]

Row ``i`` holds the entries ``rowptr[i]:rowptr[i+1]`` of ``msg``, or of
``perm`` (a stable argsort of an unsorted index) when one is given;
``rowptr[N]`` must equal ``E``.  Column ``(s*A + a)*F + f`` of the
output is aggregator ``a`` of feature ``f`` times scaler ``s``: the
layout of the module's two ``cat``s.

Semantics, the same on the HIP kernels (csrc/pna_aggr.hip) and on the
pure-torch doubles below, with n the row length and every sum in the
accumulator type (fp32 for bf16/f16):

    mu = sum x / n          v = sum (x - mu)^2 / n   (centered)
    var = v                 std = sqrt(v + 1e-5)
    min/max: the lowest position attaining the extreme wins; presence
    is decided by the arg; an empty row gives 0 and arg -1; +-inf count.
    An empty row gives sum = mean = var = 0 and std = sqrt(1e-5).

The accumulator is multiplied by ``scale`` and rounded once.

Orders of differentiation, in the manner of ``varlen_attn``:

* forward: ``pna_fwd`` -> (out, stats = (mu, v), arg = (argmin, argmax));
* first order: ``pna_bwd`` (``_PNAAggrBwd.forward``);
* second order, grad mode off (the ``loss.backward()`` of force
  training): ``pna_bwd2`` -> the gradients with respect to (G, msg);
* third order, or grad mode on inside the second: the torch double of
  the first-order backward, differentiated by autograd.

CPU tensors, ``HYDRAGNN_AMD_FORCE_EAGER=1`` and operands outside the
envelope (dtype other than fp32/fp64/bf16/f16, E >= 2^31, more than 8
scalers) run the pure-torch doubles of the three entry points: indexing
and ``index_add_`` only, no ``bincount``, no host sync.
"""

from __future__ import annotations

from typing import Optional, Sequence

import torch

from ._extension import get_extension, use_eager

__all__ = ["pna_aggregate", "pna_scale", "path_counts",
           "reset_path_counts", "AGGREGATORS", "SCALERS"]

AGGREGATORS = ("sum", "mean", "min", "max", "std", "var")
SCALERS = ("identity", "amplification", "attenuation", "linear",
           "inverse_linear")
STD_EPS = 1e-5
MAX_SCALERS = 8
_SUM, _MEAN, _MIN, _MAX, _STD, _VAR = range(6)
_KERNEL_DTYPES = (torch.float32, torch.float64, torch.bfloat16,
                  torch.float16)

_counts = {"fwd": 0, "bwd": 0, "bwd2": 0, "composition": 0}


def path_counts() -> dict:
    """Fused forward / backward / second-order kernel launches, and
    calls that ran a torch composition instead (the doubles below, the
    third-order fallback, or the module's aggregator-by-aggregator
    path)."""
    return dict(_counts)


def reset_path_counts() -> None:
    for k in _counts:
        _counts[k] = 0


def count_composition() -> None:
    _counts["composition"] += 1


def acc_dtype(dtype: torch.dtype) -> torch.dtype:
    """fp32 for the half types, the dtype itself otherwise."""
    return torch.float32 if dtype in (torch.bfloat16, torch.float16) \
        else dtype


def aggregator_ids(aggregators: Sequence[str]):
    ids = []
    for a in aggregators:
        a = "sum" if a == "add" else a
        if a not in AGGREGATORS:
            raise ValueError(f"unknown aggregator '{a}'")
        ids.append(AGGREGATORS.index(a))
    if not ids or len(set(ids)) != len(ids):
        raise ValueError("aggregators must be a non-empty list without "
                         "repeats")
    return tuple(ids)


def pna_scale(rowptr: torch.Tensor, scalers: Sequence[str], avg_deg_lin,
              avg_deg_log, dtype: torch.dtype) -> torch.Tensor:
    """Per-row scaler factors [N, S] for messages of ``dtype``, in its
    accumulator type, from ``rowptr`` alone with d = clamp(len, 1).
    No sync, no ``bincount``; the factors carry no gradient."""
    acc = acc_dtype(dtype)
    with torch.no_grad():
        d = (rowptr[1:] - rowptr[:-1]).clamp(min=1).to(acc)
        lin = torch.as_tensor(avg_deg_lin, device=rowptr.device).to(acc)
        log = torch.as_tensor(avg_deg_log, device=rowptr.device).to(acc)
        cols = []
        for s in scalers:
            if s == "identity":
                cols.append(torch.ones_like(d))
            elif s == "amplification":
                cols.append((d + 1).log() / log)
            elif s == "attenuation":
                cols.append(log / (d + 1).log())
            elif s == "linear":
                cols.append(d / lin)
            elif s == "inverse_linear":
                cols.append(lin / d)
            else:
                raise ValueError(f"unknown scaler {s}")
        if not cols:
            raise ValueError("at least one scaler")
        return torch.stack(cols, dim=1).contiguous()


# ---------------------------------------------------------------------------
# pure-torch doubles of the three entry points
# ---------------------------------------------------------------------------
def _row_of(rowptr, n_edges):
    """Row of each position 0..E-1; no sync (E is a shape)."""
    pos = torch.arange(n_edges, device=rowptr.device)
    return torch.searchsorted(rowptr[1:].contiguous(), pos, right=True)


def _sorted(t, perm):
    return t if perm is None else t.index_select(0, perm)


def _unsorted(t, perm):
    """Inverse of ``_sorted``: position order back to edge order."""
    if perm is None:
        return t
    inv = torch.empty_like(perm).scatter_(
        0, perm, torch.arange(perm.numel(), device=perm.device))
    return t.index_select(0, inv)


def _lengths(rowptr, acc):
    n = rowptr[1:] - rowptr[:-1]
    return n, n.clamp(min=1).to(acc).unsqueeze(1)


def _seg_sum(t, row, n_rows):
    return t.new_zeros(n_rows, t.shape[1]).index_add_(0, row, t)


def torch_pna_stats(xs, row, d, n_rows):
    """(mu, v) of position-ordered ``xs`` in its dtype; differentiable."""
    mu = _seg_sum(xs, row, n_rows) / d
    y = xs - mu.index_select(0, row)
    return mu, _seg_sum(y * y, row, n_rows) / d


def _extreme(xs, row, n_rows, is_max):
    """Value and arg (position, -1 for an empty row) of the segment
    extreme; the lowest position attaining it wins."""
    n_edges, feat = xs.shape
    fill = float("-inf") if is_max else float("inf")
    idx = row.unsqueeze(1).expand(n_edges, feat)
    val = xs.new_full((n_rows, feat), fill).scatter_reduce(
        0, idx, xs, "amax" if is_max else "amin", include_self=True)
    pos = torch.arange(n_edges, device=xs.device).unsqueeze(1).expand(
        n_edges, feat)
    cand = torch.where(val.index_select(0, row) == xs, pos,
                       torch.full_like(pos, n_edges))
    arg = torch.full((n_rows, feat), n_edges, dtype=torch.long,
                     device=xs.device).scatter_reduce(
        0, idx, cand, "amin", include_self=True)
    present = arg < n_edges
    return (torch.where(present, val, torch.zeros_like(val)),
            torch.where(present, arg, torch.full_like(arg, -1)))


def torch_pna_fwd(msg, rowptr, perm, scale, aggs):
    """Double of ``pna_fwd``: (out, stats [N, F, 2], arg [N, F, 2])."""
    n_rows = rowptr.numel() - 1
    acc = scale.dtype
    xs = _sorted(msg, perm).to(acc)
    n_edges, feat = xs.shape
    row = _row_of(rowptr, n_edges)
    _, d = _lengths(rowptr, acc)
    total = _seg_sum(xs, row, n_rows)
    mu, var = torch_pna_stats(xs, row, d, n_rows)
    arg = torch.full((n_rows, feat, 2), -1, dtype=torch.int32,
                     device=msg.device)
    blocks = []
    for a in aggs:
        if a == _SUM:
            blocks.append(total)
        elif a == _MEAN:
            blocks.append(mu)
        elif a in (_MIN, _MAX):
            val, where = _extreme(xs, row, n_rows, a == _MAX)
            arg[:, :, 0 if a == _MIN else 1] = where.to(torch.int32)
            blocks.append(val)
        elif a == _STD:
            blocks.append(torch.sqrt(var + STD_EPS))
        else:
            blocks.append(var)
    block = torch.stack(blocks, dim=1)                   # [N, A, F]
    out = block.unsqueeze(1) * scale[:, :, None, None]
    return (out.flatten(1).to(msg.dtype),
            torch.stack([mu, var], dim=2), arg)


def _fold(G, scale, aggs, feat):
    """g[a] = sum_s scale[:, s] G[:, s, a, :] per aggregator id."""
    n_rows = scale.shape[0]
    g = (G.to(scale.dtype).view(n_rows, scale.shape[1], len(aggs), feat)
         * scale[:, :, None, None]).sum(1)
    return {a: g[:, k] for k, a in enumerate(aggs)}


def _hit(arg, col, row, n_edges):
    """[E, F] mask of the positions that hold the row's arg."""
    pos = torch.arange(n_edges, device=row.device).unsqueeze(1)
    return arg[:, :, col].to(torch.long).index_select(0, row) == pos


def torch_pna_bwd(msg, rowptr, perm, scale, aggs, stats, arg, G):
    """Double of ``pna_bwd``; differentiable in (msg, G) when ``stats``
    is None (mu and v are then recomputed from ``msg``)."""
    n_rows = rowptr.numel() - 1
    acc = scale.dtype
    xs = _sorted(msg, perm).to(acc)
    n_edges, feat = xs.shape
    row = _row_of(rowptr, n_edges)
    _, d = _lengths(rowptr, acc)
    g = _fold(G, scale, aggs, feat)
    dx = xs.new_zeros(n_edges, feat)
    if _SUM in g:
        dx = dx + g[_SUM].index_select(0, row)
    if _MEAN in g:
        dx = dx + (g[_MEAN] / d).index_select(0, row)
    zero = xs.new_zeros(())
    if _MAX in g:
        dx = dx + torch.where(_hit(arg, 1, row, n_edges),
                              g[_MAX].index_select(0, row), zero)
    if _MIN in g:
        dx = dx + torch.where(_hit(arg, 0, row, n_edges),
                              g[_MIN].index_select(0, row), zero)
    if _STD in g or _VAR in g:
        if stats is None:
            mu, var = torch_pna_stats(xs, row, d, n_rows)
        else:
            mu, var = stats[:, :, 0], stats[:, :, 1]
        k = 0
        if _STD in g:
            k = k + g[_STD] / (d * torch.sqrt(var + STD_EPS))
        if _VAR in g:
            k = k + 2 * g[_VAR] / d
        dx = dx + k.index_select(0, row) * (xs - mu.index_select(0, row))
    return _unsorted(dx, perm).to(msg.dtype).view(msg.shape)


def torch_pna_bwd2(msg, rowptr, perm, scale, aggs, stats, arg, G, c,
                   need_G=True, need_x=True):
    """Double of ``pna_bwd2``: the gradients of R = <c, dx> with respect
    to (G, msg), dx = pna_bwd(...).  With y = x - mu, Cbar = sum c / n,
    Sc = sum c y and sd = sqrt(v + 1e-5):

        dR/dG[i, s, a, f] = scale[i, s] h_a,
          h_sum = sum c, h_mean = Cbar, h_max = c[argmax],
          h_min = c[argmin], h_std = Sc / (n sd), h_var = 2 Sc / n;
        dR/dx_k = g_std / (n sd) [(c_k - Cbar) - Sc y_k / (n sd^2)]
                  + g_var (2 / n) (c_k - Cbar).

    min, max, sum and mean contribute nothing to dR/dx: without std or
    var that gradient is None."""
    n_rows = rowptr.numel() - 1
    acc = scale.dtype
    xs = _sorted(msg, perm).to(acc)
    cs = _sorted(c.reshape(xs.shape), perm).to(acc)
    n_edges, feat = xs.shape
    row = _row_of(rowptr, n_edges)
    _, d = _lengths(rowptr, acc)
    mu, var = stats[:, :, 0], stats[:, :, 1]
    sd = torch.sqrt(var + STD_EPS)
    y = xs - mu.index_select(0, row)
    sum_c = _seg_sum(cs, row, n_rows)
    cbar = sum_c / d
    sc_y = _seg_sum(cs * y, row, n_rows)
    hG = gx = None
    if need_G:
        zero = xs.new_zeros(())
        h = []
        for a in aggs:
            if a == _SUM:
                h.append(sum_c)
            elif a == _MEAN:
                h.append(cbar)
            elif a in (_MIN, _MAX):
                hit = _hit(arg, 0 if a == _MIN else 1, row, n_edges)
                h.append(_seg_sum(torch.where(hit, cs, zero), row, n_rows))
            elif a == _STD:
                h.append(sc_y / (d * sd))
            else:
                h.append(2 * sc_y / d)
        hG = (torch.stack(h, dim=1).unsqueeze(1)
              * scale[:, :, None, None]).flatten(1).to(G.dtype)
    if need_x and (_STD in aggs or _VAR in aggs):
        g = _fold(G, scale, aggs, feat)
        dc = cs - cbar.index_select(0, row)
        gx = xs.new_zeros(n_edges, feat)
        if _STD in g:
            ks = g[_STD] / (d * sd)
            q = sc_y / (d * sd * sd)
            gx = gx + ks.index_select(0, row) * (
                dc - q.index_select(0, row) * y)
        if _VAR in g:
            gx = gx + (2 * g[_VAR] / d).index_select(0, row) * dc
        gx = _unsorted(gx, perm).to(msg.dtype).view(msg.shape)
    return hG, gx


# ---------------------------------------------------------------------------
# dispatch of the three entry points
# ---------------------------------------------------------------------------
def _kernel_route(msg, scale) -> bool:
    return (msg.is_cuda and not use_eager()
            and msg.dtype in _KERNEL_DTYPES
            and msg.shape[0] < 2 ** 31 and msg.shape[0] > 0
            and scale.shape[0] > 0 and scale.shape[1] <= MAX_SCALERS)


def _fwd(msg, rowptr, perm, scale, aggs):
    if _kernel_route(msg, scale):
        _counts["fwd"] += 1
        return get_extension(required=True).pna_fwd(
            msg, rowptr, perm, scale, list(aggs))
    _counts["composition"] += 1
    return torch_pna_fwd(msg, rowptr, perm, scale, aggs)


def _bwd(msg, rowptr, perm, scale, aggs, stats, arg, G):
    if _kernel_route(msg, scale):
        _counts["bwd"] += 1
        return get_extension(required=True).pna_bwd(
            msg, rowptr, perm, scale, list(aggs), stats, arg, G)
    _counts["composition"] += 1
    return torch_pna_bwd(msg, rowptr, perm, scale, aggs, stats, arg, G)


def _bwd2(msg, rowptr, perm, scale, aggs, stats, arg, G, c, need_G,
          need_x):
    if _kernel_route(msg, scale):
        _counts["bwd2"] += 1
        return get_extension(required=True).pna_bwd2(
            msg, rowptr, perm, scale, list(aggs), stats, arg, G, c,
            need_G, need_x)
    _counts["composition"] += 1
    return torch_pna_bwd2(msg, rowptr, perm, scale, aggs, stats, arg, G, c,
                          need_G, need_x)


class _PNAAggr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, msg, rowptr, scale, perm, aggs):
        out, stats, arg = _fwd(msg, rowptr, perm, scale, aggs)
        ctx.save_for_backward(msg, rowptr, scale, perm, stats, arg)
        ctx.aggs = aggs
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, G):
        if G is None:
            return (None,) * 5
        msg, rowptr, scale, perm, stats, arg = ctx.saved_tensors
        dx = _PNAAggrBwd.apply(msg, G.contiguous(), rowptr, scale, perm,
                               stats, arg, ctx.aggs)
        return dx, None, None, None, None


class _PNAAggrBwd(torch.autograd.Function):
    """(msg, G) -> dx on the backward kernel.  Its own backward (the
    double backward) runs the second-order kernel when no third order is
    requested (grad mode off), and otherwise differentiates the torch
    double of the first-order formulas."""

    @staticmethod
    def forward(ctx, msg, G, rowptr, scale, perm, stats, arg, aggs):
        dx = _bwd(msg, rowptr, perm, scale, aggs, stats, arg, G)
        ctx.save_for_backward(msg, G, rowptr, scale, perm, stats, arg)
        ctx.aggs = aggs
        ctx.set_materialize_grads(False)
        return dx

    @staticmethod
    def backward(ctx, c):
        if c is None:
            return (None,) * 8
        msg, G, rowptr, scale, perm, stats, arg = ctx.saved_tensors
        need_x, need_G = ctx.needs_input_grad[:2]
        if not torch.is_grad_enabled():
            hG, gx = _bwd2(msg, rowptr, perm, scale, ctx.aggs, stats, arg,
                           G, c.contiguous(), need_G, need_x)
            return (gx, hG) + (None,) * 6
        # third order: mu and v are recomputed from msg, so autograd
        # sees their dependence; the args are piecewise constant.  G
        # enters as a leaf: its own history is the caller's graph's.
        _counts["composition"] += 1
        with torch.enable_grad():
            x = msg if msg.requires_grad else \
                msg.detach().requires_grad_(True)
            g = G.detach().requires_grad_(True)
            dx = torch_pna_bwd(x, rowptr, perm, scale, ctx.aggs, None, arg,
                               g)
            gx, hG = torch.autograd.grad(dx, (x, g), c, create_graph=True,
                                         allow_unused=True)
        return (gx if need_x else None, hG if need_G else None) \
            + (None,) * 6


def pna_aggregate(msg: torch.Tensor, rowptr: torch.Tensor,
                  scale: torch.Tensor, aggregators: Sequence[str],
                  perm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[N, S*A*F] from msg[E, ...] (trailing dims flattened into F),
    rowptr[N+1] int64, scale[N, S] from ``pna_scale`` and any subset of
    ``AGGREGATORS`` in the given order.  See the module docstring."""
    aggs = aggregator_ids(aggregators)
    if msg.dim() < 2:
        raise ValueError("msg must be [E, F] or [E, ...]")
    acc = acc_dtype(msg.dtype)
    if scale.dim() != 2 or scale.shape[0] != rowptr.numel() - 1:
        raise ValueError("scale must be [N, S]")
    if rowptr.dtype != torch.long:
        raise ValueError("rowptr must be int64")
    if scale.dtype != acc:
        scale = scale.to(acc)
    feat = 1
    for k in msg.shape[1:]:
        feat *= k
    msg2 = msg.reshape(msg.shape[0], feat).contiguous()
    return _PNAAggr.apply(msg2, rowptr.contiguous(),
                          scale.detach().contiguous(), perm, aggs)
