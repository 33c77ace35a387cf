"""Fused gather-multiply-sum: the continuous-filter message of SchNet's
``CFConv`` and of both DimeNet++ aggregations, closed under
differentiation by two primitives.

    gather_mul_sum(x[M, ...], w[E, ...], src, dst) -> out[dst.size, ...]
        out[i, f] = sum_{e : dst.index[e] = i} x[src.index[e], f] w[e, f]
    gather_mul(a[M, ...], b[N, ...], src, dst) -> out[E, ...]
        out[e, f] = a[src.index[e], f] b[dst.index[e], f]

``src`` and ``dst`` are ``SegmentPlan``s: one grouping each of the E
edges into ``size`` rows, with a lazily built and cached CSR
``(perm | None, rowptr)``.  Trailing dims are flattened into F.

Semantics, the same on the HIP kernels (csrc/gather_mul.hip) and on the
pure-torch doubles below: the sum runs in ascending edge id within a
row, in the accumulator type (fp32 for bf16/f16/fp32, fp64 for fp64);
each product is rounded to the accumulator type and then added (no
fused multiply-add), and the result is rounded once.  For fp32/fp64 the
op therefore equals, bit for bit, the fixed-order composition
``scatter(gather(x, src) * w, dst, csr=...)``; for the half types it
skips the composition's rounding of every product.  An empty row gives
0.  Indices outside their range are unspecified.

The operation is bilinear, and its gradients are the two primitives
again on the transposed grouping, so every order of differentiation
stays on the kernels:

    of gather_mul_sum(x, w, src, dst), cotangent g[N, F]:
        dx = gather_mul_sum(g, w, src=dst, dst=src)
        dw = gather_mul(x, g, src, dst)
    of gather_mul(a, b, src, dst), cotangent G[E, F]:
        da = gather_mul_sum(b, G, src=dst, dst=src)
        db = gather_mul_sum(a, G, src, dst)

The transposed grouping uses the other plan's CSR: the ``src`` side is
sorted once per plan, at the first backward, and never for inference.

The kernels serve device tensors of fp32, fp64, bf16 and f16 with
E < 2^31.  CPU tensors, ``HYDRAGNN_AMD_FORCE_EAGER=1`` and anything
outside that envelope run the doubles: ``index_select``, a product and
an ``index_add_`` in the accumulator type, one cast; no host sync.
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from ._extension import get_extension, use_eager
from .scatter import _rowptr_from_sorted

__all__ = ["SegmentPlan", "gather_mul_sum", "gather_mul", "path_counts",
           "reset_path_counts"]

_KERNEL_DTYPES = (torch.float32, torch.float64, torch.bfloat16,
                  torch.float16)

_counts = {"sum": 0, "mul": 0, "composition": 0}


def path_counts() -> dict:
    """Launches of the sum kernel and of the product kernel, and calls
    that ran a torch double instead."""
    return dict(_counts)


def reset_path_counts() -> None:
    for k in _counts:
        _counts[k] = 0


def fused_messages(default: bool) -> bool:
    """Whether a model stack takes the fused route: HYDRAGNN_GATHER_MUL=0
    restores the composition of generic ops, any other value selects the
    fused route, and unset leaves the stack's own default (on where the
    end-to-end step measured no slower, see profiles/README.md).  Read at
    call time."""
    value = os.environ.get("HYDRAGNN_GATHER_MUL")
    return default if value is None else value != "0"


def acc_dtype(dtype: torch.dtype) -> torch.dtype:
    """fp32 for the half types, the dtype itself otherwise."""
    return torch.float32 if dtype in (torch.bfloat16, torch.float16) \
        else dtype


class SegmentPlan:
    """One grouping of E edges into ``size`` rows: ``index[e]`` is the
    row of edge e.  ``csr()`` gives ``(perm | None, rowptr[size + 1])``
    with ``perm = argsort(index, stable=True)`` (None for a sorted
    index), built on first use and kept.  Nothing here syncs with the
    host."""

    def __init__(self, index: torch.Tensor, size: int,
                 sorted_index: bool = False, _identity: bool = False):
        if index.dim() != 1:
            raise ValueError("index must be [E]")
        if index.dtype != torch.long:
            index = index.long()
        self.index = index.contiguous()
        self.size = int(size)
        self.sorted_index = bool(sorted_index) or _identity
        self.is_identity = _identity
        self._csr: Optional[Tuple[Optional[torch.Tensor],
                                  torch.Tensor]] = None

    @classmethod
    def from_index(cls, index: torch.Tensor, size: int,
                   sorted_index: bool = False) -> "SegmentPlan":
        return cls(index, size, sorted_index)

    @classmethod
    def identity(cls, n_edges: int, device=None) -> "SegmentPlan":
        """index = arange(E): row e holds edge e alone."""
        plan = cls(torch.arange(n_edges, device=device), n_edges,
                   _identity=True)
        plan._csr = (None, torch.arange(n_edges + 1, device=device))
        return plan

    @property
    def n_edges(self) -> int:
        return self.index.shape[0]

    def csr(self):
        if self._csr is None:
            with torch.no_grad():
                if self.sorted_index:
                    perm, sidx = None, self.index
                else:
                    perm = torch.argsort(self.index, stable=True)
                    sidx = self.index.index_select(0, perm)
                self._csr = (perm, _rowptr_from_sorted(sidx, self.size))
        return self._csr


# ---------------------------------------------------------------------------
# pure-torch doubles
# ---------------------------------------------------------------------------
def torch_gather_mul_sum(x, w, src: SegmentPlan, dst: SegmentPlan):
    acc = acc_dtype(x.dtype)
    prod = x.index_select(0, src.index).to(acc) * w.to(acc)
    out = prod.new_zeros(dst.size, x.shape[1]).index_add_(0, dst.index, prod)
    return out.to(x.dtype)


def torch_gather_mul(a, b, src: SegmentPlan, dst: SegmentPlan):
    acc = acc_dtype(a.dtype)
    return (a.index_select(0, src.index).to(acc)
            * b.index_select(0, dst.index).to(acc)).to(a.dtype)


# ---------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------
def _kernel_route(t, n_edges) -> bool:
    return (t.is_cuda and not use_eager() and t.dtype in _KERNEL_DTYPES
            and n_edges < 2 ** 31)


def _gidx(plan: SegmentPlan):
    return None if plan.is_identity else plan.index


def _sum(x, w, src, dst):
    n_edges, feat = w.shape
    if n_edges == 0 or dst.size == 0 or feat == 0:
        return x.new_zeros(dst.size, feat)
    if _kernel_route(x, n_edges):
        perm, rowptr = dst.csr()
        _counts["sum"] += 1
        return get_extension(required=True).gather_mul_sum(
            x, w, _gidx(src), rowptr, perm)
    _counts["composition"] += 1
    return torch_gather_mul_sum(x, w, src, dst)


def _mul(a, b, src, dst):
    n_edges, feat = src.n_edges, a.shape[1]
    if n_edges == 0 or feat == 0:
        return a.new_empty(n_edges, feat)
    if _kernel_route(a, n_edges):
        _counts["mul"] += 1
        return get_extension(required=True).gather_mul(
            a, b, _gidx(src), _gidx(dst), n_edges)
    _counts["composition"] += 1
    return torch_gather_mul(a, b, src, dst)


class _GatherMulSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, src, dst):
        ctx.save_for_backward(x, w)
        ctx.plans = (src, dst)
        ctx.set_materialize_grads(False)
        return _sum(x, w, src, dst)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        x, w = ctx.saved_tensors
        src, dst = ctx.plans
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = gather_mul_sum(g, w, dst, src)
        if ctx.needs_input_grad[1]:
            dw = gather_mul(x, g, src, dst)
        return dx, dw, None, None


class _GatherMul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, src, dst):
        ctx.save_for_backward(a, b)
        ctx.plans = (src, dst)
        ctx.set_materialize_grads(False)
        return _mul(a, b, src, dst)

    @staticmethod
    def backward(ctx, G):
        if G is None:
            return None, None, None, None
        a, b = ctx.saved_tensors
        src, dst = ctx.plans
        da = db = None
        if ctx.needs_input_grad[0]:
            da = gather_mul_sum(b, G, dst, src)
        if ctx.needs_input_grad[1]:
            db = gather_mul_sum(a, G, src, dst)
        return da, db, None, None


def _flat(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dim() < 1:
        raise ValueError(f"{name} needs a row dim")
    feat = 1
    for k in t.shape[1:]:
        feat *= k
    return t.reshape(t.shape[0], feat).contiguous()


def _check_plans(src, dst):
    if not (isinstance(src, SegmentPlan) and isinstance(dst, SegmentPlan)):
        raise TypeError("src and dst must be SegmentPlans")
    if src.n_edges != dst.n_edges:
        raise ValueError(
            f"the plans group {src.n_edges} and {dst.n_edges} edges")


def gather_mul_sum(x: torch.Tensor, w: torch.Tensor, src: SegmentPlan,
                   dst: SegmentPlan) -> torch.Tensor:
    """out[dst.size, ...] = sum over the edges of each dst row of
    x[src.index[e]] * w[e].  See the module docstring."""
    _check_plans(src, dst)
    if x.dtype != w.dtype:
        raise ValueError(f"x is {x.dtype} and w is {w.dtype}")
    if x.shape[1:] != w.shape[1:]:
        raise ValueError(f"trailing shapes differ: {tuple(x.shape[1:])} "
                         f"and {tuple(w.shape[1:])}")
    if x.shape[0] != src.size:
        raise ValueError(f"x has {x.shape[0]} rows, src.size is {src.size}")
    if w.shape[0] != src.n_edges:
        raise ValueError(f"w has {w.shape[0]} rows for {src.n_edges} edges")
    out = _GatherMulSum.apply(_flat(x, "x"), _flat(w, "w"), src, dst)
    return out.view((dst.size,) + tuple(x.shape[1:]))


def gather_mul(a: torch.Tensor, b: torch.Tensor, src: SegmentPlan,
               dst: SegmentPlan) -> torch.Tensor:
    """out[E, ...] = a[src.index[e]] * b[dst.index[e]].  See the module
    docstring."""
    _check_plans(src, dst)
    if a.dtype != b.dtype:
        raise ValueError(f"a is {a.dtype} and b is {b.dtype}")
    if a.shape[1:] != b.shape[1:]:
        raise ValueError(f"trailing shapes differ: {tuple(a.shape[1:])} "
                         f"and {tuple(b.shape[1:])}")
    if a.shape[0] != src.size:
        raise ValueError(f"a has {a.shape[0]} rows, src.size is {src.size}")
    if b.shape[0] != dst.size:
        raise ValueError(f"b has {b.shape[0]} rows, dst.size is {dst.size}")
    out = _GatherMul.apply(_flat(a, "a"), _flat(b, "b"), src, dst)
    return out.view((src.n_edges,) + tuple(a.shape[1:]))


# `hydragnn_amd.ops.gather_mul` names this function once the package has
# exported it, so the counters are reachable through either spelling
gather_mul.path_counts = path_counts
gather_mul.reset_path_counts = reset_path_counts
