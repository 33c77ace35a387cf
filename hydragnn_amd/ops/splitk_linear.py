"""Linear layer with a split-K weight gradient.

Per-edge MLPs (e.g. the MACE radial network) have tiny in/out widths
but E ~ 10^5-10^6 rows: the weight-gradient GEMM dW = X^T g has
M, N <= a few hundred and K = E, which hipBLASLt schedules on only
(M/16)x(N/16) workgroups — a serial-K crawl on a 256-CU chip.  Here the
K dimension is split into S chunks computed as a bmm (S x tiles
workgroups) and summed — an order of magnitude faster at these shapes.

backward() is built from differentiable torch ops, so the force
training double-backward works unchanged.
"""

from __future__ import annotations

import torch
from torch import nn

from ._extension import get_extension, use_eager
from .segment_plan import KERNEL_DTYPES, PathCounter, env_default

# HYDRAGNN_WGRAD_KERNEL, tri-state: unset leaves the caller's default
# (off for SplitKLinear and MFMALinear, models/dimenet.py states its own),
# "0" is off, anything else on.
WGRAD_FLAG = "HYDRAGNN_WGRAD_KERNEL"
# csrc/wgrad.hip: widths up to 256, and rows from where it beats the
# library GEMM at 64 x 64 fp64 (32.5 us against 36.6 us at 512 rows, the
# GEMM ahead at 256: profiles/README.md)
MAX_WIDTH = 256
MIN_ROWS = 512

wgrad_paths = PathCounter("kernel", "composition")


def wgrad_kernel_enabled(default: bool = False) -> bool:
    return env_default(WGRAD_FLAG, default)


def wgrad_route(x2d: torch.Tensor, n_out: int) -> bool:
    """Whether dW = g^T x for x2d [E, K] and g [E, n_out] of x2d's dtype
    is inside the envelope of the weight-gradient kernel."""
    E, K = x2d.shape
    return (x2d.is_cuda and not use_eager()
            and x2d.dtype in KERNEL_DTYPES
            and 1 <= K <= MAX_WIDTH and 1 <= n_out <= MAX_WIDTH
            and MIN_ROWS <= E < 2 ** 31)


class _WgradFn(torch.autograd.Function):
    """(gW, gb) = (g^T x, g.sum(0)) on the HIP kernel, in the accumulator
    dtype; gb is empty without want_bias.  For cotangents C [N, K] and
    c [N]: dx = g C and dg = x C^T + c, plain differentiable matmuls."""

    @staticmethod
    def forward(ctx, x, g, want_bias):
        ctx.save_for_backward(x, g)
        ctx.want_bias = want_bias
        gW, gb = get_extension(required=True).linear_wgrad(g, x, want_bias)
        wgrad_paths.hit("kernel")
        return gW, gb

    @staticmethod
    def backward(ctx, C, c):
        x, g = ctx.saved_tensors
        dx = dg = None
        if ctx.needs_input_grad[0]:
            dx = (g.to(C.dtype) @ C).to(x.dtype)
        if ctx.needs_input_grad[1]:
            dg = x.to(C.dtype) @ C.t()
            if ctx.want_bias:
                dg = dg + c
            dg = dg.to(g.dtype)
        return dx, dg, None


def _splitk_weight_grad(x2d: torch.Tensor, g2d: torch.Tensor,
                        chunks: int) -> torch.Tensor:
    E = x2d.shape[0]
    S = min(chunks, max(1, E // 256))
    if S <= 1 or not x2d.is_cuda:
        # split-K only pays on the GPU (hipBLASLt's serial-K underfill);
        # on CPU the chunked bmm is strictly slower than one mm
        return g2d.t() @ x2d
    pad = (S - E % S) % S
    if pad:
        x2d = torch.nn.functional.pad(x2d, (0, 0, 0, pad))
        g2d = torch.nn.functional.pad(g2d, (0, 0, 0, pad))
    xs = x2d.view(S, -1, x2d.shape[1])
    gs = g2d.view(S, -1, g2d.shape[1])
    return torch.bmm(gs.transpose(1, 2), xs).sum(0)


def _weight_grad(x2d: torch.Tensor, g2d: torch.Tensor,
                 chunks: int) -> torch.Tensor:
    """g2d^T x2d in g2d's dtype: the kernel where HYDRAGNN_WGRAD_KERNEL
    is on and the route applies, the bmm composition otherwise."""
    if (wgrad_kernel_enabled() and x2d.dtype == g2d.dtype
            and wgrad_route(x2d, g2d.shape[1])):
        return _WgradFn.apply(x2d, g2d, False)[0].to(g2d.dtype)
    if g2d.is_cuda:
        wgrad_paths.hit("composition")
    return _splitk_weight_grad(x2d, g2d, chunks)


class _SplitKLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, wgrad_default=False):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.wgrad_default = wgrad_default
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g2d = g.reshape(-1, g.shape[-1])
        x2d = x.reshape(-1, x.shape[-1]).to(g2d.dtype)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            if g2d.is_cuda:
                # gx = g2d @ W == linear(g2d, W^T): route through the
                # split-K Function so the SECOND-order pass (force
                # double backward differentiating this product by W)
                # also gets a split-K weight grad — a plain mm here
                # regenerates the serial-K [out, E] @ [E, in] GEMM
                gx = _SplitKLinearFn.apply(
                    g2d, weight.t().to(g2d.dtype), None, ctx.wgrad_default
                ).view_as(x).to(x.dtype)
            else:
                gx = (g2d @ weight.to(g2d.dtype)).view_as(x).to(x.dtype)
        want_gb = ctx.has_bias and ctx.needs_input_grad[2]
        if (ctx.needs_input_grad[1]
                and wgrad_kernel_enabled(ctx.wgrad_default)
                and wgrad_route(x2d, g2d.shape[1])):
            # gb comes out of the same pass over g
            gw, kb = _WgradFn.apply(x2d, g2d, want_gb)
            gw = gw.to(weight.dtype)
            if want_gb:
                gb = kb.to(g2d.dtype)
            return gx, gw, gb, None
        if ctx.needs_input_grad[1]:
            if g2d.is_cuda:
                wgrad_paths.hit("composition")
            gw = _splitk_weight_grad(x2d, g2d, 64).to(weight.dtype)
        if want_gb:
            gb = g2d.sum(0)
        return gx, gw, gb, None


class SplitKLinear(nn.Linear):
    def forward(self, x):
        if not x.is_cuda:
            # plain autograd linear on CPU (no custom Function
            # overhead; split-K is a GPU-shape fix)
            return torch.nn.functional.linear(x, self.weight,
                                              self.bias)
        return _SplitKLinearFn.apply(x, self.weight, self.bias)
