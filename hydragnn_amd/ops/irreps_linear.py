"""MFMA-backed per-l channel mixing for irreps towers.

`IrrepsLinear` (models/mace/o3.py) is the o3.Linear equivalent on the
dense [N, C, D] layout and the biggest GEMM family after the tensor
products.  The torch route (bmm over D slices) pays 3x HBM traffic
(permute copy, D skinny hipBLASLt GEMMs at 1.4-3% MFMA issue density,
permute-back copy — see profiles/README.md PMC audit).  The HIP kernel
(csrc/irreps_linear.hip) does the whole map in one pass: x tile and the
full weight stack LDS-resident, all D GEMMs on
v_mfma_f32_16x16x32_bf16, registers holding every m until the single
output write.

Gradient closure: gX is the same kernel with the weight read
transposed (trans_w flipped); gW is a second HIP kernel
(irreps_linear_gw_kernel) contracting over n with MFMA from the same
LDS staging — copy-free and deterministic (per-block fp32 partials,
summed on the stream).  An earlier bmm/einsum gW was measured SLOWER
than the torch path end-to-end (permuted copies of x and g); the
kernel version flips the A/B to +1.3% (32.7k vs 32.3k g/s, default
bench).  First and second order both stay on the kernels, so force
training works.

Eligibility is decided on the forward shape only, so every backward
route checks the host envelope of the kernel it would enter for the
shape that kernel will see (gX swaps the channels, gW has its own LDS
footprint) and otherwise runs the differentiable torch composition.
"""

from __future__ import annotations

import torch

from ._extension import get_extension, use_eager

# host envelopes of the two entry points (csrc/irreps_linear.hip): the
# dynamic LDS plus the kernels' static 64 B lmap table must fit 160 KiB
_MAX_LDS = 160 * 1024 - 64
_BM = 32


def irreps_fwd_kernel_ok(c_in: int, c_out: int, d: int,
                         n_l: int) -> bool:
    """Host envelope of `irreps_linear` (either trans_w) for a
    [*, c_in, d] input mixed to c_out channels."""
    if c_in % 32 != 0 or c_out % 64 != 0 or d > 16:
        return False
    lds = (d * _BM * (c_in + 8) + n_l * c_in * (c_out + 8)) * 2
    return lds <= _MAX_LDS


def irreps_gw_kernel_ok(c_in: int, c_out: int, d: int,
                        n_l: int) -> bool:
    """Host envelope of `irreps_linear_gw` for x [*, c_in, d] and
    g [*, c_out, d]."""
    tiles = (c_in // 16) * (c_out // 16)
    if (c_in % 16 != 0 or c_out % 16 != 0 or tiles % 4 != 0
            or tiles > 16 or n_l > 4 or d > 16):
        return False
    lds = (d * _BM * (c_in + 8) + d * _BM * (c_out + 8)) * 2
    return lds <= _MAX_LDS


def irreps_kernel_ok(n: int, c_in: int, c_out: int, d: int,
                     n_l: int) -> bool:
    return irreps_fwd_kernel_ok(c_in, c_out, d, n_l) and n >= 64


def _mix(x, W, lmap, trans_w):
    """The forward map (no bias/residual) as differentiable torch ops:
    one batched GEMM over the D slices."""
    Wk = W.transpose(1, 2) if trans_w else W
    return torch.bmm(x.permute(2, 0, 1),
                     Wk[lmap]).permute(1, 2, 0).contiguous()


def _mix_routed(x, W, lmap, trans_w):
    """`_mix` on the kernel when the shape THIS call sees is inside the
    host envelope, else the torch composition."""
    c_out = W.shape[1] if trans_w else W.shape[2]
    if irreps_fwd_kernel_ok(x.shape[1], c_out, x.shape[2], W.shape[0]):
        return _IrrepsLinearFn.apply(x, W, lmap, None, trans_w)
    return _mix(x, W, lmap, trans_w)


class _IrrepsLinearFn(torch.autograd.Function):
    """out[n,o,m] = sum_i x[n,i,m] * Wk[lmap[m]][i,o], with
    Wk[i,o] = W[l,i,o] (trans_w=False) or W[l,o,i] (trans_w=True)."""

    @staticmethod
    def forward(ctx, x, W, lmap, bias, trans_w, add=None):
        ext = get_extension(required=True)
        out = ext.irreps_linear(x.contiguous(), W.contiguous(), lmap,
                                bias, trans_w, add)
        ctx.save_for_backward(x, W, lmap, bias)
        ctx.trans_w = trans_w
        return out

    @staticmethod
    def backward(ctx, g):
        x, W, lmap, bias = ctx.saved_tensors
        trans_w = ctx.trans_w
        g = g.contiguous()
        gx = gw = gb = None
        ga = g if (len(ctx.needs_input_grad) > 5
                   and ctx.needs_input_grad[5]) else None
        if ctx.needs_input_grad[0]:
            # same kernel, channels swapped: its envelope is checked
            # for the swapped shape
            gx = _mix_routed(g, W, lmap, not trans_w)
        if ctx.needs_input_grad[1]:
            gw = _weight_grad(x, g, lmap, W.shape[0])
            if trans_w:
                gw = gw.transpose(1, 2)
            gw = gw.to(W.dtype)
        if bias is not None and ctx.needs_input_grad[3]:
            gb = g[:, :, 0].sum(0).to(bias.dtype)
        return gx, gw, None, gb, None, ga


class _IrrepsGWFn(torch.autograd.Function):
    """gW[l,i,o] = sum_{n, m in l} x[n,i,m] * g[n,o,m] in fp32 on the
    copy-free MFMA contraction over n: per-block fp32 partials
    (deterministic), summed here.  Bilinear in (x, g), so both
    gradients are the forward map again with the cotangent as weight."""

    @staticmethod
    def forward(ctx, x, g, lmap, n_l):
        ext = get_extension(required=True)
        nblocks = min(512, (x.shape[0] + _BM - 1) // _BM)
        parts = ext.irreps_linear_gw(x.contiguous(), g.contiguous(),
                                     lmap, n_l, nblocks)
        ctx.save_for_backward(x, g, lmap)
        return parts.sum(0)

    @staticmethod
    def backward(ctx, h):
        x, g, lmap = ctx.saved_tensors
        h = h.to(x.dtype).contiguous()
        gx = gg = None
        if ctx.needs_input_grad[0]:
            gx = _mix_routed(g, h, lmap, True)
        if ctx.needs_input_grad[1]:
            gg = _mix_routed(x, h, lmap, False)
        return gx, gg, None, None


def _weight_grad(x, g, lmap, n_l):
    """[n_l, c_in, c_out] weight gradient: the gW kernel (fp32) inside
    its host envelope, else a per-m batched GEMM folded m -> l."""
    c_in, c_out = x.shape[1], g.shape[1]
    if irreps_gw_kernel_ok(c_in, c_out, x.shape[2], n_l):
        return _IrrepsGWFn.apply(x, g, lmap, n_l)
    gw_m = torch.bmm(x.permute(2, 1, 0), g.permute(2, 0, 1))
    gw = gw_m.new_zeros(n_l, c_in, c_out)
    gw.index_add_(0, lmap, gw_m)
    return gw


def irreps_linear(x: torch.Tensor, W: torch.Tensor, lmap: torch.Tensor,
                  bias=None, add=None) -> torch.Tensor:
    """[N, Cin, D] x, [L, Cin, Cout] W -> [N, Cout, D] on the MFMA
    kernel (bf16); `add` is an optional residual fused into the
    epilogue (its gradient is the identity)."""
    return _IrrepsLinearFn.apply(x, W, lmap, bias, False, add)


def irreps_linear_eligible(x: torch.Tensor, W: torch.Tensor) -> bool:
    import os
    if use_eager() or not x.is_cuda:
        return False
    if os.environ.get("HYDRAGNN_IRREPS_MFMA", "1") == "0":
        return False
    from .mfma_linear import _bf16_ok
    if not _bf16_ok(x):
        return False
    return irreps_kernel_ok(x.shape[0], x.shape[1], W.shape[2],
                            x.shape[2], W.shape[0])
