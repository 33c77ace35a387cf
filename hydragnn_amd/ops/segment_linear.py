"""Segment linear-attention primitives.

Rows are [N, H, .]; graphs are contiguous row ranges given by the rowptr
``ptr`` [G+1] (and, for the torch form, the per-row graph index
``batch``); g(i) is the graph of row i.

    segment_outer_sum   K[g,h,al,be] = sum_{i in g} A[i,h,al] B[i,h,be]
    segment_matvec      O[i,h,be] = sum_al A[i,h,al] K[g(i),h,al,be]
        trans=True      O[i,h,al] = sum_be A[i,h,be] K[g(i),h,al,be]

Linear (Performer) attention is ``segment_matvec(phi(q),
segment_outer_sum(phi(k), [v, 1]))`` over exactly each graph's rows.  The
two are bilinear and each one's gradients are the other one:

    outer sum         dA = matvec(B, dK, trans=True)   dB = matvec(A, dK)
    matvec            dA = matvec(dO, K, trans=True)   dK = outer(A, dO)
    matvec, trans     dA = matvec(dO, K)               dK = outer(dO, A)

so the autograd Functions below call the public functions in their
backwards and the pair is closed under differentiation to every order:
on the GPU no order leaves the HIP kernels (csrc/segment_linear.hip).

Dtype rule: segment matrices are always in the accumulator type -- fp32
for fp32, bf16 (and fp16) rows, fp64 for fp64 rows -- as output of the
first primitive and as input of the second, so a sum over a whole graph
is never rounded to bf16 and every gradient has a row operand in the row
dtype and a matrix operand in the accumulator type.  Row outputs are
rounded once to the row dtype.

``torch_segment_outer_sum`` / ``torch_segment_matvec`` are pure-torch
doubles of the two entry points: the CPU path, the path outside the
kernels' envelope, under HYDRAGNN_AMD_FORCE_EAGER and for other dtypes,
and the numerics reference of the tests.
"""

from __future__ import annotations

from typing import Optional

import torch

from ._extension import get_extension, use_eager

_KERNEL_DTYPES = (torch.float32, torch.bfloat16, torch.float64)
_LDS_BUDGET = 160 * 1024
MAX_A, MAX_B = 128, 132

# how often each entry point ran (tests read this to see which one served)
segment_linear_stats = {"outer": 0, "matvec": 0, "torch_outer": 0,
                        "torch_matvec": 0}


def acc_dtype(dtype: torch.dtype) -> torch.dtype:
    """The accumulator type of a row dtype: the dtype of every segment
    matrix."""
    return torch.float64 if dtype == torch.float64 else torch.float32


def segment_linear_ok(a: int, b: int, tensor: torch.Tensor) -> bool:
    """True when rows like ``tensor`` with widths (a, b) run on the HIP
    kernels, all three passes (a gradient needs the other two)."""
    if not tensor.is_cuda or use_eager():
        return False
    if tensor.dtype not in _KERNEL_DTYPES:
        return False
    if not (1 <= a <= MAX_A and 1 <= b <= MAX_B):
        return False
    ext = get_extension(required=True)
    return all(ext.segment_linear_lds_bytes(a, b, tensor.dtype, p)
               <= _LDS_BUDGET for p in (0, 1, 2))


def segment_linear_tiling(a: int, b: int, dtype: torch.dtype):
    """(row-tile length R of the outer sum, rows one matvec workgroup
    handles per pass) of the kernels that serve (a, b, dtype)."""
    r, bw = get_extension(required=True).segment_linear_tiling(a, b, dtype)
    return r, bw


def torch_segment_outer_sum(A, B, ptr, batch):
    """Pure-torch double of the ``segment_outer_sum`` entry point."""
    acc = acc_dtype(A.dtype)
    G = ptr.numel() - 1
    with torch.autocast(A.device.type, enabled=False):
        prod = A.to(acc).unsqueeze(-1) * B.to(acc).unsqueeze(-2)
        K = prod.new_zeros((G,) + tuple(prod.shape[1:]))
        return K.index_add(0, batch, prod)


def torch_segment_matvec(A, K, ptr, batch, trans=False):
    """Pure-torch double of the ``segment_matvec`` entry point."""
    eq = "nhb,nhab->nha" if trans else "nha,nhab->nhb"
    with torch.autocast(A.device.type, enabled=False):
        return torch.einsum(eq, A.to(K.dtype), K[batch]).to(A.dtype)


def _outer_entry(A, B, ptr, batch, z):
    if segment_linear_ok(A.shape[2], B.shape[2], A):
        segment_linear_stats["outer"] += 1
        return get_extension(required=True).segment_outer_sum(
            A.contiguous(), B.contiguous(), ptr, int(z or 0))
    segment_linear_stats["torch_outer"] += 1
    return torch_segment_outer_sum(A, B, ptr, batch)


def _matvec_entry(A, K, ptr, batch, trans):
    if segment_linear_ok(K.shape[2], K.shape[3], A):
        segment_linear_stats["matvec"] += 1
        return get_extension(required=True).segment_matvec(
            A.contiguous(), K.contiguous(), ptr, bool(trans))
    segment_linear_stats["torch_matvec"] += 1
    return torch_segment_matvec(A, K, ptr, batch, trans)


class _SegmentOuterSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, ptr, batch, z):
        ctx.save_for_backward(A, B, ptr, batch)
        return _outer_entry(A, B, ptr, batch, z)

    @staticmethod
    def backward(ctx, dK):
        A, B, ptr, batch = ctx.saved_tensors
        dA = dB = None
        if ctx.needs_input_grad[0]:
            dA = segment_matvec(B, dK, ptr, batch, trans=True)
        if ctx.needs_input_grad[1]:
            dB = segment_matvec(A, dK, ptr, batch)
        return dA, dB, None, None, None


class _SegmentMatvec(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, K, ptr, batch, trans):
        ctx.save_for_backward(A, K, ptr, batch)
        ctx.trans = trans
        return _matvec_entry(A, K, ptr, batch, trans)

    @staticmethod
    def backward(ctx, dO):
        A, K, ptr, batch = ctx.saved_tensors
        dA = dK = None
        if ctx.needs_input_grad[0]:
            dA = segment_matvec(dO, K, ptr, batch, trans=not ctx.trans)
        if ctx.needs_input_grad[1]:
            dK = (segment_outer_sum(dO, A, ptr, batch) if ctx.trans
                  else segment_outer_sum(A, dO, ptr, batch))
        return dA, dK, None, None, None


def segment_outer_sum(A: torch.Tensor, B: torch.Tensor, ptr: torch.Tensor,
                      batch: torch.Tensor, z: Optional[int] = None):
    """A [N, H, a], B [N, H, b], graph rowptr [G+1] and per-row graph
    index [N] -> K [G, H, a, b] in the accumulator type of the rows'
    (promoted) dtype.  ``z`` pins the kernel's row split (tests)."""
    rows = torch.promote_types(A.dtype, B.dtype)
    return _SegmentOuterSum.apply(A.to(rows), B.to(rows), ptr, batch, z)


def segment_matvec(A: torch.Tensor, K: torch.Tensor, ptr: torch.Tensor,
                   batch: torch.Tensor, trans: bool = False):
    """A [N, H, a] (trans: [N, H, b]) and K [G, H, a, b] -> [N, H, b]
    (trans: [N, H, a]) in A's dtype; K is taken in the accumulator type
    of A's dtype."""
    return _SegmentMatvec.apply(A, K.to(acc_dtype(A.dtype)), ptr, batch,
                                bool(trans))
