"""Segment linear-attention primitives on the CPU: the torch doubles
against a naive per-segment loop, closure of the autograd Function pair
under differentiation, and PerformerAttention.forward_segments against
the dense-batch forward."""

import pytest
import torch

from hydragnn_amd.data import to_dense_batch
from hydragnn_amd.globalatt.gps import PerformerAttention
from hydragnn_amd.ops import segment_matvec, segment_outer_sum
from hydragnn_amd.ops.segment_linear import (
    torch_segment_matvec, torch_segment_outer_sum)

H = 2
WIDTHS = [(1, 1), (3, 5), (8, 9)]
SIZES = [3, 0, 1, 7]


def _segments(sizes):
    sizes = torch.tensor(sizes, dtype=torch.long)
    ptr = torch.zeros(len(sizes) + 1, dtype=torch.long)
    ptr[1:] = sizes.cumsum(0)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), sizes)
    return ptr, batch


def _rows(n, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, H, w, dtype=torch.float64, generator=g)


def _naive_outer(A, B, ptr):
    G = ptr.numel() - 1
    K = torch.zeros(G, A.shape[1], A.shape[2], B.shape[2], dtype=A.dtype)
    for g in range(G):
        for i in range(int(ptr[g]), int(ptr[g + 1])):
            for h in range(A.shape[1]):
                K[g, h] += torch.outer(A[i, h], B[i, h])
    return K


def _naive_matvec(A, K, ptr, trans):
    G = ptr.numel() - 1
    wout = K.shape[2] if trans else K.shape[3]
    O = torch.zeros(A.shape[0], A.shape[1], wout, dtype=A.dtype)
    for g in range(G):
        for i in range(int(ptr[g]), int(ptr[g + 1])):
            for h in range(A.shape[1]):
                O[i, h] = (K[g, h] @ A[i, h] if trans
                           else A[i, h] @ K[g, h])
    return O


@pytest.mark.parametrize("a,b", WIDTHS)
def test_torch_doubles_match_naive_loop(a, b):
    ptr, batch = _segments(SIZES)
    n = int(ptr[-1])
    A, B = _rows(n, a, 1), _rows(n, b, 2)
    K = torch_segment_outer_sum(A, B, ptr, batch)
    K_ref = _naive_outer(A, B, ptr)
    assert K.dtype == torch.float64 and K.shape == (len(SIZES), H, a, b)
    # a handful of addends of magnitude ~1: a few ulp of fp64
    torch.testing.assert_close(K, K_ref, rtol=0, atol=1e-13)
    assert torch.count_nonzero(K[1]) == 0          # the empty segment
    for trans in (False, True):
        X = B if trans else A
        O = torch_segment_matvec(X, K_ref, ptr, batch, trans)
        torch.testing.assert_close(
            O, _naive_matvec(X, K_ref, ptr, trans), rtol=0, atol=1e-12)
    # the public functions on the CPU are the same doubles
    assert torch.equal(segment_outer_sum(A, B, ptr, batch), K)
    assert torch.equal(segment_matvec(A, K_ref, ptr, batch),
                       torch_segment_matvec(A, K_ref, ptr, batch))


@pytest.mark.parametrize("sizes", [[], [0, 0, 0]])
def test_no_rows_and_no_graphs(sizes):
    ptr, batch = _segments(sizes)
    G = len(sizes)
    A, B = _rows(0, 3, 1), _rows(0, 5, 2)
    K = segment_outer_sum(A, B, ptr, batch)
    assert K.shape == (G, H, 3, 5) and torch.count_nonzero(K) == 0
    assert segment_matvec(A, K, ptr, batch).shape == (0, H, 5)
    assert segment_matvec(B, K, ptr, batch, trans=True).shape == (0, H, 3)


def test_matrix_dtype_is_the_accumulator_type():
    ptr, batch = _segments(SIZES)
    n = int(ptr[-1])
    for rows, acc in ((torch.float32, torch.float32),
                      (torch.bfloat16, torch.float32),
                      (torch.float64, torch.float64)):
        A, B = _rows(n, 3, 1).to(rows), _rows(n, 5, 2).to(rows)
        K = segment_outer_sum(A, B, ptr, batch)
        assert K.dtype == acc
        assert segment_matvec(A, K, ptr, batch).dtype == rows
        assert segment_matvec(B, K, ptr, batch, trans=True).dtype == rows


@pytest.mark.parametrize("a,b", WIDTHS)
def test_outer_sum_gradcheck(a, b):
    ptr, batch = _segments(SIZES)
    n = int(ptr[-1])
    A = _rows(n, a, 3).requires_grad_(True)
    B = _rows(n, b, 4).requires_grad_(True)
    fn = lambda A, B: segment_outer_sum(A, B, ptr, batch)  # noqa: E731
    assert torch.autograd.gradcheck(fn, (A, B))
    assert torch.autograd.gradgradcheck(fn, (A, B))


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("a,b", WIDTHS)
def test_matvec_gradcheck(a, b, trans):
    ptr, batch = _segments(SIZES)
    n = int(ptr[-1])
    X = _rows(n, b if trans else a, 5).requires_grad_(True)
    g = torch.Generator().manual_seed(6)
    K = torch.randn(len(SIZES), H, a, b, dtype=torch.float64,
                    generator=g).requires_grad_(True)
    fn = lambda X, K: segment_matvec(X, K, ptr, batch, trans)  # noqa: E731
    assert torch.autograd.gradcheck(fn, (X, K))
    assert torch.autograd.gradgradcheck(fn, (X, K))


def test_backward_masks_unneeded_gradients():
    ptr, batch = _segments(SIZES)
    n = int(ptr[-1])
    A = _rows(n, 3, 7).requires_grad_(True)
    B = _rows(n, 5, 8)
    K = segment_outer_sum(A, B, ptr, batch)
    O = segment_matvec(B, K, ptr, batch, trans=True)
    (gA,) = torch.autograd.grad(O.sum(), (A,))
    assert gA.shape == A.shape and B.grad is None


def test_forward_segments_matches_dense_forward():
    """Same fp64 module and input through the dense-batch forward and
    through forward_segments; output and input gradient.

    The two forms are the same arithmetic and differ only in the order
    of their sums.  Written as one sum, an output element is

        out[i,c] = sum_{h,d,m,j} W[c,hd] qp[i,h,m] kp[j,h,m] v[j,h,d]
                   / den[i,h]

    with n = C * m * n_g addends for the largest graph, so the bound is
    n * 2^-52 * sum|addend| (den is a sum of positive terms; 2^-52 is
    twice the unit roundoff and covers the normaliser's own error).  The
    gradient goes back through the same chain, each bilinear step's
    gradient being the other primitive with the same addend counts, and
    ends in the qkv projection's backward dx = g_qkv @ W_qkv: its bound
    is the same n * 2^-52 times that last reduction's sum|addend|.
    Observed on the CPU: 2e-16 (output) and 1e-15 (gradient).
    """
    torch.manual_seed(11)
    C, heads = 32, 4
    sizes = [5, 1, 9, 3]
    mod = PerformerAttention(C, heads).double()
    ptr, batch = _segments(sizes)
    n = int(ptr[-1])
    x0 = torch.randn(n, C, dtype=torch.float64)
    w = torch.randn(n, C, dtype=torch.float64)

    kept = {}

    def keep_qkv(module, inputs, output):
        output.retain_grad()
        kept["qkv"] = output

    hook = mod.qkv.register_forward_hook(keep_qkv)
    xd = x0.clone().requires_grad_(True)
    dense, mask = to_dense_batch(xd, batch)
    out_d = mod(dense, mask=mask)[mask]
    (out_d * w).sum().backward()
    g_qkv = kept["qkv"].grad[mask]
    hook.remove()

    xs = x0.clone().requires_grad_(True)
    out_s = mod.forward_segments(xs, ptr, batch)
    (out_s * w).sum().backward()

    with torch.no_grad():
        d = C // heads
        q, k, v = mod.qkv(x0).view(n, 3, heads, d).unbind(1)
        qp, kp = mod._phi(q), mod._phi(k)
        kv_abs = torch.zeros(len(sizes), heads, qp.shape[-1], d,
                             dtype=torch.float64).index_add_(
            0, batch, kp.unsqueeze(-1) * v.abs().unsqueeze(-2))
        ksum = torch.zeros(len(sizes), heads, qp.shape[-1],
                           dtype=torch.float64).index_add_(0, batch, kp)
        den = torch.einsum("nhm,nhm->nh", qp, ksum[batch]) + 1e-6
        num_abs = torch.einsum("nhm,nhmd->nhd", qp, kv_abs[batch])
        s_out = ((num_abs / den[..., None]).reshape(n, C)
                 @ mod.out.weight.abs().t()).max()
        s_grad = (g_qkv.abs() @ mod.qkv.weight.abs()).max()
        n_add = C * mod.num_features * max(sizes)
        err_out = (out_s - out_d).abs().max()
        err_grad = (xs.grad - xd.grad).abs().max()
    print(f"out err {err_out:.3e} bound {n_add * 2.0 ** -52 * s_out:.3e}; "
          f"grad err {err_grad:.3e} "
          f"bound {n_add * 2.0 ** -52 * s_grad:.3e}")
    assert err_out <= n_add * 2.0 ** -52 * s_out
    assert err_grad <= n_add * 2.0 ** -52 * s_grad
