"""Autograd closure of segment-varlen attention, without a GPU.

The pure-torch doubles of the two kernel entry points
(``torch_varlen_attention_fwd`` / ``torch_varlen_attention_bwd``) and
the autograd Function pair driven by them on CPU tensors, against the
dense-batch torch reference in fp64.  The segment sizes include a
single-row and an empty graph."""

import math

import pytest
import torch

from hydragnn_amd.ops.varlen_attn import (
    torch_varlen_attention, torch_varlen_attention_bwd,
    torch_varlen_attention_fwd, varlen_attention_fn)

SIZES = [1, 0, 7, 33]
H = 3


def _inputs(dh):
    torch.manual_seed(dh)
    sizes = torch.tensor(SIZES)
    ptr = torch.zeros(len(SIZES) + 1, dtype=torch.long)
    ptr[1:] = sizes.cumsum(0)
    batch = torch.repeat_interleave(torch.arange(len(SIZES)), sizes)
    N = int(sizes.sum())
    q, k, v, w = (torch.randn(N, H, dh, dtype=torch.float64)
                  for _ in range(4))
    return q, k, v, w, ptr, batch


@pytest.mark.parametrize("dh", [5, 16])
def test_torch_fwd_double_matches_reference(dh):
    q, k, v, _, ptr, batch = _inputs(dh)
    out, lse = torch_varlen_attention_fwd(q, k, v, ptr)
    ref = torch_varlen_attention(q, k, v, batch)
    assert (out - ref).abs().max() < 1e-12
    assert lse.shape == (q.shape[0], H)
    p = ptr.tolist()
    for lo, hi in zip(p[:-1], p[1:]):
        if hi == lo:
            continue
        s = torch.einsum("ihd,jhd->hij", q[lo:hi], k[lo:hi]) \
            / math.sqrt(dh)
        want = torch.logsumexp(s, dim=-1).transpose(0, 1)
        assert (lse[lo:hi] - want).abs().max() < 1e-12


@pytest.mark.parametrize("dh", [5, 16])
def test_torch_bwd_double_matches_autograd(dh):
    q, k, v, w, ptr, batch = _inputs(dh)
    out, lse = torch_varlen_attention_fwd(q, k, v, ptr)
    got = torch_varlen_attention_bwd(q, k, v, out, lse, w, ptr)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    want = torch.autograd.grad(
        torch_varlen_attention(qr, kr, vr, batch), (qr, kr, vr), w)
    for a, b in zip(got, want):
        assert (a - b).abs().max() < 1e-10


@pytest.mark.parametrize("dh", [5, 16])
def test_function_pair_first_and_second_order(dh):
    """varlen_attention_fn on CPU tensors: first order, and the
    double-backward closure (every gradient differentiated again
    w.r.t. every operand), against the reference."""
    q, k, v, w, ptr, batch = _inputs(dh)

    def grads(fn):
        x = [t.clone().requires_grad_(True) for t in (q, k, v)]
        first = torch.autograd.grad((fn(*x) * w).sum(), x,
                                    create_graph=True)
        second = [[torch.autograd.grad(g.square().sum(), t,
                                       retain_graph=True)[0]
                   for t in x] for g in first]
        return first, second

    f1, s1 = grads(lambda a, b, c: varlen_attention_fn(a, b, c, ptr,
                                                       batch))
    f2, s2 = grads(lambda a, b, c: torch_varlen_attention(a, b, c,
                                                          batch))
    for a, b in zip(f1, f2):
        assert (a - b).abs().max() < 1e-10
    for ra, rb in zip(s1, s2):
        for a, b in zip(ra, rb):
            assert (a - b).abs().max() < 1e-8


def test_function_pair_cotangent_depending_on_output():
    """A loss whose cotangent is itself a function of the output
    (out.square().sum(), g = 2 out): the second order must count the
    path through g exactly once."""
    q, k, v, _, ptr, batch = _inputs(16)

    def second(fn):
        x = q.clone().requires_grad_(True)
        g = torch.autograd.grad(fn(x).square().sum(), x,
                                create_graph=True)[0]
        return torch.autograd.grad(g.square().sum(), x)[0]

    a = second(lambda x: varlen_attention_fn(x, k, v, ptr, batch))
    b = second(lambda x: torch_varlen_attention(x, k, v, batch))
    assert (a - b).abs().max() < 1e-8


def test_recompute_backward_switch(monkeypatch):
    """HYDRAGNN_VARLEN_ATTN_BWD=0 is read at call time and gives the
    same first-order gradients through the recompute route."""
    q, k, v, w, ptr, batch = _inputs(5)

    def first():
        x = [t.clone().requires_grad_(True) for t in (q, k, v)]
        return torch.autograd.grad(
            (varlen_attention_fn(*x, ptr, batch) * w).sum(), x)

    on = first()
    monkeypatch.setenv("HYDRAGNN_VARLEN_ATTN_BWD", "0")
    off = first()
    for a, b in zip(on, off):
        assert (a - b).abs().max() < 1e-10
