"""Second order of segment-varlen attention, without a GPU.

``torch_varlen_attention_bwd2`` (the pure-torch double of the
``varlen_attention_bwd2`` entry point) against autograd of the two
first-order doubles in fp64, and the route the autograd Function pair
takes for its double backward on CPU tensors: the closed form when no
third order is requested, the torch recompute otherwise or under
``HYDRAGNN_VARLEN_ATTN_BWD2=0``.  The segment sizes include a
single-row and an empty graph."""

import pytest
import torch

import hydragnn_amd.ops.varlen_attn as va
from hydragnn_amd.ops.varlen_attn import (
    torch_varlen_attention, torch_varlen_attention_bwd,
    torch_varlen_attention_bwd2, torch_varlen_attention_fwd,
    varlen_attention_fn)

SIZES = [1, 0, 7, 33]
H = 3


def _inputs(dh, n=4):
    torch.manual_seed(dh)
    sizes = torch.tensor(SIZES)
    ptr = torch.zeros(len(SIZES) + 1, dtype=torch.long)
    ptr[1:] = sizes.cumsum(0)
    batch = torch.repeat_interleave(torch.arange(len(SIZES)), sizes)
    N = int(sizes.sum())
    ts = [torch.randn(N, H, dh, dtype=torch.float64) for _ in range(n)]
    return ts, ptr, batch


@pytest.mark.parametrize("absent", [None, 0, 1, 2])
@pytest.mark.parametrize("dh", [5, 16])
def test_torch_bwd2_double_matches_autograd(dh, absent):
    """The closed form against torch.autograd.grad of bwd(fwd(.)), with
    all three cotangents and with each of cq/ck/cv absent in turn."""
    (q, k, v, g, cq, ck, cv), ptr, _ = _inputs(dh, 7)
    cots = [cq, ck, cv]
    if absent is not None:
        cots[absent] = None
    out, lse = torch_varlen_attention_fwd(q, k, v, ptr)
    got = torch_varlen_attention_bwd2(q, k, v, out, lse, g, *cots, ptr)

    x = [t.clone().requires_grad_(True) for t in (q, k, v, g)]
    o, ls = torch_varlen_attention_fwd(*x[:3], ptr)
    first = torch_varlen_attention_bwd(*x[:3], o, ls, x[3], ptr)
    r = sum((c * d).sum() for c, d in zip(cots, first) if c is not None)
    want = torch.autograd.grad(r, x)
    for a, b in zip(got, want):
        assert (a - b).abs().max() < 1e-10


def _force_style(fn, q, k, v, w, create_graph=False):
    """First-order gradients with create_graph, then the gradient of
    their squared norm with respect to every operand."""
    x = [t.clone().requires_grad_(True) for t in (q, k, v)]
    first = torch.autograd.grad((fn(*x) * w).sum(), x, create_graph=True)
    loss = sum(g.square().sum() for g in first)
    second = torch.autograd.grad(loss, x, create_graph=create_graph)
    return x, second


def _count_recompute(monkeypatch):
    calls = []
    real = va._recompute_out

    def spy(*a):
        calls.append(1)
        return real(*a)

    monkeypatch.setattr(va, "_recompute_out", spy)
    return calls


@pytest.mark.parametrize("dh", [5, 16])
def test_double_backward_skips_recompute_and_matches_reference(
        dh, monkeypatch):
    """The ordinary double backward (grad mode off) of the Function
    pair never rebuilds the attention through the torch reference, and
    its result matches the reference's double backward."""
    (q, k, v, w), ptr, batch = _inputs(dh)
    _, want = _force_style(
        lambda a, b, c: torch_varlen_attention(a, b, c, batch), q, k, v, w)

    def boom(*a):
        raise AssertionError("_recompute_out called on the kernel route")

    monkeypatch.setattr(va, "_recompute_out", boom)
    _, got = _force_style(
        lambda a, b, c: varlen_attention_fn(a, b, c, ptr, batch),
        q, k, v, w)
    for a, b in zip(got, want):
        assert (a - b).abs().max() < 1e-8


def test_single_cotangent_double_backward(monkeypatch):
    """Only dK is used downstream, so autograd supplies one cotangent
    of three; the absent ones count as zero."""
    (q, k, v, w), ptr, batch = _inputs(16)

    def second(fn):
        x = [t.clone().requires_grad_(True) for t in (q, k, v)]
        gk = torch.autograd.grad((fn(*x) * w).sum(), x[1],
                                 create_graph=True)[0]
        return torch.autograd.grad(gk.square().sum(), x)

    want = second(lambda a, b, c: torch_varlen_attention(a, b, c, batch))

    def boom(*a):
        raise AssertionError("_recompute_out called on the kernel route")

    monkeypatch.setattr(va, "_recompute_out", boom)
    got = second(lambda a, b, c: varlen_attention_fn(a, b, c, ptr, batch))
    for a, b in zip(got, want):
        assert (a - b).abs().max() < 1e-8


def test_third_order_takes_recompute_route(monkeypatch):
    """create_graph=True on the second backward asks for a third order:
    the recompute path runs and the third-order gradients match the
    reference.  Bound: the sibling file allows 1e-10 at first and 1e-8
    at second order in fp64, two decades per differentiation (each one
    multiplies the magnitudes by sums over up to 33 rows); 1e-6 follows
    the same progression."""
    (q, k, v, w), ptr, batch = _inputs(5)
    calls = _count_recompute(monkeypatch)

    def third(fn):
        x, second = _force_style(fn, q, k, v, w, create_graph=True)
        assert all(s.requires_grad for s in second)
        return second, torch.autograd.grad(
            sum(s.square().sum() for s in second), x)

    s1, t1 = third(lambda a, b, c: varlen_attention_fn(a, b, c, ptr, batch))
    assert calls
    s2, t2 = third(lambda a, b, c: torch_varlen_attention(a, b, c, batch))
    for a, b in zip(s1, s2):
        assert (a - b).abs().max() < 1e-8
    for a, b in zip(t1, t2):
        assert (a - b).abs().max() < 1e-6


def test_second_order_switch(monkeypatch):
    """HYDRAGNN_VARLEN_ATTN_BWD2=0 is read at call time, sends the
    double backward through the recompute, and gives the same
    gradients."""
    (q, k, v, w), ptr, batch = _inputs(5)
    calls = _count_recompute(monkeypatch)

    def fn(a, b, c):
        return varlen_attention_fn(a, b, c, ptr, batch)

    _, on = _force_style(fn, q, k, v, w)
    assert not calls
    monkeypatch.setenv("HYDRAGNN_VARLEN_ATTN_BWD2", "0")
    _, off = _force_style(fn, q, k, v, w)
    assert calls
    for a, b in zip(on, off):
        assert (a - b).abs().max() < 1e-8
