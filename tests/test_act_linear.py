"""act_linear on the CPU: the pure-torch doubles and the two Functions'
closure under differentiation against plain linear(silu(h)) in fp64, the
fallback orders, the switch, the envelope and the MACE blocks'
state_dict (helpers: _exact_act_linear.py)."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact_act_linear as X  # noqa: E402
from hydragnn_amd.ops import act_linear as al  # noqa: E402

F64 = torch.float64
CASES = [(5, 64, 64), (300, 128, 64)]


def _operands(E, N, K, bias, seed=0):
    gen = torch.Generator().manual_seed(seed)
    h = (2 * torch.randn(E, K, generator=gen, dtype=F64)).requires_grad_()
    W = (torch.randn(N, K, generator=gen, dtype=F64) / 8).requires_grad_()
    b = torch.randn(N, generator=gen, dtype=F64).requires_grad_() \
        if bias else None
    r = torch.randn(E, N, generator=gen, dtype=F64)
    return h, W, b, r


def _close(got, ref):
    assert got is not None and got.shape == ref.shape
    tol = 1e-12 * max(float(ref.abs().max()), 1e-300)
    assert float((got - ref).abs().max()) <= tol


@pytest.fixture(autouse=True)
def _switch_unset(monkeypatch):
    monkeypatch.delenv("HYDRAGNN_ACT_LINEAR", raising=False)
    al.reset_path_counts()


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("E,N,K", CASES)
def test_flagship_pattern_matches_composition(E, N, K, bias):
    h, W, b, r = _operands(E, N, K, bias)
    y, first, second = X.flagship(al.act_linear, h, W, b, r)
    y0, first0, second0 = X.flagship(X.composition, h, W, b, r)
    assert type(y.grad_fn).__name__.startswith("_ActLinear")
    _close(y, y0)
    for got, ref in zip(first + second, first0 + second0):
        _close(got, ref)
    counts = al.path_counts()
    assert counts["composition"] > 0
    assert all(v == 0 for k, v in counts.items() if k != "composition")


@pytest.mark.parametrize("E,N,K", CASES)
def test_primitive_doubles_match_formulas(E, N, K):
    h, W, b, r = _operands(E, N, K, True)
    h, W, b = h.detach(), W.detach(), b.detach()
    gen = torch.Generator().manual_seed(1)
    u = torch.randn(E, K, generator=gen, dtype=F64)
    gW_lin = r @ W
    _close(al.torch_act_linear(h, W, b), X.phi(h) @ W.t() + b)
    _close(al.torch_dgrad(r, W, h), gW_lin * X.dphi(h))
    _close(al.torch_dgrad_dg(u, W, h), (u * X.dphi(h)) @ W.t())
    _close(al.torch_dgrad_dh(u, r, W, h), u * gW_lin * X.d2phi(h))
    gW, gb = al.torch_wgrad(r, h, None, True)
    _close(gW, r.t() @ X.phi(h))
    _close(gb, r.sum(0))
    gW, gb = al.torch_wgrad(r, h, u)
    _close(gW, r.t() @ (u * X.dphi(h)))
    assert gb is None
    _close(al.torch_wgrad(r, h, act=False)[0], r.t() @ h)


@pytest.mark.parametrize("E,N,K", CASES)
def test_cotangent_on_a_weight_gradient(E, N, K):
    h, W, b, r = _operands(E, N, K, True)
    out = []
    for fn in (al.act_linear, X.composition):
        e = (fn(h, W, b) * r).sum()
        gW, gb = torch.autograd.grad(e, (W, b), create_graph=True)
        loss = (gW ** 2).sum() + (gb ** 3).sum()
        out.append(torch.autograd.grad(loss, (h, W), allow_unused=True))
    _close(out[0][0], out[1][0])
    # e is linear in W: no path from its weight gradient back to W
    assert out[1][1] is None or float(out[1][1].abs().max()) == 0
    assert out[0][1] is None or float(out[0][1].abs().max()) == 0


@pytest.mark.parametrize("E,N,K", CASES)
def test_third_order(E, N, K):
    h, W, b, r = _operands(E, N, K, True)
    out = []
    for fn in (al.act_linear, X.composition):
        e = (fn(h, W, b) * r).sum()
        (gh,) = torch.autograd.grad(e, h, create_graph=True)
        (gg,) = torch.autograd.grad((gh ** 2).sum(), h, create_graph=True)
        out.append(torch.autograd.grad((gg ** 2).sum(), (h, W)))
    for got, ref in zip(*out):
        _close(got, ref)


def test_switch_selects_the_route_the_counters_report(monkeypatch):
    h, W, b, r = _operands(300, 64, 64, True)
    monkeypatch.setenv("HYDRAGNN_ACT_LINEAR", "0")
    assert not al.fused_route()
    y = al.act_linear(h, W, b)
    assert not type(y.grad_fn).__name__.startswith("_ActLinear")
    assert torch.equal(y, X.composition(h, W, b))
    assert al.path_counts()["composition"] == 1
    monkeypatch.setenv("HYDRAGNN_ACT_LINEAR", "1")
    assert al.fused_route() and al.fused_route(default=False)
    y = al.act_linear(h, W, b)
    assert type(y.grad_fn).__name__.startswith("_ActLinear")
    # a CPU tensor is outside the kernels' reach: the double ran
    assert al.path_counts()["composition"] == 2
    monkeypatch.delenv("HYDRAGNN_ACT_LINEAR")
    assert al.fused_route() and not al.fused_route(default=False)


def test_envelope():
    for E, N, K, ok in [(256, 64, 64, True), (255, 64, 64, False),
                        (332668, 256, 64, True), (1000, 320, 64, True),
                        (1000, 384, 64, False), (1000, 64, 320, False),
                        (1000, 32, 64, False),
                        (1000, 96, 64, False), (1000, 64, 96, False),
                        (1000, 192, 256, True), (0, 64, 64, False)]:
        assert al.in_envelope(E, N, K) is ok, (E, N, K)
    with pytest.raises(ValueError):
        al.act_linear(torch.zeros(4, 8), torch.zeros(3, 7))


def test_mace_blocks_keep_their_state_dict_and_values():
    from hydragnn_amd.models.mace.blocks import (
        RealAgnosticAttResidualInteractionBlock as Att,
        RealAgnosticResidualInteractionBlock as Res)
    torch.manual_seed(0)
    for cls, lmax_node, paths in [(Res, 0, 2), (Att, 0, 2), (Att, 1, 5)]:
        blk = cls(64, lmax_node, 2, 1, 8, 20.0)
        keys = [k for k in blk.state_dict() if k.startswith("radial_mlp")]
        assert keys == [f"radial_mlp.{i}.{p}" for i in (0, 2, 4, 6)
                        for p in ("weight", "bias")]
        assert blk.radial_mlp[6].out_features == 64 * paths
        # off the kernels' reach the tail is the Sequential itself
        h = torch.randn(7, 64)
        assert torch.equal(blk._radial_tail(h), blk.radial_mlp[1:](h))


@pytest.mark.parametrize("how", ["backward", "grad_W", "grad_b",
                                 "backward_inputs_W", "grad_h_then_all"])
def test_every_way_of_asking_gets_its_gradients(how):
    """The backwards ask the engine which outputs the running pass uses
    (`_wanted`); whichever way a gradient is asked for, it is there and
    equals the composition's."""
    def run(fn):
        h, W, b, r = _operands(300, 64, 64, True)
        e = (fn(h, W, b) * r).sum()
        if how == "backward":
            e.backward()
            return h.grad, W.grad, b.grad
        if how == "grad_W":
            return torch.autograd.grad(e, W)
        if how == "grad_b":
            return torch.autograd.grad(e, b)
        if how == "backward_inputs_W":
            e.backward(inputs=[W])
            assert h.grad is None and b.grad is None
            return (W.grad,)
        (gh,) = torch.autograd.grad(e, h, create_graph=True)
        ((gh ** 2).sum() + e).backward()
        return h.grad, W.grad, b.grad

    got, ref = run(al.act_linear), run(X.composition)
    assert len(got) == len(ref)
    for a, c in zip(got, ref):
        _close(a, c)
