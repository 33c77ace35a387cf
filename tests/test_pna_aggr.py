"""Fused PNA aggregation on the CPU: the pure-torch doubles of the three
entry points behind `pna_aggregate`, checked exactly where the answer
is determined and against derived bounds elsewhere (cases, references
and bounds: _exact_pna.py)."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact_pna as X  # noqa: E402
from _exact_agg import (BF, DTYPES, F32, F64, N_SEG, dtype_id,  # noqa: E402
                        within_one_ulp)
from hydragnn_amd import ops  # noqa: E402
from hydragnn_amd.ops import pna_aggr  # noqa: E402

CPU = torch.device("cpu")
ROUTES = ("sorted", "perm")


def test_exported():
    for name in ("pna_aggregate", "pna_scale", "path_counts",
                 "reset_path_counts"):
        assert name in ops.__all__ and hasattr(ops, name)


@pytest.mark.parametrize("name", X.LAYOUTS)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_int_blocks(dtype, route, name):
    X.check_int_blocks(ops, CPU, dtype, route, name)


@pytest.mark.parametrize("aggs", [("std",), ("max", "sum"),
                                  ("var", "min", "mean", "sum", "max",
                                   "std")])
def test_subsets_keep_the_given_order(aggs):
    src, index = X.int_case("gaps", (3,))
    out, _ = X.run(ops, "perm", src.to(F32), index, N_SEG, aggs,
                   ("identity",), CPU)
    got = X.split_blocks(out, 1, len(aggs))[:, 0]
    for a, agg in enumerate(aggs):
        ref = X.ref_block(agg, src, index, N_SEG)
        assert torch.allclose(got[:, a].to(F64), ref, rtol=1e-5, atol=0), agg


def test_rejects_bad_aggregators():
    src, index = X.int_case("single", (3,))
    for aggs in ((), ("sum", "sum"), ("median",)):
        with pytest.raises(ValueError):
            X.run(ops, "sorted", src.to(F32), index, N_SEG, aggs,
                  ("identity",), CPU)
    with pytest.raises(ValueError):
        ops.pna_scale(torch.zeros(3, dtype=torch.long), ("cubic",), 1.0,
                      1.0, F32)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_extremes_and_routing(dtype, route):
    for name, trailing in (("gaps", (3,)), ("long", (1,)),
                           ("single", (4, 3)), ("one_row", (3,))):
        X.check_extremes(ops, CPU, dtype, route, name, trailing)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_pairs_var_exact_std_bounded(dtype, route):
    X.check_pairs(ops, CPU, dtype, route)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_general_var_std_within_derived_bound(dtype):
    X.check_general(ops, CPU, dtype, "perm")


def test_bf16_shifted_std_within_one_ulp():
    """The case of the issue: E[x^2] - E[x]^2 in bf16 is off by more
    than the answer here; the centered form rounded once is within one
    bf16 ulp of the truth."""
    src, index, n = X.shifted_case()
    out, _ = X.run(ops, "perm", src.to(BF), index, n, X.DEFAULT_AGGS,
                   ("identity",), CPU)
    std = X.split_blocks(out, 1, 4)[:, 0, 3]
    assert within_one_ulp(std, X.ref_block("std", src, index, n), BF)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_empty(dtype):
    X.check_empty(ops, CPU, dtype)


def test_sorted_and_perm_routes_agree():
    x64, index, c64, _ = X.grad_case(F32, "long")
    o = torch.argsort(index, stable=True)
    res = {}
    for route in ROUTES:
        xs, idx = X.route_case(route, x64, index)
        x = xs.to(F32).requires_grad_(True)
        out, _ = X.run(ops, route, x, idx, N_SEG, X.DEFAULT_AGGS,
                       X.DEFAULT_SCALERS, CPU)
        (dx,) = torch.autograd.grad(out, x, torch.ones_like(out))
        res[route] = (out.detach(), dx)
    assert torch.equal(res["sorted"][0], res["perm"][0])
    assert torch.equal(res["sorted"][1], res["perm"][1][o])


def test_scale_matches_module_formulas():
    rowptr = torch.tensor([0, 0, 1, 4, 9])
    s = ops.pna_scale(rowptr, X.ALL_SCALERS, 2.0, 0.5, BF)
    d = torch.tensor([1., 1., 3., 5.])
    assert s.dtype == F32 and not s.requires_grad
    want = torch.stack([torch.ones(4), (d + 1).log() / 0.5,
                        0.5 / (d + 1).log(), d / 2.0, 2.0 / d], 1)
    assert torch.allclose(s, want, rtol=1e-6)
    assert ops.pna_scale(rowptr, ("linear",), 2.0, 0.5, F64).dtype == F64


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", [F32, F64], ids=dtype_id)
def test_gradients_match_fp64_autograd(dtype, route):
    aggs = ("sum", "mean", "min", "max", "std", "var")
    got, ref = X.grads_of(ops, CPU, dtype, route, aggs, X.ALL_SCALERS)
    tol = 1e-4 if dtype == F32 else 1e-11
    for name, a, b in zip(("out", "dx", "gx", "hw"), got, ref):
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= tol * scale, name


def _tiny(route):
    """Tiny fp64 case with distinct values: unique args."""
    g = X.gen("pna_tiny")
    index = torch.tensor([2, 0, 2, 3, 0, 2, 3, 2])
    x = torch.randn(8, 2, generator=g, dtype=F64)
    x, index = X.route_case(route, x, index)
    rowptr, perm = X.operands(route, index, 5, CPU)
    scale = ops.pna_scale(rowptr, X.ALL_SCALERS, X.AVG_LIN, X.AVG_LOG, F64)
    return x, rowptr, perm, scale


@pytest.mark.parametrize("route", ROUTES)
def test_gradcheck_and_gradgradcheck(route):
    x, rowptr, perm, scale = _tiny(route)
    aggs = ("sum", "mean", "min", "max", "std", "var")
    x.requires_grad_(True)

    def fn(t):
        return ops.pna_aggregate(t, rowptr, scale, aggs, perm=perm)

    assert torch.autograd.gradcheck(fn, (x,))
    assert torch.autograd.gradgradcheck(fn, (x,))


def test_third_order_fallback_equals_second_order_double():
    """With grad mode on inside the double backward the op
    differentiates the torch double of the first order; with it off it
    runs the closed-form second-order double.  Same numbers."""
    x, rowptr, perm, scale = _tiny("perm")
    aggs = ("mean", "min", "max", "std", "var")
    g = X.gen("pna_tiny_cot")
    res = []
    for create_graph in (False, True):
        xi = x.clone().requires_grad_(True)
        out = ops.pna_aggregate(xi, rowptr, scale, aggs, perm=perm)
        g.manual_seed(7)
        w = torch.randn(out.shape, generator=g, dtype=F64,
                        ).requires_grad_(True)
        c = torch.randn(x.shape, generator=g, dtype=F64)
        (dx,) = torch.autograd.grad(out, xi, w, create_graph=True)
        ops.reset_path_counts()
        res.append(torch.autograd.grad(dx, (xi, w), c,
                                       create_graph=create_graph))
        assert ops.path_counts()["composition"] >= 1
    for a, b in zip(*res):
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-14)
    # and the result of the fallback is differentiable once more
    assert res[1][0].requires_grad


def test_rank3_source_flattens_trailing_dims():
    src, index = X.int_case("gaps", (4, 3))
    out3, _ = X.run(ops, "perm", src.to(F32), index, N_SEG, ("sum", "max"),
                    ("identity", "linear"), CPU)
    out2, _ = X.run(ops, "perm", src.to(F32).reshape(-1, 12), index, N_SEG,
                    ("sum", "max"), ("identity", "linear"), CPU)
    assert out3.shape == (N_SEG, 2 * 2 * 12) and torch.equal(out3, out2)


def test_module_cpu_path_is_the_composition():
    """CPU tensors keep the module's aggregator-by-aggregator path."""
    from hydragnn_amd.models.layers import DegreeScalerAggregation
    mod = DegreeScalerAggregation(list(X.DEFAULT_AGGS),
                                  list(X.DEFAULT_SCALERS),
                                  torch.tensor([0, 3, 5, 2]))
    src, index = X.int_case("gaps", (3,))
    ops.reset_path_counts()
    out = mod(src.to(F32), index, N_SEG)
    assert out.shape == (N_SEG, 4 * 4 * 3)
    counts = ops.path_counts()
    assert counts["composition"] == 1 and counts["fwd"] == 0
    assert pna_aggr.acc_dtype(BF) == F32
