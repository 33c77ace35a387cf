"""The pair-affine primitives on wide edge attributes
(csrc/edge_affine_mfma.hip): bf16/f16, D in {32, 96} and H in {64, 192}
on the MFMA kernels, exact on integer data, within twice the torch
doubles on general data, closed at second order, and E_GCL with
edge_dim = 64 under HYDRAGNN_EGNN_FUSED (references: test_edge_affine.py).

Measured on an MI355X, absolute error against fp64 autograd on
unit-normal data; kernels and torch doubles agree to three digits in
every value: bf16 (64, 96) z 0.125, dP 0.049, dr2 0.060, dea 0.122, dw_r
0.097, dW_e 0.126, db 0.090; bf16 (192, 96) 0.125, 0.062, 0.062, 0.125,
0.125, 0.143, 0.089; f16 (192, 32) 7.8e-3, 7.7e-3, 7.7e-3, 0.0156,
0.0155, 0.0156, 0.0137.  Second order, bf16 (64, 32), kernels / doubles
chain (one ulp): dP 1429 / 1687 (3949), dr2 596 / 446 (1003), dea 276 /
213 (395), dw_r 3162 / 2062 (6599), dW_e 444 / 463 (904), db 2083 / 2083
(6000).  E_GCL, flag 1 / flag 0: output 0.0203 / 0.0186,
edge_mlp.0.weight gradient 1.85 / 2.31, node_mlp.0.weight 1.67 / 1.94.
"""

import copy
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_edge_affine as C  # noqa: E402
from _exact_agg import BF, F16, F32, F64, dtype_id, gen, ints, put, same  # noqa: E402
from hydragnn_amd.ops.edge_affine import (  # noqa: E402
    edge_pair_affine, pair_affine_edge, pair_affine_node, pair_affine_param,
    path_counts, reset_path_counts, torch_edge_pair_affine, wide_envelope)

DEV = torch.device("cuda:0")
NAMES = ("z", "dP", "dr2", "dea", "dw_r", "dW_e", "db")


@pytest.fixture(autouse=True)
def _counts():
    reset_path_counts()
    yield


def wide_case(feat, edge_dim, route, normal_as=None):
    """E = 300 over the rows of test_edge_affine.py doubled: two param
    chunks of 150 edges (stages of 64, 64, 22) and five forward tiles,
    the last of 44.  Integers with ea, W_e, w_r, g in {-1, 0, 1}, so
    |z| <= 10 + D and |dea| <= H; or unit normals rounded to `normal_as`."""
    k = gen("edge_affine_wide", feat, edge_dim)
    dst = torch.repeat_interleave(torch.arange(C.N),
                                  2 * torch.tensor(C.ROW_LENS))
    dst = dst[torch.randperm(dst.numel(), generator=k)]
    if route == "sorted":
        dst = dst.sort().values
    n = dst.numel()
    src = torch.randint(0, C.N - 1, (n,), generator=k)
    x = {"P": ints(k, -2, 2, C.N, 2 * feat), "r2": ints(k, 0, 4, n),
         "ea": ints(k, -1, 1, n, edge_dim), "w_r": ints(k, -1, 1, feat),
         "W_e": ints(k, -1, 1, feat, edge_dim), "b": ints(k, -2, 2, feat)}
    x["g"] = ints(k, -1, 1, n, feat)
    if normal_as is not None:
        x = {m: torch.randn(t.shape, generator=k, dtype=F64).to(normal_as)
             .to(F64) for m, t in x.items()}
    return x, src, dst, x.pop("g")


def check_exact(dtype, route, feat, edge_dim, absent=""):
    x0, src, dst, g = wide_case(feat, edge_dim, route)
    x = {m: None if m in absent.split() else t for m, t in x0.items()}
    want = [C.ref_fwd(*x.values(), src, dst, feat), C.ref_node(g, src, dst),
            *C.ref_edge(g, x0["w_r"], x0["W_e"]),
            *C.ref_param(g, x0["r2"], x0["ea"])]
    assert all(C.representable(t, dtype) for t in want)
    sp, dp = C.plans(src, dst, DEV, route)
    d, gd = C.cast(x, DEV, dtype), put(g, DEV, dtype)
    got = [edge_pair_affine(*d.values(), sp, dp), pair_affine_node(gd, sp, dp),
           *pair_affine_edge(gd, d["w_r"], d["W_e"]),
           *pair_affine_param(gd, d["r2"], d["ea"], bias=d["b"] is not None)]
    gone = {"dr2": "w_r", "dw_r": "r2", "db": "b"}
    for name, a, b in zip(NAMES, got, want):
        if x.get(gone.get(name), 0) is None:
            assert a is None, name
        else:
            assert same(a, b, dtype), name
    assert path_counts() == {"fwd": 1, "node": 1, "edge": 1, "param": 1,
                             "composition": 0}


@pytest.mark.parametrize("edge_dim", (32, 96))
@pytest.mark.parametrize("feat", (64, 192))
@pytest.mark.parametrize("route", ("sorted", "perm"))
@pytest.mark.parametrize("dtype", (BF, F16), ids=dtype_id)
def test_exact(dtype, route, feat, edge_dim):
    check_exact(dtype, route, feat, edge_dim)


@pytest.mark.parametrize("absent", ("P", "b", "r2 w_r", "P b"))
def test_absent_groups(absent):
    check_exact(BF, "perm", 64, 32, absent)


def leaves(x, dev, dtype):
    return {m: put(t.detach(), dev, dtype).clone().requires_grad_(True)
            for m, t in x.items()}


def step(fn, d, g):
    for t in d.values():
        t.grad = None
    z = fn(d)
    z.backward(g)
    return [z.detach()] + [t.grad for t in d.values()]


def within(names, got, yard, want, dtype):
    """|got - want| <= 2 |yard - want| + one ulp of dtype at max |want|."""
    for name, a, c, b in zip(names, got, yard, want):
        e_got = float((a.double().cpu() - b).abs().max())
        e_yard = float((c.double().cpu() - b).abs().max())
        one_ulp = torch.finfo(dtype).eps * float(b.abs().max())
        print(f"{name} {dtype}: kernels {e_got:.3e} doubles {e_yard:.3e} "
              f"ulp {one_ulp:.3e}")
        assert e_got <= 2 * e_yard + one_ulp, name


@pytest.mark.parametrize("dtype,feat,edge_dim",
                         ((BF, 64, 96), (F16, 192, 32), (BF, 192, 96)))
def test_general_data(dtype, feat, edge_dim):
    x, src, dst, g = wide_case(feat, edge_dim, "perm", normal_as=dtype)
    sp, dp = C.plans(src, dst, DEV, "perm")
    want = step(lambda d: C.ref_fwd(*d.values(), src, dst, feat),
                leaves(x, "cpu", F64), g)
    d, gd = leaves(x, DEV, dtype), put(g, DEV, dtype)

    def op(d):
        return edge_pair_affine(*d.values(), sp, dp)

    first = [t.clone() for t in step(op, d, gd)]
    yard = step(lambda d: torch_edge_pair_affine(*d.values(), sp, dp,
                                                 src.numel()),
                leaves(x, DEV, dtype), gd)
    within(NAMES, first, yard, want, dtype)
    assert all(torch.equal(a, c) for a, c in zip(first, step(op, d, gd)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(op, d, gd)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static = step(op, d, gd)
    for t in static:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(static, first))
    assert path_counts()["composition"] == 0


def test_second_order_stays_on_the_kernels():
    """Forward, create_graph gradients in r2 and P, backward to all
    leaves: 3 fwd, 2 node, 2 edge, 3 param by the closure table."""
    x, src, dst, _ = wide_case(64, 32, "perm", normal_as=BF)

    def chain(fn, dev, dtype):
        d = leaves(x, dev, dtype)
        sp, dp = C.plans(src, dst, dev, "perm")
        z = fn(*d.values(), sp, dp, src.numel())
        gr, gp = torch.autograd.grad((z * z).sum(), (d["r2"], d["P"]),
                                     create_graph=True)
        ((gr * gr).sum() + (gp * gp).sum()).backward()
        return [t.grad for t in d.values()]

    got = chain(edge_pair_affine, DEV, BF)
    assert path_counts() == {"fwd": 3, "node": 2, "edge": 2, "param": 3,
                             "composition": 0}
    within(NAMES[1:], got, chain(torch_edge_pair_affine, DEV, BF),
           chain(edge_pair_affine, "cpu", F64), BF)


@pytest.mark.parametrize("dtype,feat,edge_dim",
                         ((BF, 64, 48), (F32, 64, 64), (BF, 70, 32)))
def test_outside_the_envelope_runs_the_doubles(dtype, feat, edge_dim):
    assert not wide_envelope(dtype, feat, edge_dim)
    x, src, dst, g = wide_case(feat, edge_dim, "perm")
    sp, dp = C.plans(src, dst, DEV, "perm")
    d, gd = C.cast(x, DEV, dtype), put(g, DEV, dtype)
    got = [edge_pair_affine(*d.values(), sp, dp),
           *pair_affine_edge(gd, d["w_r"], d["W_e"]),
           *pair_affine_param(gd, d["r2"], d["ea"])]
    want = [C.ref_fwd(*x.values(), src, dst, feat),
            *C.ref_edge(g, x["w_r"], x["W_e"]),
            *C.ref_param(g, x["r2"], x["ea"])]
    assert all(same(a, b, dtype) for a, b in zip(got, want))
    assert path_counts() == {"fwd": 0, "node": 0, "edge": 0, "param": 0,
                             "composition": 3}


def test_no_edges_launch_nothing():
    x, src, dst, g = wide_case(64, 32, "perm")
    d = C.cast(dict(x, r2=x["r2"][:0], ea=x["ea"][:0]), DEV, BF)
    gd = put(g[:0], DEV, BF)
    sp, dp = C.plans(src[:0], dst[:0], DEV, "perm")
    got = [edge_pair_affine(*d.values(), sp, dp),
           *pair_affine_edge(gd, d["w_r"], d["W_e"]),
           *pair_affine_param(gd, d["r2"], d["ea"])]
    shapes = [(0, 64), (0,), (0, 32), (64,), (64, 32), (64,)]
    assert [tuple(t.shape) for t in got] == shapes
    assert all(t.dtype == BF and not t.any() for t in got)
    assert not any(path_counts().values())


def test_egcl_edge_dim_64_under_bf16_autocast(monkeypatch):
    """E_GCL(64, 64, 64, edge_dim=64), outputs and parameter gradients
    against the fp64 CPU layer: flag 1 within twice flag 0 plus one bf16
    ulp, on the kernels alone; flag 0 launches none of the family."""
    from hydragnn_amd.models.egnn import E_GCL
    x, src, dst, _ = wide_case(64, 64, "perm", normal_as=F32)
    src = torch.where(src == dst, (src + 1) % C.N, src)
    k = gen("edge_affine_wide_egcl")
    h = torch.randn(C.N, 64, generator=k, dtype=F64)
    pos = torch.randn(C.N, 3, generator=k, dtype=F64)
    torch.manual_seed(5)
    layer = E_GCL(64, 64, 64, edge_dim=64, equivariant=True)

    def run(flag, dev, dtype):
        monkeypatch.setenv("HYDRAGNN_EGNN_FUSED", flag)
        reset_path_counts()
        net = copy.deepcopy(layer).to(dev, dtype)
        with torch.autocast("cuda", dtype=BF, enabled=dtype == F32):
            out, new_pos = net(put(h, dev, dtype), put(pos, dev, dtype),
                               put(torch.stack([src, dst]), dev),
                               put(x["ea"], dev, dtype))
        ((out * out).sum() + (new_pos * new_pos).sum()).backward()
        return [out.detach(), new_pos.detach()] + \
            [p.grad for p in net.parameters()]

    want = run("0", "cpu", F64)
    comp = run("0", DEV, F32)
    assert not any(path_counts().values())
    fused = run("1", DEV, F32)
    assert path_counts()["fwd"] >= 1 and path_counts()["composition"] == 0
    names = ["out", "pos"] + [n for n, _ in layer.named_parameters()]
    within(names, fused, comp, want, BF)
