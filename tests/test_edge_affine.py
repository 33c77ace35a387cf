"""edge_pair_affine and its companions on the CPU: the doubles against
fp64 einsum references, both derivative orders with absent groups, the
argument checks, and E_GCL with HYDRAGNN_EGNN_FUSED on against off.
Cases and references are shared with test_gpu_edge_affine.py."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _exact_agg import DTYPES, F64, dtype_id, gen, ints, put, same  # noqa: E402
from hydragnn_amd import ops  # noqa: E402
from hydragnn_amd.ops.edge_affine import (  # noqa: E402
    edge_pair_affine, fused_egnn, pair_affine_edge, pair_affine_node,
    pair_affine_param, path_counts, reset_path_counts)
from hydragnn_amd.ops.gather_mul import SegmentPlan  # noqa: E402

N = 9
# edges per dst row: empty, single, both sides of a four-deep
# look-ahead, long; node 8 is never a source
ROW_LENS = (0, 1, 4, 5, 64, 19, 19, 19, 19)
GROUPS = ("P", "r2", "ea", "w_r", "W_e", "b")


def ref_fwd(P, r2, ea, w_r, W_e, b, src, dst, feat):
    """fp64, by plain indexing and einsum; None groups are left out."""
    z = torch.zeros(src.numel(), feat, dtype=F64)
    if P is not None:
        z = z + P[dst, :feat] + P[src, feat:]
    if r2 is not None:
        z = z + torch.einsum("e,f->ef", r2, w_r)
    if ea is not None:
        z = z + torch.einsum("ek,fk->ef", ea, W_e)
    return z if b is None else z + b


def ref_node(g, src, dst):
    zero = torch.zeros(N, g.shape[1], dtype=F64)
    return torch.cat([zero.index_add(0, dst, g), zero.index_add(0, src, g)], 1)


def ref_edge(g, w_r, W_e):
    return (torch.einsum("ef,f->e", g, w_r),
            None if W_e is None else torch.einsum("ef,fk->ek", g, W_e))


def ref_param(g, r2, ea):
    return (torch.einsum("e,ef->f", r2, g),
            None if ea is None else torch.einsum("ek,ef->fk", ea, g),
            g.sum(0))


def int_case(feat, edge_dim, route):
    """Integers: P, ea, W_e, b in [-2, 2], r2 in [0, 4], w_r and the
    cotangent g in {-1, 0, 1}; the callers assert that the dtype holds
    every expected value.  Returns the six groups, src, dst, g."""
    k = gen("edge_affine", feat, edge_dim)
    dst = torch.repeat_interleave(torch.arange(N), torch.tensor(ROW_LENS))
    dst = dst[torch.randperm(dst.numel(), generator=k)]
    if route == "sorted":
        dst = dst.sort().values
    n_edges = dst.numel()
    src = torch.randint(0, N - 1, (n_edges,), generator=k)
    x = {"P": ints(k, -2, 2, N, 2 * feat), "r2": ints(k, 0, 4, n_edges),
         "ea": ints(k, -2, 2, n_edges, edge_dim) if edge_dim else None,
         "w_r": ints(k, -1, 1, feat),
         "W_e": ints(k, -2, 2, feat, edge_dim) if edge_dim else None,
         "b": ints(k, -2, 2, feat)}
    return x, src, dst, ints(k, -1, 1, n_edges, feat)


def representable(ref, dtype):
    return ref is None or torch.equal(ref.to(dtype).to(F64), ref)


def plans(src, dst, dev, route):
    return (SegmentPlan.from_index(put(src, dev), N),
            SegmentPlan.from_index(put(dst, dev), N,
                                   sorted_index=(route == "sorted")))


def cast(x, dev, dtype):
    return {k: None if t is None else put(t, dev, dtype) for k, t in x.items()}


def check_int(dev, dtype, route, feat, edge_dim):
    """All four primitives on the integer case, bit for bit."""
    x, src, dst, g = int_case(feat, edge_dim, route)
    sp, dp = plans(src, dst, dev, route)
    want = [ref_fwd(*x.values(), src, dst, feat), ref_node(g, src, dst),
            *ref_edge(g, x["w_r"], x["W_e"]), *ref_param(g, x["r2"], x["ea"])]
    assert all(representable(t, dtype) for t in want)
    d, gd = cast(x, dev, dtype), put(g, dev, dtype)
    got = [edge_pair_affine(*d.values(), sp, dp), pair_affine_node(gd, sp, dp),
           *pair_affine_edge(gd, d["w_r"], d["W_e"]),
           *pair_affine_param(gd, d["r2"], d["ea"])]
    for name, a, b in zip(("z", "dP", "dr2", "dea", "dw_r", "dW_e", "db"),
                          got, want):
        assert (a is None and b is None) or same(a, b, dtype), name


@pytest.mark.parametrize("edge_dim", (0, 3))
@pytest.mark.parametrize("route", ("sorted", "perm"))
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_doubles_equal_the_reference(dtype, route, edge_dim):
    reset_path_counts()
    check_int("cpu", dtype, route, 6, edge_dim)
    assert path_counts() == {"fwd": 0, "node": 0, "edge": 0, "param": 0,
                             "composition": 4}


@pytest.mark.parametrize("absent", ("", "P", "r2 w_r", "ea W_e", "b",
                                    "P ea W_e b"))
def test_gradcheck_and_gradgradcheck(absent):
    """H = 3, D = 2, E = 12, unsorted edges, each group absent in turn."""
    k = gen("edge_affine_gradcheck")
    dst = torch.tensor([1, 2, 2, 3, 3, 3, 4, 6, 6, 7, 8, 8])[
        torch.randperm(12, generator=k)]
    src = torch.randint(0, N, (12,), generator=k)
    sp, dp = plans(src, dst, "cpu", "perm")
    shapes = dict(zip(GROUPS, ((N, 6), (12,), (12, 2), (3,), (3, 2), (3,))))
    x = {n: None if n in absent.split() else
         torch.randn(s, generator=k, dtype=F64).requires_grad_(True)
         for n, s in shapes.items()}
    g = torch.randn(12, 3, generator=k, dtype=F64).requires_grad_(True)
    live = [n for n in GROUPS if x[n] is not None]

    def some(outs):
        return tuple(t for t in outs if t is not None)

    def fwd(*a):
        return edge_pair_affine(*(dict(x, **dict(zip(live, a)))[n]
                                  for n in GROUPS), sp, dp)

    cases = [(fwd, [x[n] for n in live]),
             (lambda a: pair_affine_node(a, sp, dp), [g])]
    if x["w_r"] is not None or x["W_e"] is not None:
        cases.append((lambda a: some(pair_affine_edge(a, x["w_r"], x["W_e"])),
                      [g]))
    cases.append((lambda a: some(pair_affine_param(
        a, x["r2"], x["ea"], bias=x["b"] is not None)), [g]))
    for f, leaves in cases:
        assert torch.autograd.gradcheck(f, leaves)
        assert torch.autograd.gradgradcheck(f, leaves)


def test_mismatches_raise():
    x, src, dst, g = int_case(2, 3, "perm")
    sp, dp = plans(src, dst, "cpu", "perm")
    edge_pair_affine(*x.values(), sp, dp)
    bad = [dict(x, P=x["P"][:, :3]), dict(x, r2=x["r2"][:-1]),
           dict(x, ea=x["ea"][:, :2]), dict(x, w_r=x["w_r"][:1]),
           dict(x, W_e=None), dict(x, r2=None), dict(x, b=x["b"].float()),
           dict(x, b=x["b"][:1]), dict(x, P=x["P"][:-1])]
    for args in bad:
        with pytest.raises(ValueError):
            edge_pair_affine(*args.values(), sp, dp)
    with pytest.raises(TypeError):
        edge_pair_affine(*x.values(), src, dp)
    for call in (lambda: edge_pair_affine(None, None, None, None, None, x["b"]),
                 lambda: pair_affine_node(g[:-1], sp, dp),
                 lambda: pair_affine_edge(g, x["w_r"][:1], None),
                 lambda: pair_affine_param(g, x["r2"], x["ea"][:-1])):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("equivariant", (False, True))
@pytest.mark.parametrize("edge_dim", (0, 3))
def test_egcl_flag_on_equals_off(edge_dim, equivariant, monkeypatch):
    """Outputs, parameter gradients and a force-style second order of
    one fp64 layer: only the association of the K-sum differs, so the
    project's fp64 bound of 1e-12 relative holds."""
    from hydragnn_amd.models.egnn import E_GCL
    monkeypatch.delenv("HYDRAGNN_EGNN_FUSED", raising=False)
    assert fused_egnn(True) and not fused_egnn(False)
    assert ops.edge_pair_affine is edge_pair_affine
    k = gen("edge_affine_egcl", edge_dim, equivariant)
    torch.manual_seed(5)
    layer = E_GCL(8, 8, 8, edge_dim=edge_dim, equivariant=equivariant).double()
    h = torch.randn(N, 8, generator=k, dtype=F64)
    pos = torch.randn(N, 3, generator=k, dtype=F64).requires_grad_(True)
    x, src, dst, _ = int_case(2, edge_dim, "perm")
    src = torch.where(src == dst, (src + 1) % N, src)
    got = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("HYDRAGNN_EGNN_FUSED", flag)
        layer.zero_grad()
        reset_path_counts()
        out, new_pos = layer(h, pos, torch.stack([src, dst]), x["ea"])
        assert path_counts()["composition"] == int(flag)
        energy = (out * out).sum() + (new_pos * new_pos).sum()
        force, = torch.autograd.grad(energy, pos, create_graph=True)
        (energy + (force * force).sum()).backward()
        got[flag] = [out.detach(), new_pos.detach(), force.detach()] + \
            [p.grad.clone() for p in layer.parameters()]
    for a, b in zip(got["1"], got["0"]):
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
