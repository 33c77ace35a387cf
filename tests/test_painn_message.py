"""painn_message on the CPU: the pure-torch doubles against a plain fp64
reference, gradcheck / gradgradcheck, and the argument checks.  The case
and the reference here also serve test_gpu_painn_message.py."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _exact_agg import DTYPES, F64, dtype_id, gen, ints, put, same  # noqa: E402
from hydragnn_amd import ops  # noqa: E402
from hydragnn_amd.ops.gather_mul import SegmentPlan  # noqa: E402
from hydragnn_amd.ops.painn_message import (fused_painn,  # noqa: E402
                                            painn_message, path_counts,
                                            reset_path_counts,
                                            torch_painn_message_bwd)

N = 9
# edges per dst row: empty, single, both sides of a four-deep
# look-ahead, long; node 8 is never a source
ROW_LENS = (0, 1, 4, 5, 64, 19, 19, 19, 19)


def ref_fwd(phi, w, v, u, src, dst):
    """(ds, dv) in fp64 by plain indexing and index_add_."""
    feat = v.shape[2]
    gate = w * phi[src]
    msg = gate[:, None, :feat] * v[src] + \
        gate[:, None, feat:2 * feat] * u[:, :, None]
    dv = torch.zeros(N, 3, feat, dtype=F64).index_add_(0, dst, msg)
    ds = torch.zeros(N, feat, dtype=F64).index_add_(0, dst,
                                                    gate[:, 2 * feat:])
    return ds, dv


def ref_grads(ops_, src, dst, gs, gv):
    """(dphi, dw, dv, du) of the reference by fp64 autograd."""
    leaves = [t.clone().requires_grad_(True) for t in ops_]
    ds, dv = ref_fwd(*leaves, src, dst)
    return torch.autograd.grad((ds, dv), leaves, (gs, gv))


def int_case(feat, route, lens=ROW_LENS):
    """Integer operands and cotangents: phi, v, gs, gv in [-2, 2], w and
    u in [-1, 1].  Every partial sum is an integer far below 2^24, and
    every output and gradient stays an integer of at most 256 in
    magnitude, which bf16 holds exactly (asserted by the callers through
    `representable`).  Returns (phi, w, v, u), src, dst, gs, gv."""
    g = gen("painn_message", feat)
    dst = torch.repeat_interleave(torch.arange(N), torch.tensor(lens))
    dst = dst[torch.randperm(dst.numel(), generator=g)]
    if route == "sorted":
        dst = dst.sort().values
    n_edges = dst.numel()
    src = torch.randint(0, N - 1, (n_edges,), generator=g)
    operands = (ints(g, -2, 2, N, 3 * feat), ints(g, -1, 1, n_edges, 3 * feat),
                ints(g, -2, 2, N, 3, feat), ints(g, -1, 1, n_edges, 3))
    return (operands, src, dst, ints(g, -2, 2, N, feat),
            ints(g, -2, 2, N, 3, feat))


def representable(ref, dtype):
    return torch.equal(ref.to(dtype).to(F64), ref)


def plans(src, dst, dev, route):
    return (SegmentPlan.from_index(put(src, dev), N),
            SegmentPlan.from_index(put(dst, dev), N,
                                   sorted_index=(route == "sorted")))


@pytest.mark.parametrize("route", ("sorted", "perm"))
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_doubles_equal_the_reference(dtype, route):
    operands, src, dst, gs, gv = int_case(6, route)
    sp, dp = plans(src, dst, "cpu", route)
    want = ref_fwd(*operands, src, dst) + ref_grads(operands, src, dst,
                                                    gs, gv)
    assert all(representable(t, dtype) for t in want)
    x = [t.to(dtype) for t in operands]
    reset_path_counts()
    ds, dv = painn_message(*x, sp, dp)
    none, dv2 = painn_message(*x, sp, dp, scalar=False)
    assert path_counts() == {"fwd": 0, "bwd_node": 0, "bwd_edge": 0,
                             "composition": 2}
    assert none is None and torch.equal(dv, dv2)
    got = (ds, dv) + torch_painn_message_bwd(*x, gs.to(dtype), gv.to(dtype),
                                             sp, dp)
    for name, a, b in zip(("ds", "dv", "dphi", "dw", "dv_in", "du"), got,
                          want):
        assert same(a, b, dtype), f"{name} {dtype} {route}"


@pytest.mark.parametrize("scalar", (True, False))
def test_gradcheck_and_gradgradcheck(scalar):
    """F = 3, E = 12, rows 0 and 5 empty, unsorted edges."""
    g = gen("painn_message_gradcheck")
    dst = torch.tensor([1, 2, 2, 3, 3, 3, 4, 6, 6, 7, 8, 8])[
        torch.randperm(12, generator=g)]
    src = torch.randint(0, N, (12,), generator=g)
    sp, dp = plans(src, dst, "cpu", "perm")
    x = [torch.randn(s, generator=g, dtype=F64).requires_grad_(True)
         for s in ((N, 9), (12, 9), (N, 3, 3), (12, 3))]

    def f(*a):
        out = painn_message(*a, sp, dp, scalar=scalar)
        return out if scalar else out[1]

    assert torch.autograd.gradcheck(f, x)
    assert torch.autograd.gradgradcheck(f, x)


def test_mismatches_raise():
    (phi, w, v, u), src, dst, _, _ = int_case(2, "perm", lens=(1,) * N)
    sp, dp = plans(src, dst, "cpu", "perm")
    painn_message(phi, w, v, u, sp, dp)
    bad = [(phi[:, :5], w, v, u), (phi, w[:-1], v, u), (phi, w, v[:, :2], u),
           (phi, w, v.reshape(N, 6), u), (phi, w, v, u[:, :2]),
           (phi.float(), w, v, u), (phi, w, v, u.float()), (phi[:-1], w, v, u)]
    for args in bad:
        with pytest.raises(ValueError):
            painn_message(*args, sp, dp)
    with pytest.raises(ValueError):
        painn_message(phi, w, v, u, sp, SegmentPlan.from_index(dst, N + 1))
    with pytest.raises(TypeError):
        painn_message(phi, w, v, u, src, dp)


def test_export_and_flag(monkeypatch):
    assert ops.painn_message is painn_message
    assert ops.painn_message.path_counts is path_counts
    monkeypatch.delenv("HYDRAGNN_PAINN_FUSED", raising=False)
    assert fused_painn(True) and not fused_painn(False)
    monkeypatch.setenv("HYDRAGNN_PAINN_FUSED", "0")
    assert not fused_painn(True)
    monkeypatch.setenv("HYDRAGNN_PAINN_FUSED", "1")
    assert fused_painn(False)
