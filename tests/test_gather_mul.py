"""gather_mul_sum / gather_mul on the CPU: the pure-torch doubles, the
plans, the closure of the Function pairs under differentiation, and the
SchNet and DimeNet stacks with the fused route on and off (cases and
references: _exact_gather_mul.py)."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact_gather_mul as X  # noqa: E402
from _exact_agg import (DTYPES, F64, N_SEG, csr_of, dtype_id,  # noqa: E402
                        gen, ints)
from hydragnn_amd import ops  # noqa: E402
from hydragnn_amd.ops.gather_mul import (SegmentPlan, gather_mul,  # noqa: E402
                                         gather_mul_sum, path_counts,
                                         reset_path_counts)

CPU = torch.device("cpu")


def test_exported_from_ops():
    assert ops.gather_mul_sum is gather_mul_sum
    assert ops.gather_mul is gather_mul
    assert ops.SegmentPlan is SegmentPlan
    # ops.path_counts stays the PNA one; ours is reachable both ways
    assert "fwd" in ops.path_counts()
    assert set(path_counts()) == {"sum", "mul", "composition"}
    assert ops.gather_mul.path_counts is path_counts


@pytest.mark.parametrize("name", X.LAYOUTS)
@pytest.mark.parametrize("route", X.ROUTES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_int_grid(dtype, route, name):
    reset_path_counts()
    X.check_int(CPU, dtype, route, name)
    counts = path_counts()
    assert counts["composition"] == 2 * len(X.TRAILING)
    assert counts["sum"] == counts["mul"] == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_empty_and_identity(dtype):
    X.check_empty(CPU, dtype)


def test_plan_csr_is_lazy_stable_and_cached():
    index = torch.tensor([5, 2, 5, 0, 2, 5])
    plan = SegmentPlan.from_index(index, 7)
    assert plan._csr is None and plan.size == 7
    assert torch.equal(plan.index, index)
    perm, rowptr = plan.csr()
    want_perm, want_rowptr = csr_of(index, 7)
    assert torch.equal(perm, want_perm) and torch.equal(rowptr, want_rowptr)
    assert plan.csr()[0] is perm and plan.csr()[1] is rowptr
    srt = SegmentPlan.from_index(index.sort().values, 7, sorted_index=True)
    assert srt.csr()[0] is None and torch.equal(srt.csr()[1], want_rowptr)


def test_shape_mismatches_raise():
    sp = SegmentPlan.from_index(torch.tensor([0, 1, 1]), 2)
    dp = SegmentPlan.from_index(torch.tensor([2, 0, 1]), 3)
    x, w = torch.ones(2, 4), torch.ones(3, 4)
    gather_mul_sum(x, w, sp, dp)
    with pytest.raises(ValueError):
        gather_mul_sum(torch.ones(3, 4), w, sp, dp)       # rows of x
    with pytest.raises(ValueError):
        gather_mul_sum(x, torch.ones(2, 4), sp, dp)       # rows of w
    with pytest.raises(ValueError):
        gather_mul_sum(x, torch.ones(3, 5), sp, dp)       # trailing
    with pytest.raises(ValueError):
        gather_mul_sum(x, w.double(), sp, dp)             # dtype
    with pytest.raises(ValueError):
        gather_mul(x, torch.ones(2, 4), sp, dp)           # rows of b
    with pytest.raises(ValueError):
        gather_mul_sum(x, w, sp, SegmentPlan.from_index(
            torch.tensor([0, 1]), 3))                     # edge counts
    with pytest.raises(TypeError):
        gather_mul_sum(x, w, sp.index, dp)


def _small(route="perm"):
    g = gen("gm_gradcheck", route)
    src = torch.randint(0, 5, (9,), generator=g)
    dst = torch.randint(0, 4, (9,), generator=g)
    if route == "sorted":
        dst = dst.sort().values
    sp, dp = X.plans(src, dst, 5, 4, CPU, route)
    x = torch.randn(5, 3, generator=g, dtype=F64, requires_grad=True)
    w = torch.randn(9, 3, generator=g, dtype=F64, requires_grad=True)
    b = torch.randn(4, 3, generator=g, dtype=F64, requires_grad=True)
    return x, w, b, sp, dp


@pytest.mark.parametrize("route", X.ROUTES)
def test_gradcheck_and_gradgradcheck(route):
    x, w, b, sp, dp = _small(route)
    f_sum = lambda x, w: gather_mul_sum(x, w, sp, dp)  # noqa: E731
    f_mul = lambda a, b: gather_mul(a, b, sp, dp)      # noqa: E731
    assert torch.autograd.gradcheck(f_sum, (x, w))
    assert torch.autograd.gradgradcheck(f_sum, (x, w))
    assert torch.autograd.gradcheck(f_mul, (x, b))
    assert torch.autograd.gradgradcheck(f_mul, (x, b))


def test_unrequested_gradients_are_skipped():
    x, w, _, sp, dp = _small()
    reset_path_counts()
    out = gather_mul_sum(x, w.detach(), sp, dp)
    torch.autograd.grad(out.sum(), x)
    # the forward and dx; no product for dw
    assert path_counts()["composition"] == 2


def test_third_order_matches_plain_autograd():
    """d/dx d/dw d/dx of a scalar of the op against autograd of the
    index_select / index_add_ formula."""
    x, w, _, sp, dp = _small()

    def third(op):
        y = (op(x, w) ** 3).sum()
        (g1,) = torch.autograd.grad(y, x, create_graph=True)
        (g2,) = torch.autograd.grad((g1 ** 2).sum(), w, create_graph=True)
        return torch.autograd.grad((g2 ** 2).sum(), (x, w))

    def plain(x, w):
        prod = x.index_select(0, sp.index) * w
        return prod.new_zeros(dp.size, x.shape[1]).index_add(
            0, dp.index, prod)

    got = third(lambda x, w: gather_mul_sum(x, w, sp, dp))
    want = third(plain)
    for a, b in zip(got, want):
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_closure_chain_is_exact(dtype):
    """The chain the device test compares against: on the doubles it
    equals the fp64 chain rounded at the same places."""
    x, w, src, dst = X.closure_case()
    sp, dp = X.plans(src, dst, X.CLOSURE_M, N_SEG, CPU, "perm")
    ref = X.closure_chain(x, w, sp, dp)
    assert max(float(t.abs().max()) for t in ref) < 2 ** 15
    got = X.closure_chain(x.to(dtype), w.to(dtype), sp, dp)
    # out, dx and dw are integers every format here holds
    for a, b in zip(got[:3], ref[:3]):
        assert torch.equal(a.double(), b)


def test_flag_and_the_stacks_defaults(monkeypatch):
    """Unset, each stack follows its measured default (DimeNet on,
    SchNet off); 0 and 1 decide for both."""
    from hydragnn_amd.models import dimenet, schnet
    from hydragnn_amd.ops.gather_mul import fused_messages
    monkeypatch.delenv("HYDRAGNN_GATHER_MUL", raising=False)
    assert fused_messages(True) and not fused_messages(False)
    assert dimenet.FUSED_BY_DEFAULT and not schnet.FUSED_BY_DEFAULT
    monkeypatch.setenv("HYDRAGNN_GATHER_MUL", "0")
    assert not fused_messages(True) and not fused_messages(False)
    monkeypatch.setenv("HYDRAGNN_GATHER_MUL", "1")
    assert fused_messages(True) and fused_messages(False)


@pytest.mark.parametrize("mpnn_type", ["SchNet", "DimeNet"])
def test_models_fused_equals_composition_fp64(mpnn_type, monkeypatch):
    """Energy + forces step in fp64: outputs and parameter gradients of
    the fused route agree with the composition's to 1e-12 relative."""
    from hydragnn_amd.data import Batch
    from hydragnn_amd.utils.datasets.synthetic import lj_dataset
    dataset = lj_dataset(num_samples=4, num_atoms=27, pbc=False)
    model = X.build_model(mpnn_type, dataset).double().train()

    def run():
        return X.energy_force_step(model, X.double_batch(
            Batch.from_data_list([d.clone() for d in dataset])))

    monkeypatch.setenv("HYDRAGNN_GATHER_MUL", "1")
    reset_path_counts()
    out1, grads1 = run()
    assert path_counts()["composition"] > 0      # the route was taken
    monkeypatch.setenv("HYDRAGNN_GATHER_MUL", "0")
    reset_path_counts()
    out0, grads0 = run()
    assert path_counts()["composition"] == 0
    assert set(grads0) == set(grads1) and len(grads0) > 0
    assert X.rel_err(out1, out0) <= 1e-12
    assert X.rel_err(grads1, grads0) <= 1e-12
