"""painn_message on the HIP kernels (csrc/painn_message.hip): exact on
integer data in the four dtypes, bit-equal to the composition it
replaces in fp32/fp64, no further from fp64 than twice the composition
on general data, second order through the documented unfused route,
reproducible and capturable, and the PaiNN and PNAEq stacks (case and
reference: test_painn_message.py).

Measured on an MI355X, worst over F and the two routes, absolute error
against fp64 autograd, fused / composition: fp32 dphi 7.7e-6 / 7.2e-6,
dw 1.7e-6 / 1.7e-6, dv 5.6e-6 / 6.2e-6, du 6.0e-6 / 5.6e-6; bf16 dphi
0.12 / 0.37, dw 0.060 / 0.090, dv 0.11 / 0.18, du 0.12 / 0.17.  Stacks,
fp32 parameter gradients against the fp64 CPU model: PAINN 6.39e-8 on
both routes, PNAEq 4.39e-7 on both.
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

import _exact_gather_mul as X  # noqa: E402
import test_painn_message as C  # noqa: E402
from _exact_agg import BF, DTYPES, F32, F64, dtype_id, gen, put, same  # noqa: E402
from hydragnn_amd import ops  # noqa: E402
from hydragnn_amd.ops.painn_message import (painn_message,  # noqa: E402
                                            path_counts, reset_path_counts)

DEV = torch.device("cuda:0")
ROUTES = ("sorted", "perm")
# rows off 16 bytes and L = 8 with idle lanes; the packed path; more than
# 64 element-wise packs; more than 64 packed packs in fp32
FEATS = (6, 64, 70, 264)
NAMES = ("dphi", "dw", "dv", "du")


@pytest.fixture(autouse=True)
def _counts():
    reset_path_counts()
    yield


def leaves(operands, dtype, grad=True):
    return [put(t, DEV, dtype).requires_grad_(grad) for t in operands]


@pytest.mark.parametrize("feat", FEATS)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_exact_forward(dtype, route, feat):
    operands, src, dst, _, _ = C.int_case(feat, route)
    want = C.ref_fwd(*operands, src, dst)
    assert all(C.representable(t, dtype) for t in want)
    sp, dp = C.plans(src, dst, DEV, route)
    x = leaves(operands, dtype, grad=False)
    ds, dv = painn_message(*x, sp, dp)
    assert same(ds, want[0], dtype) and same(dv, want[1], dtype)
    none, dv2 = painn_message(*x, sp, dp, scalar=False)
    assert none is None and torch.equal(dv2, dv)
    assert path_counts() == {"fwd": 2, "bwd_node": 0, "bwd_edge": 0,
                             "composition": 0}


@pytest.mark.parametrize("feat", FEATS)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_exact_first_order(dtype, route, feat):
    operands, src, dst, gs, gv = C.int_case(feat, route)
    want = C.ref_grads(operands, src, dst, gs, gv)
    assert all(C.representable(t, dtype) for t in want)
    sp, dp = C.plans(src, dst, DEV, route)
    cot = (put(gs, DEV, dtype), put(gv, DEV, dtype))
    x = leaves(operands, dtype)
    got = torch.autograd.grad(painn_message(*x, sp, dp), x, cot)
    for name, a, b in zip(NAMES, got, want):
        assert same(a, b, dtype), name
    # u without a gradient: the edge kernel still runs, for dw
    x = leaves(operands, dtype)
    x[3].requires_grad_(False)
    torch.autograd.backward(painn_message(*x, sp, dp), cot)
    assert x[3].grad is None
    for name, t, b in zip(NAMES[:3], x, want):
        assert same(t.grad, b, dtype), name
    assert path_counts() == {"fwd": 2, "bwd_node": 2, "bwd_edge": 2,
                             "composition": 0}


def normal_case(feat, route, dtype):
    """Unit-normal operands and cotangents rounded to `dtype`, as fp64."""
    operands, src, dst, gs, gv = C.int_case(feat, route)
    g = gen("painn_message_normal", feat, route)
    draw = [torch.randn(t.shape, generator=g, dtype=F64).to(dtype).to(F64)
            for t in operands + (gs, gv)]
    return tuple(draw[:4]), src, dst, draw[4], draw[5]


def composition(phi, w, v, u, src, dst, sorted_index):
    """The message of PainnMessage.forward on the generic ops."""
    n, _, feat = v.shape
    filter_out = w * ops.gather(phi, src)
    g0, g1, msg_s = torch.split(filter_out, feat, dim=1)
    vj = ops.gather(v.reshape(-1, 3 * feat), src).view(-1, 3, feat)
    msg_v = vj * g0.unsqueeze(1) + g1.unsqueeze(1) * u.unsqueeze(-1)
    ds = ops.scatter(msg_s, dst, n, "sum", sorted_index=sorted_index)
    dv = ops.scatter(msg_v.reshape(-1, 3 * feat), dst, n, "sum",
                     sorted_index=sorted_index).view(-1, 3, feat)
    return ds, dv


@pytest.mark.parametrize("feat", FEATS)
@pytest.mark.parametrize("dtype", (F32, F64), ids=dtype_id)
def test_forward_equals_todays_path(dtype, feat):
    operands, src, dst, _, _ = normal_case(feat, "sorted", dtype)
    sp, dp = C.plans(src, dst, DEV, "sorted")
    x = leaves(operands, dtype, grad=False)
    ds, dv = painn_message(*x, sp, dp)
    cs, cv = composition(*x, sp.index, dp.index, True)
    assert torch.equal(ds, cs) and torch.equal(dv, cv)


@pytest.mark.parametrize("feat", FEATS)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", (F32, BF), ids=dtype_id)
def test_first_order_general(dtype, route, feat):
    """Each gradient is no further from fp64 autograd than twice the
    composition on the same data, plus one ulp of the output type at
    the gradient's largest magnitude."""
    operands, src, dst, gs, gv = normal_case(feat, route, dtype)
    want = C.ref_grads(operands, src, dst, gs, gv)
    sp, dp = C.plans(src, dst, DEV, route)
    cot = (put(gs, DEV, dtype), put(gv, DEV, dtype))
    x = leaves(operands, dtype)
    fused = torch.autograd.grad(painn_message(*x, sp, dp), x, cot)
    assert path_counts()["composition"] == 0
    comp = torch.autograd.grad(
        composition(*x, sp.index, dp.index, route == "sorted"), x, cot)
    for name, a, c, b in zip(NAMES, fused, comp, want):
        e_fused = float((a.double().cpu() - b).abs().max())
        e_comp = float((c.double().cpu() - b).abs().max())
        one_ulp = torch.finfo(dtype).eps * float(b.abs().max())
        print(f"{name} {dtype} F={feat} {route}: fused {e_fused:.3e} "
              f"composition {e_comp:.3e} ulp {one_ulp:.3e}")
        assert e_fused <= 2 * e_comp + one_ulp, name


def force_chain(x, sp, dp):
    """A force-style second order: the gradients with respect to all
    four operands of |dE/du|^2 + |dE/dw|^2, E = |dv|^2 + |ds|^2."""
    ds, dv = painn_message(*x, sp, dp)
    energy = (dv * dv).sum() + (ds * ds).sum()
    gu, gw = torch.autograd.grad(energy, (x[3], x[1]), create_graph=True)
    return torch.autograd.grad((gu * gu).sum() + (gw * gw).sum(), x)


@pytest.mark.parametrize("feat", (6, 64))
@pytest.mark.parametrize("route", ROUTES)
def test_second_order_matches_the_cpu_double(route, feat):
    operands, src, dst, _, _ = normal_case(feat, route, F64)
    want = force_chain([t.clone().requires_grad_(True) for t in operands],
                       *C.plans(src, dst, "cpu", route))
    reset_path_counts()
    got = force_chain(leaves(operands, F64), *C.plans(src, dst, DEV, route))
    counts = path_counts()
    assert counts["fwd"] == 1 and counts["composition"] >= 1, counts
    for name, a, b in zip(NAMES, got, want):
        rel = float((a.cpu() - b).abs().max() / b.abs().max())
        assert rel <= 1e-12, f"{name} {rel:.3e}"


def step(x, cot, sp, dp):
    for t in x:
        t.grad = None
    out = painn_message(*x, sp, dp)
    torch.autograd.backward(out, cot)
    return [t.detach() for t in out] + [t.grad for t in x]


@pytest.mark.parametrize("feat", (6, 64))
@pytest.mark.parametrize("dtype", (F32, BF), ids=dtype_id)
def test_reruns_routes_and_capture_give_the_same_bits(dtype, feat):
    operands, src, dst, gs, gv = normal_case(feat, "perm", dtype)
    cot = (put(gs, DEV, dtype), put(gv, DEV, dtype))
    x = leaves(operands, dtype)
    sp, dp = C.plans(src, dst, DEV, "perm")
    first = [t.clone() for t in step(x, cot, sp, dp)]
    for a, c in zip(first, step(x, cot, sp, dp)):
        assert torch.equal(a, c)
    # the dst-sorted edge list: the same row sums, and the edge-wise dw
    # and du in the sorted order (the sums over the rows of src run in
    # the renumbered edge order: the same terms in another order)
    o = torch.argsort(dst, stable=True)
    xs = leaves((operands[0], operands[1][o], operands[2], operands[3][o]),
                dtype)
    srt = step(xs, cot, *C.plans(src[o], dst[o], DEV, "sorted"))
    o = put(o, DEV)
    assert torch.equal(first[0], srt[0]) and torch.equal(first[1], srt[1])
    assert torch.equal(first[3][o], srt[3])
    assert torch.equal(first[5][o], srt[5])
    # forward + backward captured into a device graph, plans warm;
    # stream handling as in test_gpu_gather_mul.py
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(x, cot, sp, dp)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static = step(x, cot, sp, dp)
    for _ in range(3):
        for t in static:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, c in zip(static, first):
            assert torch.equal(a, c)
    assert path_counts()["composition"] == 0


@pytest.fixture(scope="module")
def graphs():
    from hydragnn_amd.utils.datasets.synthetic import lj_dataset
    return lj_dataset(num_samples=3, num_atoms=27, pbc=False)


def batch_of(dataset, sort):
    from hydragnn_amd.data import Batch
    batch = Batch.from_data_list([d.clone() for d in dataset])
    if sort:
        batch.sort_edges_by_dst()
        batch["edges_sorted_"] = True
    return batch


@pytest.mark.parametrize("mpnn_type", ("PAINN", "PNAEq"))
def test_stacks(mpnn_type, graphs, monkeypatch):
    """hidden 64, 2 layers, 3 graphs, fp32: on dst-sorted edges the
    flag changes no output bit; the parameter gradients stay within
    twice the composition's distance from the fp64 CPU model plus one
    fp32 ulp; one launch of each kernel per layer."""
    from hydragnn_amd.models import create_model_config
    from hydragnn_amd.preprocess import create_dataloaders
    from hydragnn_amd.utils.config import update_config
    config = X.model_config(mpnn_type, mlip=False)
    config["NeuralNetwork"]["Architecture"].update(
        {"hidden_dim": 64, "equivariance": True, "num_radial": 8})
    config = update_config(config, *create_dataloaders(
        graphs, graphs, graphs, 4, config=config))
    torch.manual_seed(11)
    model = create_model_config(config["NeuralNetwork"],
                                use_gpu=False).train()
    monkeypatch.setenv("HYDRAGNN_PAINN_FUSED", "0")
    _, ref = X.graph_step(copy.deepcopy(model).double(),
                          X.double_batch(batch_of(graphs, True)))
    dev_model = copy.deepcopy(model).to(DEV)
    out_c, comp = X.graph_step(dev_model, batch_of(graphs, True).to(DEV))
    assert path_counts()["fwd"] == 0
    monkeypatch.setenv("HYDRAGNN_PAINN_FUSED", "1")
    out_f, fused = X.graph_step(dev_model, batch_of(graphs, True).to(DEV))
    assert path_counts() == {"fwd": 2, "bwd_node": 2, "bwd_edge": 2,
                             "composition": 0}
    for a, c in zip(out_f, out_c):
        assert torch.equal(a, c)
    assert set(fused) == set(comp) == set(ref)
    e_fused = max(float((fused[k] - ref[k]).abs().max()) for k in ref)
    e_comp = max(float((comp[k] - ref[k]).abs().max()) for k in ref)
    one_ulp = 2.0 ** -23 * max(float(v.abs().max()) for v in ref.values())
    print(f"{mpnn_type} parameter gradients vs fp64: fused {e_fused:.3e} "
          f"composition {e_comp:.3e} one ulp {one_ulp:.3e}")
    assert e_fused <= 2 * e_comp + one_ulp
