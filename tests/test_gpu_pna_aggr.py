"""Fused PNA aggregation on the HIP kernels (csrc/pna_aggr.hip): exact
where the answer is determined, derived bounds elsewhere, the CPU
doubles as the yardstick for the gradients (cases, references and
bounds: _exact_pna.py), and the PNAEq model level.

Measured on an MI355X (worst over the cases here), in units of the
accumulator eps: var of general data 3.1 (fp32) and 1.6 (fp64), std 1.9
and 1.0, against derived bounds of up to 34 and 20.  bf16 std on the
shifted data: worst absolute error 9.8e-4, every output within one
bf16 ulp.
"""

import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact_pna as X  # noqa: E402
from _exact_agg import (BF, DTYPES, F32, F64, N_SEG, dtype_id,  # noqa: E402
                        put, within_one_ulp)
from hydragnn_amd import ops  # noqa: E402
from hydragnn_amd.ops import get_extension  # noqa: E402

DEV = torch.device("cuda:0")
CPU = torch.device("cpu")
ROUTES = ("sorted", "perm")
ALL_AGGS = ("sum", "mean", "min", "max", "std", "var")


@pytest.fixture(autouse=True)
def _counts():
    ops.reset_path_counts()
    yield


@pytest.mark.parametrize("name", X.LAYOUTS)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_int_blocks(dtype, route, name):
    X.check_int_blocks(ops, DEV, dtype, route, name)
    counts = ops.path_counts()
    assert counts["fwd"] == len(X.TRAILING) and counts["composition"] == 0


@pytest.mark.parametrize("aggs", [("std",), ("max", "sum"),
                                  ("var", "min", "mean", "sum", "max",
                                   "std")])
def test_subsets_equal_the_full_set(aggs):
    """Any subset, in any order, holds the blocks of the full set bit
    for bit."""
    src, index = X.int_case("gaps", (3,))
    x = put(src, DEV, F32)
    idx = put(index, DEV)
    full, _ = X.run(ops, "perm", x, idx, N_SEG, ALL_AGGS,
                    X.DEFAULT_SCALERS, DEV)
    part, _ = X.run(ops, "perm", x, idx, N_SEG, aggs, X.DEFAULT_SCALERS,
                    DEV)
    full = X.split_blocks(full, 4, 6)
    part = X.split_blocks(part, 4, len(aggs))
    for a, agg in enumerate(aggs):
        assert torch.equal(part[:, :, a], full[:, :, ALL_AGGS.index(agg)])


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_extremes_and_routing(dtype, route):
    for name, trailing in (("gaps", (3,)), ("long", (1,)),
                           ("single", (4, 3)), ("one_row", (64,))):
        X.check_extremes(ops, DEV, dtype, route, name, trailing)
    counts = ops.path_counts()
    assert counts["bwd"] == 8 and counts["bwd2"] == 8
    assert counts["composition"] == 0


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_pairs_var_exact_std_bounded(dtype, route):
    X.check_pairs(ops, DEV, dtype, route)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_general_var_std_within_derived_bound(dtype, route):
    worst_v, worst_s = X.check_general(ops, DEV, dtype, route)
    print(f"general {dtype} {route}: var {worst_v:.2f} eps, "
          f"std {worst_s:.2f} eps")


def _module(aggs=X.DEFAULT_AGGS, scalers=("identity",)):
    from hydragnn_amd.models.layers import DegreeScalerAggregation
    return DegreeScalerAggregation(list(aggs), list(scalers),
                                   torch.tensor([0, 3, 5, 2])).to(DEV)


def test_bf16_shifted_std_within_one_ulp_through_module():
    """Values 16 + k/8, rows of 0 .. 64 entries: every std output of
    DegreeScalerAggregation on the device is within one bf16 ulp of the
    fp64 truth."""
    src, index, n = X.shifted_case()
    out = _module()(put(src, DEV, BF), put(index, DEV), n)
    std = X.split_blocks(out.cpu(), 1, 4)[:, 0, 3]
    ref = X.ref_block("std", src, index, n)
    err = (std.to(F64) - ref).abs().max()
    print(f"bf16 shifted std: worst abs error {err:.3e}")
    assert within_one_ulp(std, ref, BF)
    assert ops.path_counts()["composition"] == 0


def test_module_flag_restores_the_composition(monkeypatch):
    src, index = X.int_case("gaps", (3,))
    mod = _module(scalers=X.DEFAULT_SCALERS)
    fused = mod(put(src, DEV, F32), put(index, DEV), N_SEG)
    assert ops.path_counts()["fwd"] == 1
    monkeypatch.setenv("HYDRAGNN_PNA_FUSED", "0")
    comp = mod(put(src, DEV, F32), put(index, DEV), N_SEG)
    counts = ops.path_counts()
    assert counts["fwd"] == 1 and counts["composition"] == 1
    # same layout: the blocks line up (std differs in the last bits)
    assert fused.shape == comp.shape
    assert torch.allclose(fused, comp, rtol=1e-3, atol=1e-3)
    # sorted edges take the rowptr route and give the same bits
    o = torch.argsort(index, stable=True)
    monkeypatch.delenv("HYDRAGNN_PNA_FUSED")
    mod._edges_sorted = True
    again = mod(put(src[o], DEV, F32), put(index[o], DEV), N_SEG)
    assert torch.equal(again, fused)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_empty(dtype):
    X.check_empty(ops, DEV, dtype)
    counts = ops.path_counts()
    assert counts["fwd"] == 0 and counts["bwd"] == 0     # no launch


def _all_orders(dtype, route, name="long"):
    got, _ = X.grads_of(ops, DEV, dtype, route, ALL_AGGS, X.ALL_SCALERS,
                        name)
    return got


@pytest.mark.parametrize("dtype", [F32, BF], ids=dtype_id)
def test_routes_agree_and_runs_repeat(dtype):
    """Sorted and perm routes on the same data, and two runs of one
    route: identical bits in all three orders."""
    x64, index, _, _ = X.grad_case(dtype, "long")
    o = torch.argsort(index, stable=True)
    s = _all_orders(dtype, "sorted")
    p = _all_orders(dtype, "perm")
    p2 = _all_orders(dtype, "perm")
    for a, b in zip(p, p2):
        assert torch.equal(a, b)
    assert torch.equal(s[0], p[0]) and torch.equal(s[3], p[3])
    assert torch.equal(s[1], p[1][o]) and torch.equal(s[2], p[2][o])
    assert ops.path_counts()["composition"] == 0


@pytest.mark.parametrize("name", ["gaps", "long"])
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", [F32, BF], ids=dtype_id)
def test_first_and_second_order_against_cpu_double(dtype, route, name):
    """Max-abs error of (out, dx, gx, hG) against fp64 autograd of the
    plain-torch reference: at most twice that of the op's CPU double in
    the same dtype, plus one ulp of the output type at the largest
    reference value (association differences only)."""
    got, ref = X.grads_of(ops, DEV, dtype, route, ALL_AGGS, X.ALL_SCALERS,
                          name)
    cpu, ref_cpu = X.grads_of(ops, CPU, dtype, route, ALL_AGGS,
                              X.ALL_SCALERS, name)
    e_dev = X.max_errors(got, ref)
    e_cpu = X.max_errors(cpu, ref_cpu)
    for what, d, c, r in zip(("out", "dx", "gx", "hG"), e_dev, e_cpu, ref):
        ulp = X.ulp_at(r.abs().max(), dtype)
        print(f"{what} {dtype} {route} {name}: device {d:.3e} "
              f"cpu double {c:.3e} ulp {ulp:.3e}")
        assert d <= 2 * c + ulp, what
    counts = ops.path_counts()
    assert counts["fwd"] == 1 and counts["bwd"] == 1 and counts["bwd2"] == 1


@pytest.mark.parametrize("route", ROUTES)
def test_fp64_agrees_with_cpu_double(route):
    got, _ = X.grads_of(ops, DEV, F64, route, ALL_AGGS, X.ALL_SCALERS,
                        "long")
    cpu, _ = X.grads_of(ops, CPU, F64, route, ALL_AGGS, X.ALL_SCALERS,
                        "long")
    for what, a, b in zip(("out", "dx", "gx", "hG"), got, cpu):
        rel = float((a - b).abs().max() / b.abs().max())
        print(f"fp64 {what} {route}: {rel:.3e}")
        assert rel <= 1e-12, what


def test_just_above_the_grid_cap():
    """More (row, feature) pairs than the capped grid has threads: the
    grid-stride loop serves the rest.  One aggregator, one scaler, one
    entry per row: the output is the source, the gradient the
    cotangent."""
    ext = get_extension(required=True)
    n, feat = 8193 * 4, 64
    assert n * feat > 8192 * 256 and ext.pna_grid_blocks(n * feat) == 8192
    g = X.gen("pna_cap")
    x = torch.randint(-8, 9, (n, feat), generator=g).to(F32).to(DEV)
    x.requires_grad_(True)
    rowptr = torch.arange(n + 1, device=DEV)
    scale = ops.pna_scale(rowptr, ("identity",), 1.0, 1.0, F32)
    out = ops.pna_aggregate(x, rowptr, scale, ("sum",))
    assert torch.equal(out, x.detach())
    w = torch.randint(1, 9, (n, feat), generator=g).to(F32).to(DEV)
    (dx,) = torch.autograd.grad(out, x, w)
    assert torch.equal(dx, w)


def test_third_order_falls_back_to_the_composition():
    x64, index, c64, g = X.grad_case(F32, "gaps")
    x = put(x64, DEV, F32).requires_grad_(True)
    out, _ = X.run(ops, "perm", x, put(index, DEV), N_SEG, X.DEFAULT_AGGS,
                   X.DEFAULT_SCALERS, DEV)
    w = torch.ones_like(out).requires_grad_(True)
    (dx,) = torch.autograd.grad(out, x, w, create_graph=True)
    c = put(c64, DEV, F32)
    (k,) = torch.autograd.grad(dx, x, c, retain_graph=True)
    (f,) = torch.autograd.grad(dx, x, c, create_graph=True)
    assert ops.path_counts()["composition"] == 1 and f.requires_grad
    assert torch.allclose(k, f, rtol=1e-4, atol=1e-5)


def test_capture_forward_and_backward_replays_bit_for_bit():
    """Forward plus first-order backward on static tensors captured
    into a device graph: nothing in the path may sync (a sync fails the
    capture), and the replay equals eager bit for bit.

    As in train/captured.py, eager run and capture share one side
    stream and no autograd graph of the eager run is alive at capture:
    a surviving graph keeps the leaf's AccumulateGrad node with the
    stream it was built on, and the capture-time backward would then
    order that stream against the capturing one."""
    x64, index, _, g = X.grad_case(F32, "long")
    index = put(index, DEV)
    x = put(x64, DEV, F32).requires_grad_(True)
    mod = _module(scalers=X.DEFAULT_SCALERS)
    w = torch.randn(N_SEG, 4 * 4 * 3, generator=g).to(DEV)

    def step():
        out = mod(x, index, N_SEG)
        (dx,) = torch.autograd.grad(out, x, w)
        return out.detach(), dx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in step()]      # the warm-up as well
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static = step()
    for t in static:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert ops.path_counts()["composition"] == 0
    for a, b in zip(static, eager):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# model level: PNAEq energy + forces
# ---------------------------------------------------------------------------
def _pnaeq(dataset):
    from deterministic_graph_data import base_config
    from hydragnn_amd.models import create_model_config
    from hydragnn_amd.preprocess import create_dataloaders
    from hydragnn_amd.utils.config import update_config
    config = base_config("PNAEq", heads=("node",), num_epoch=1,
                         hidden_dim=32, lr=0.005, batch_size=4)
    arch = config["NeuralNetwork"]["Architecture"]
    arch.update({"enable_interatomic_potential": True,
                 "energy_weight": 1.0, "energy_peratom_weight": 0.0,
                 "force_weight": 10.0, "radius": 2.5,
                 "equivariance": True, "num_radial": 8,
                 "num_conv_layers": 2})
    config["NeuralNetwork"]["Variables_of_interest"]["output_dim"] = [1]
    loaders = create_dataloaders(dataset, dataset, dataset, 4,
                                 config=config)
    config = update_config(config, *loaders)
    torch.manual_seed(11)
    return create_model_config(config["NeuralNetwork"], use_gpu=False)


def _param_grads(model, batch):
    model.zero_grad(set_to_none=True)
    batch.pos.requires_grad_(True)
    pred = model(batch)
    loss, _ = model.energy_force_loss(pred, batch, create_graph=True)
    loss.backward()
    return {k: p.grad.detach().double().cpu()
            for k, p in model.named_parameters() if p.grad is not None}


def _double(batch):
    for k, v in batch._store.items():
        if torch.is_tensor(v) and v.is_floating_point():
            batch._store[k] = v.double()
    return batch


def _worst(grads, ref):
    return max(float((grads[k] - ref[k]).abs().max()) for k in ref)


def test_pnaeq_energy_force_step(monkeypatch):
    """2-layer PNAEq, energy + forces with create_graph=True: all three
    kernels run and no composition; the parameter gradients are no
    further from the fp64 CPU model than twice the composition's."""
    import copy
    from hydragnn_amd.data import Batch
    from hydragnn_amd.utils.datasets.synthetic import lj_dataset
    dataset = lj_dataset(num_samples=4, num_atoms=27, pbc=False)
    model = _pnaeq(dataset).train()
    ref = _param_grads(copy.deepcopy(model).double(), _double(
        Batch.from_data_list([d.clone() for d in dataset])))
    dev_model = copy.deepcopy(model).to(DEV)

    def batch():
        return Batch.from_data_list([d.clone() for d in dataset]).to(DEV)

    ops.reset_path_counts()
    fused = _param_grads(dev_model, batch())
    counts = ops.path_counts()
    assert counts["fwd"] >= 2 and counts["bwd"] >= 2 and counts["bwd2"] >= 2
    assert counts["composition"] == 0, counts
    monkeypatch.setenv("HYDRAGNN_PNA_FUSED", "0")
    comp = _param_grads(dev_model, batch())
    assert ops.path_counts()["fwd"] == counts["fwd"]
    assert set(fused) == set(ref) == set(comp)
    e_fused, e_comp = _worst(fused, ref), _worst(comp, ref)
    print(f"PNAEq parameter gradients vs fp64: fused {e_fused:.3e} "
          f"composition {e_comp:.3e}")
    assert e_fused <= 2 * e_comp
