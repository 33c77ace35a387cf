"""edge_pair_affine on the HIP kernels (csrc/edge_affine.hip): exact on
integer data, bit-equal to the doubles, reruns, routes and graph replays,
a force-style chain on the kernels alone, within twice today's composition
on general data, and the EGNN stack (cases: test_edge_affine.py).

Measured on an MI355X, the first edge layer against today's
linear(cat(gather, gather, r2, ea)), worst over H, D and the routes,
absolute error against fp64 autograd, fused / composition: fp32 z 1.2e-6
/ 2.1e-6, dh 7.9e-6 / 6.6e-6, dr2 2.1e-7 / 8.9e-7, dea 2.5e-7 / 1.3e-6,
dW 2.3e-5 / 3.6e-5, db 5.9e-6 / 5.3e-6; bf16 z 0.023 / 0.016, dh 0.073 /
0.33, dr2 7.2e-3 both, dea 7.5e-3 both, dW 0.41 / 0.25, db 0.12 both;
f16 z 2.8e-3 / 2.0e-3, dh 8.7e-3 / 0.040, dW 0.040 / 0.031, db 0.013
both.  EGNN stack, fp32 parameter gradients against the fp64 CPU model:
fused 7.39e-8, composition 5.29e-8.
"""

import copy
import os
import sys

import pytest
import torch
from torch.nn import functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact_gather_mul as X  # noqa: E402
import test_edge_affine as C  # noqa: E402
from _exact_agg import (BF, DTYPES, F16, F32, F64, dtype_id, gen, put,  # noqa: E402
                        ref_ordered_sum, same)
from hydragnn_amd.ops import act_linear  # noqa: E402
from hydragnn_amd.ops.edge_affine import (  # noqa: E402
    edge_pair_affine, path_counts, reset_path_counts, torch_edge_pair_affine)

DEV = torch.device("cuda:0")
ROUTES = ("sorted", "perm")
# element-wise with idle lanes; packed; more than 64 element-wise packs;
# more than 64 fp32 packs
FEATS = (6, 64, 70, 264)
EDGE_DIMS = (0, 3)


@pytest.fixture(autouse=True)
def _counts():
    reset_path_counts()
    yield


@pytest.mark.parametrize("edge_dim", EDGE_DIMS)
@pytest.mark.parametrize("feat", FEATS)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_exact(dtype, route, feat, edge_dim):
    C.check_int(DEV, dtype, route, feat, edge_dim)
    assert path_counts() == {"fwd": 1, "node": 1, "edge": 1, "param": 1,
                             "composition": 0}


@pytest.mark.parametrize("absent", ("P", "ea W_e", "b", "r2 w_r"))
@pytest.mark.parametrize("feat", (6, 64))
@pytest.mark.parametrize("dtype", (F32, BF), ids=dtype_id)
def test_absent_groups(dtype, feat, absent):
    x, src, dst, _ = C.int_case(feat, 3, "perm")
    x = {k: None if k in absent.split() else t for k, t in x.items()}
    want = C.ref_fwd(*x.values(), src, dst, feat)
    assert C.representable(want, dtype)
    z = edge_pair_affine(*C.cast(x, DEV, dtype).values(),
                         *C.plans(src, dst, DEV, "perm"))
    assert same(z, want, dtype) and path_counts()["composition"] == 0


def normal_case(feat, edge_dim, route, dtype):
    """Unit-normal operands and cotangent rounded to `dtype`, as fp64."""
    x, src, dst, g = C.int_case(feat, edge_dim, route)
    k = gen("edge_affine_normal", feat, edge_dim, route)
    draw = {n: None if t is None else
            torch.randn(t.shape, generator=k, dtype=F64).to(dtype).to(F64)
            for n, t in dict(x, g=g).items()}
    return draw, src, dst, draw.pop("g")


def step(x, g, sp, dp):
    for t in x.values():
        if t is not None:
            t.grad = None
    z = edge_pair_affine(*x.values(), sp, dp)
    z.backward(g)
    return [z.detach()] + [t.grad for t in x.values() if t is not None]


def leaves(x, dtype):
    return {k: None if t is None else t.requires_grad_(True)
            for k, t in C.cast(x, DEV, dtype).items()}


@pytest.mark.parametrize("edge_dim", EDGE_DIMS)
@pytest.mark.parametrize("feat", FEATS)
@pytest.mark.parametrize("dtype", (F32, F64), ids=dtype_id)
def test_random_data_bit_for_bit(dtype, feat, edge_dim):
    """Products are rounded and the order is fixed: fwd equals its
    double on the device, node the ordered sum; a rerun, the dst-sorted
    edge list and three graph replays change no bit."""
    x, src, dst, g = normal_case(feat, edge_dim, "perm", dtype)
    sp, dp = C.plans(src, dst, DEV, "perm")
    d, gd = leaves(x, dtype), put(g, DEV, dtype)
    first = [t.clone() for t in step(d, gd, sp, dp)]
    with torch.no_grad():
        assert torch.equal(first[0], torch_edge_pair_affine(
            *d.values(), sp, dp, src.numel()))
    gt = g.to(dtype)
    want = torch.cat([ref_ordered_sum(gt, dst, C.N),
                      ref_ordered_sum(gt, src, C.N)], 1)
    assert torch.equal(first[1].cpu(), want)
    for a, c in zip(first, step(d, gd, sp, dp)):
        assert torch.equal(a, c)
    o = torch.argsort(dst, stable=True)
    xs = leaves(dict(x, r2=x["r2"][o],
                     ea=None if x["ea"] is None else x["ea"][o]), dtype)
    srt = step(xs, gd[put(o, DEV)], *C.plans(src[o], dst[o], DEV, "sorted"))
    # the dst half of dP keeps its order of summation; the src half adds
    # the same terms in the renumbered order
    assert torch.equal(first[0][put(o, DEV)], srt[0])
    assert torch.equal(first[1][:, :feat], srt[1][:, :feat])
    assert torch.equal(first[2][put(o, DEV)], srt[2])
    # forward + backward captured into a device graph, plans warm
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(d, gd, sp, dp)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static = step(d, gd, sp, dp)
    for _ in range(3):
        for t in static:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, c in zip(static, first):
            assert torch.equal(a, c)
    assert path_counts()["composition"] == 0


@pytest.mark.parametrize("feat", (6, 64))
@pytest.mark.parametrize("dtype", (F64, BF), ids=dtype_id)
def test_force_chain_stays_on_the_kernels(dtype, feat):
    """Launches by the closure table: the forward is one fwd; its
    backward one node, edge and param; the second order differentiates
    node (one fwd) and edge (one fwd, one param) and passes through the
    forward's backward once more (node, edge, param).  fp64 agrees with
    the CPU doubles."""
    x, src, dst, _ = normal_case(feat, 3, "perm", dtype)

    def chain(d, sp, dp):
        z = edge_pair_affine(*d.values(), sp, dp)
        gr, gp = torch.autograd.grad((z * z).sum(), (d["r2"], d["P"]),
                                     create_graph=True)
        ((gr * gr).sum() + (gp * gp).sum()).backward()
        return [t.grad for t in d.values()]

    got = chain(leaves(x, dtype), *C.plans(src, dst, DEV, "perm"))
    assert path_counts() == {"fwd": 3, "node": 2, "edge": 2, "param": 3,
                             "composition": 0}
    if dtype == F64:
        cpu = {k: t.clone().requires_grad_(True) for k, t in x.items()}
        for a, b in zip(got, chain(cpu, *C.plans(src, dst, "cpu", "perm"))):
            assert float((a.cpu() - b).abs().max()) <= \
                1e-12 * float(b.abs().max())


def layer(h, r2, ea, W, b, src, dst, fused, sp=None, dp=None):
    """The first edge layer: today's linear(cat(gather, gather, r2, ea))
    or the node-side GEMM and the op."""
    feat = h.shape[1]
    if not fused:
        parts = [h[dst], h[src], r2[:, None]] + ([] if ea is None else [ea])
        return F.linear(torch.cat(parts, 1), W, b)
    P = F.linear(h, torch.cat([W[:, :feat], W[:, feat:2 * feat]], 0))
    return edge_pair_affine(P, r2, ea, W[:, 2 * feat],
                            None if ea is None else W[:, 2 * feat + 1:], b,
                            sp, dp)


@pytest.mark.parametrize("edge_dim", EDGE_DIMS)
@pytest.mark.parametrize("feat", FEATS)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", (F32, BF, F16), ids=dtype_id)
def test_general_data(dtype, route, feat, edge_dim):
    """Output and gradients are no further from fp64 autograd than twice
    the composition on the same data and device plus one ulp of the type
    at the value's largest magnitude (P is rounded twice more in bf16)."""
    x, src, dst, g = normal_case(feat, edge_dim, route, dtype)
    k = gen("edge_affine_layer", feat, edge_dim)
    h = torch.randn(C.N, feat, generator=k, dtype=F64).to(dtype).to(F64)
    W = (torch.randn(feat, 2 * feat + 1 + edge_dim, generator=k, dtype=F64)
         / (2 * feat) ** 0.5).to(dtype).to(F64)
    ops64 = [h, x["r2"], x["ea"], W, x["b"]]
    sp, dp = C.plans(src, dst, DEV, route)

    def run(dev, dt, fused):
        a = [None if t is None else put(t, dev, dt).clone().requires_grad_(True)
             for t in ops64]
        z = layer(*a, put(src, dev), put(dst, dev), fused, sp, dp)
        z.backward(put(g, dev, dt))
        return [z.detach()] + [t.grad for t in a if t is not None]

    want = run("cpu", F64, False)
    fused, comp = run(DEV, dtype, True), run(DEV, dtype, False)
    assert path_counts()["composition"] == 0
    names = [n for n, t in zip(("z", "dh", "dr2", "dea", "dW", "db"),
                               [h] + ops64) if t is not None]
    for name, a, c, b in zip(names, fused, comp, want):
        e_fused = float((a.double().cpu() - b).abs().max())
        e_comp = float((c.double().cpu() - b).abs().max())
        one_ulp = torch.finfo(dtype).eps * float(b.abs().max())
        print(f"{name} {dtype} H={feat} D={edge_dim} {route}: fused "
              f"{e_fused:.3e} composition {e_comp:.3e} ulp {one_ulp:.3e}")
        assert e_fused <= 2 * e_comp + one_ulp, name


@pytest.fixture(scope="module")
def graphs():
    from hydragnn_amd.utils.datasets.synthetic import lj_dataset
    return lj_dataset(num_samples=3, num_atoms=27, pbc=False)


def egnn(graphs):
    from hydragnn_amd.models import create_model_config
    from hydragnn_amd.preprocess import create_dataloaders
    from hydragnn_amd.utils.config import update_config
    config = X.model_config("EGNN", mlip=False)
    config["NeuralNetwork"]["Architecture"].update(
        {"hidden_dim": 64, "equivariance": True})
    config = update_config(config, *create_dataloaders(
        graphs, graphs, graphs, 4, config=config))
    torch.manual_seed(11)
    return create_model_config(config["NeuralNetwork"], use_gpu=False).train()


def batch_of(dataset):
    from hydragnn_amd.data import Batch
    return Batch.from_data_list([d.clone() for d in dataset])


def test_stack_fp32(graphs, monkeypatch):
    """hidden 64, 2 layers, 3 graphs: parameter gradients against the
    fp64 CPU model within twice the composition's distance plus one fp32
    ulp; a captured replay of the forward equals the eager one."""
    model = egnn(graphs)
    monkeypatch.setenv("HYDRAGNN_EGNN_FUSED", "0")
    _, ref = X.graph_step(copy.deepcopy(model).double(),
                          X.double_batch(batch_of(graphs)))
    dev_model = copy.deepcopy(model).to(DEV)
    _, comp = X.graph_step(dev_model, batch_of(graphs).to(DEV))
    assert path_counts()["fwd"] == 0
    monkeypatch.setenv("HYDRAGNN_EGNN_FUSED", "1")
    batch = batch_of(graphs).to(DEV)
    out_f, fused = X.graph_step(dev_model, batch)
    # r2 carries a gradient only where an earlier layer moved pos
    assert path_counts() == {"fwd": 2, "node": 2, "edge": 1, "param": 2,
                             "composition": 0}
    assert set(fused) == set(comp) == set(ref)
    e_fused = max(float((fused[k] - ref[k]).abs().max()) for k in ref)
    e_comp = max(float((comp[k] - ref[k]).abs().max()) for k in ref)
    one_ulp = 2.0 ** -23 * max(float(v.abs().max()) for v in ref.values())
    print(f"EGNN parameter gradients vs fp64: fused {e_fused:.3e} "
          f"composition {e_comp:.3e} one ulp {one_ulp:.3e}")
    assert e_fused <= 2 * e_comp + one_ulp
    dev_model.eval()
    with torch.no_grad():
        eager = [t.clone() for t in dev_model(batch)]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            static = dev_model(batch)
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, c) for a, c in zip(static, eager))


def test_stack_bf16_second_layer_on_the_fused_gemms(graphs, monkeypatch):
    """Under bf16 autocast, E >= 256 puts the second edge layer inside
    act_linear's envelope: one fused SiLU GEMM per layer, and no double
    anywhere."""
    monkeypatch.setenv("HYDRAGNN_EGNN_FUSED", "1")
    model = egnn(graphs).to(DEV)
    batch = batch_of(graphs).to(DEV)
    assert batch.edge_index.shape[1] >= 256
    act_linear.reset_path_counts()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        X.graph_step(model, batch)
    counts = act_linear.path_counts()
    assert counts["act_linear"] == 2 and counts["composition"] == 0, counts
    assert path_counts()["fwd"] == 2 and path_counts()["composition"] == 0
