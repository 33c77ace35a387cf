"""gather_mul_sum / gather_mul on the HIP kernels (csrc/gather_mul.hip):
exact where the answer is determined, bit-equal to the fixed-order
composition in fp32/fp64, within one ulp in the half types, closed
under differentiation on the device, reproducible and capturable, and
the SchNet and DimeNet stacks (cases and references:
_exact_gather_mul.py).

Measured on an MI355X (worst over the cases here): bf16 and f16 sums of
non-negative operands, rows of up to 64, 0.500 ulp of the output on
both routes.  SchNet fp32 parameter gradients against the fp64 CPU
model: fused 3.40e-4, composition 3.32e-4 to 3.37e-4 (its gather
backward is atomic), one fp32 ulp of the reference 1.3e-5.  DimeNet fp64
against the fp64 CPU model: outputs 1.8e-16, parameter gradients 1.6e-13
relative.
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
from _exact_agg import (BF, DTYPES, F16, F32, F64, N_SEG, csr_of,  # noqa: E402
                        dtype_id, gen, put, same, ulp, within_one_ulp)
from hydragnn_amd import ops  # noqa: E402
from hydragnn_amd.ops.gather_mul import (SegmentPlan, gather_mul,  # noqa: E402
                                         gather_mul_sum, path_counts,
                                         reset_path_counts)

DEV = torch.device("cuda:0")
CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def _counts():
    reset_path_counts()
    yield


# ---------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.LAYOUTS)
@pytest.mark.parametrize("route", X.ROUTES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_int_grid(dtype, route, name):
    X.check_int(DEV, dtype, route, name)
    counts = path_counts()
    assert counts["sum"] == counts["mul"] == len(X.TRAILING)
    assert counts["composition"] == 0


@pytest.mark.parametrize("route", X.ROUTES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_rows_and_bases_off_16_bytes(dtype, route):
    """F = 6: a row of the half types is 12 bytes.  F = 64 on operands
    whose base is one element past a 16-byte boundary.  Both take the
    element-wise kernels and give the same bits."""
    for name in ("gaps", "long"):
        X.check_int(DEV, dtype, route, name, trailings=((6,),))
        x, w, b, src, dst = X.int_case(name, (64,), route)
        sp, dp = X.plans(src, dst, X.M_SRC, N_SEG, DEV, route)
        xs, ws, bs = (X.off_by_one(t, DEV, dtype) for t in (x, w, b))
        assert same(gather_mul_sum(xs, ws, sp, dp),
                    X.ref_gms(x, w, src, dst, N_SEG), dtype)
        assert same(gather_mul(xs, bs, sp, dp), X.ref_gm(x, b, src, dst),
                    dtype)
        # one side off only
        assert same(gather_mul_sum(put(x, DEV, dtype), ws, sp, dp),
                    X.ref_gms(x, w, src, dst, N_SEG), dtype)
    assert path_counts()["composition"] == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_empty_and_identity(dtype):
    X.check_empty(DEV, dtype)
    assert path_counts()["composition"] == 0


def test_force_eager_runs_the_doubles(monkeypatch):
    monkeypatch.setenv("HYDRAGNN_AMD_FORCE_EAGER", "1")
    X.check_int(DEV, F32, "perm", "gaps", trailings=((5,),))
    assert path_counts() == {"sum": 0, "mul": 0, "composition": 2}


# ---------------------------------------------------------------------------
# equal to the fixed-order composition of the existing ops
# ---------------------------------------------------------------------------
def _normal_case(name, trailing, dtype):
    g = gen("gather_mul_normal", name, trailing)
    x, w, b, src, dst = X.int_case(name, trailing, "perm")
    x = torch.randn(x.shape, generator=g, dtype=F64).to(dtype)
    w = torch.randn(w.shape, generator=g, dtype=F64).to(dtype)
    b = torch.randn(b.shape, generator=g, dtype=F64).to(dtype)
    return x, w, b, src, dst


@pytest.mark.parametrize("name", ("gaps", "long"))
@pytest.mark.parametrize("dtype", (F32, F64), ids=dtype_id)
def test_sum_equals_the_csr_composition(dtype, name):
    for trailing in ((), (5,), (64,), (4, 3)):
        x, w, _, src, dst = _normal_case(name, trailing, dtype)
        sp, dp = X.plans(src, dst, X.M_SRC, N_SEG, DEV, "perm")
        x, w = put(x, DEV), put(w, DEV)
        fused = gather_mul_sum(x, w, sp, dp)
        perm, rowptr = csr_of(dst, N_SEG)
        comp = ops.scatter(ops.gather(x, sp.index) * w, dp.index, N_SEG,
                           "sum", csr=(put(perm, DEV), put(rowptr, DEV)))
        assert torch.equal(fused, comp), f"{dtype} {name} {trailing}"


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_product_equals_the_gather_composition(dtype):
    for trailing in ((), (5,), (64,), (4, 3)):
        x, _, b, src, dst = _normal_case("gaps", trailing, dtype)
        sp, dp = X.plans(src, dst, X.M_SRC, N_SEG, DEV, "perm")
        x, b = put(x, DEV), put(b, DEV)
        comp = ops.gather(x, sp.index) * ops.gather(b, dp.index)
        assert torch.equal(gather_mul(x, b, sp, dp), comp)


# ---------------------------------------------------------------------------
# half precision: one rounding of an fp32 sum
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("trailing", ((6,), (64,)), ids=("F6", "F64"))
@pytest.mark.parametrize("dtype", (BF, F16), ids=dtype_id)
def test_half_within_one_ulp(dtype, trailing):
    x, w, src, dst = X.bounded_case(dtype, trailing)
    assert int(torch.bincount(dst, minlength=N_SEG).max()) == 64
    ref = X.ref_gms(x, w, src, dst, N_SEG)
    for route in X.ROUTES:
        s, d, ww = src, dst, w
        if route == "sorted":
            o = torch.argsort(dst, stable=True)
            s, d, ww = src[o], dst[o], w[o]
        sp, dp = X.plans(s, d, X.M_SRC, N_SEG, DEV, route)
        out = gather_mul_sum(put(x, DEV), put(ww, DEV), sp, dp)
        err = ((out.cpu().to(F64) - ref).abs() / ulp(ref, dtype)).max()
        print(f"half {dtype} {trailing} {route}: worst {float(err):.3f} ulp")
        assert within_one_ulp(out, ref, dtype)
    assert path_counts()["composition"] == 0


# ---------------------------------------------------------------------------
# closure under differentiation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", X.ROUTES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_closure_equals_the_doubles(dtype, route):
    """First-order gradients and the force-style second order through
    the Function pairs: the device gives the bits of the CPU doubles,
    launches what the closure table predicts and runs no composition."""
    x, w, src, dst = X.closure_case()
    if route == "sorted":
        o = torch.argsort(dst, stable=True)
        src, dst, w = src[o], dst[o], w[o]
    want = X.closure_chain(x.to(dtype), w.to(dtype),
                           *X.plans(src, dst, X.CLOSURE_M, N_SEG, CPU, route))
    assert max(float(t.abs().max()) for t in want) < 2 ** 15
    reset_path_counts()
    got = X.closure_chain(put(x, DEV, dtype), put(w, DEV, dtype),
                          *X.plans(src, dst, X.CLOSURE_M, N_SEG, DEV, route))
    counts = path_counts()
    assert counts["composition"] == 0
    assert counts["sum"] == X.CLOSURE_LAUNCHES["sum"]
    assert counts["mul"] == X.CLOSURE_LAUNCHES["mul"]
    for name, a, b in zip(("out", "dx", "dw", "hx", "hw"), got, want):
        assert a.dtype == dtype and torch.equal(a.cpu(), b), \
            f"{name} {dtype} {route}"


# ---------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------
def _step_case(dtype, name="long", trailing=(64,)):
    x, w, b, src, dst = _normal_case(name, trailing, dtype)
    return x, w, b, src, dst


def _second_order_step(x, w, b, sp, dp):
    """Forward and double backward of both ops on leaves x, w, b."""
    out = gather_mul_sum(x, w, sp, dp)
    prod = gather_mul(x, b, sp, dp)
    energy = 0.5 * (out * out).sum() + 0.5 * (prod * prod).sum()
    dx, dw = torch.autograd.grad(energy, (x, w), create_graph=True)
    r = 0.5 * ((dx * dx).sum() + (dw * dw).sum())
    hx, hw, hb = torch.autograd.grad(r, (x, w, b))
    return [t.detach() for t in (out, prod, dx, dw, hx, hw, hb)]


@pytest.mark.parametrize("dtype", (F32, BF), ids=dtype_id)
def test_sorted_route_perm_route_and_reruns_give_the_same_bits(dtype):
    x, w, b, src, dst = _step_case(dtype)
    leaves = [put(t, DEV).requires_grad_(True) for t in (x, w, b)]
    sp, dp = X.plans(src, dst, X.M_SRC, N_SEG, DEV, "perm")
    first = _second_order_step(*leaves, sp, dp)
    again = _second_order_step(*leaves, sp, dp)
    for a, c in zip(first, again):
        assert torch.equal(a, c)
    o = torch.argsort(dst, stable=True)
    inv = torch.empty_like(o)
    inv[o] = torch.arange(o.numel())
    ws = put(w[o], DEV).requires_grad_(True)
    sps, dps = X.plans(src[o], dst[o], X.M_SRC, N_SEG, DEV, "sorted")
    srt = _second_order_step(leaves[0], ws, leaves[2], sps, dps)
    inv = put(inv, DEV)
    # out, and the edge-wise prod and dw, which come back in the sorted
    # edge order.  (Sums over the rows of src run in ascending edge id,
    # and reordering the edges renumbers them: dx and the second order
    # are the same sums in another order.)
    for k in (0, 1, 3):
        a, c = first[k], srt[k]
        if k in (1, 3):
            c = c.index_select(0, inv)
        assert torch.equal(a, c), k
    assert path_counts()["composition"] == 0


def test_capture_second_order_replays_bit_for_bit():
    """Forward plus double backward of both ops on static tensors with
    prebuilt plans captured into a device graph: nothing in the path may
    sync, and the replay equals eager bit for bit.  Stream handling as
    in test_gpu_pna_aggr.py."""
    x, w, b, src, dst = _step_case(F32, "gaps", (5,))
    leaves = [put(t, DEV).requires_grad_(True) for t in (x, w, b)]
    sp, dp = X.plans(src, dst, X.M_SRC, N_SEG, DEV, "perm")
    sp.csr()
    dp.csr()

    def step():
        return _second_order_step(*leaves, sp, dp)

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
    assert path_counts()["composition"] == 0
    for a, c in zip(static, eager):
        assert torch.equal(a, c)


# ---------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------
def _lj(num_samples=4):
    from hydragnn_amd.utils.datasets.synthetic import lj_dataset
    return lj_dataset(num_samples=num_samples, num_atoms=27, pbc=False)


def _batch(dataset, sort=False):
    from hydragnn_amd.data import Batch
    batch = Batch.from_data_list([d.clone() for d in dataset])
    if sort:
        batch.sort_edges_by_dst()
        batch["edges_sorted_"] = True
    return batch


def test_schnet_fp32_forward_equals_the_composition(monkeypatch):
    """dst-sorted edges: the composition's sum is the CSR kernel, whose
    order and roundings the fused kernel reproduces."""
    dataset = _lj()
    model = X.build_model("SchNet", dataset).to(DEV).eval()
    monkeypatch.setenv("HYDRAGNN_GATHER_MUL", "1")
    with torch.no_grad():
        fused = model(_batch(dataset, sort=True).to(DEV))
        counts = path_counts()
        assert counts["sum"] == 2 and counts["composition"] == 0
        monkeypatch.setenv("HYDRAGNN_GATHER_MUL", "0")
        comp = model(_batch(dataset, sort=True).to(DEV))
    assert path_counts() == counts
    for a, c in zip(fused, comp):
        assert torch.equal(a, c)


def test_schnet_energy_force_step(monkeypatch):
    """Energy + forces with create_graph=True against the fp64 CPU
    model: the fused route's worst parameter-gradient error is at most
    twice the composition's plus one fp32 ulp of the reference, and the
    step runs no composition."""
    dataset = _lj()
    model = X.build_model("SchNet", dataset).train()
    _, ref = X.energy_force_step(copy.deepcopy(model).double(),
                                 X.double_batch(_batch(dataset)))
    dev_model = copy.deepcopy(model).to(DEV)
    monkeypatch.setenv("HYDRAGNN_GATHER_MUL", "1")
    reset_path_counts()
    _, fused = X.energy_force_step(dev_model, _batch(dataset).to(DEV))
    counts = path_counts()
    assert counts["sum"] >= 6 and counts["mul"] >= 2
    assert counts["composition"] == 0, counts
    monkeypatch.setenv("HYDRAGNN_GATHER_MUL", "0")
    _, comp = X.energy_force_step(dev_model, _batch(dataset).to(DEV))
    assert path_counts() == counts
    assert set(fused) == set(ref) == set(comp)

    def worst(grads):
        return max(float((grads[k] - ref[k]).abs().max()) for k in ref)

    one_ulp = 2.0 ** -23 * max(float(v.abs().max()) for v in ref.values())
    e_fused, e_comp = worst(fused), worst(comp)
    print(f"SchNet parameter gradients vs fp64: fused {e_fused:.3e} "
          f"composition {e_comp:.3e} one ulp {one_ulp:.3e}")
    assert e_fused <= 2 * e_comp + one_ulp


@pytest.fixture(scope="module")
def dimenet_case():
    """Three periodic cells of 27 atoms at radius 3: about 15 neighbours
    per atom and 14 triplets per edge.  The fp64 CPU reference runs the
    composition and is computed once."""
    from hydragnn_amd.utils.datasets.synthetic import lj_dataset
    dataset = lj_dataset(num_samples=3, num_atoms=27, cell_size=6.1,
                         radius=3.0, pbc=True, seed=31, dtype=F64)
    model = X.build_model("DimeNet", dataset, mlip=False,
                          radius=3.0).double().train()
    os.environ["HYDRAGNN_GATHER_MUL"] = "0"
    try:
        ref = X.graph_step(copy.deepcopy(model), _batch(dataset))
    finally:
        os.environ.pop("HYDRAGNN_GATHER_MUL")
    return dataset, model, ref


def test_dimenet_fp64_matches_the_cpu_model_and_reruns(dimenet_case):
    dataset, model, (ref_out, ref_grads) = dimenet_case
    dev_model = copy.deepcopy(model).to(DEV)
    n_edges = sum(d.edge_index.shape[1] for d in dataset)
    reset_path_counts()
    out, grads = X.graph_step(dev_model, _batch(dataset).to(DEV))
    counts = path_counts()
    # per block the triplet sum and the edge -> node sum: 4 forward
    # sums.  The second block reads the messages, not the node features
    # the first block's output sum made, so that one has no backward:
    # 3 dx sums and 3 dw products.
    assert counts == {"sum": 7, "mul": 3, "composition": 0}, counts
    assert n_edges > 1000
    e_out, e_grad = X.rel_err(out, ref_out), X.rel_err(grads, ref_grads)
    print(f"DimeNet fp64 vs the CPU model: outputs {e_out:.3e} "
          f"gradients {e_grad:.3e}")
    assert set(grads) == set(ref_grads)
    assert e_out <= 1e-12 and e_grad <= 1e-12
    out2, grads2 = X.graph_step(dev_model, _batch(dataset).to(DEV))
    for a, c in zip(out, out2):
        assert torch.equal(a, c)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k
