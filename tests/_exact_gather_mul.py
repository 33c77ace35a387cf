"""Shared pieces of the gather-multiply-sum tests (test_gather_mul.py on
the CPU doubles, test_gpu_gather_mul.py on the HIP kernels): cases,
fp64 references that do not go through the ops, and the checks, which
take the device as an argument.

Exact-integer method of _exact_agg.py: operands are seeded integers in
[-8, 8], a row holds at most 2100 entries, so every partial sum is an
integer of at most 2100 * 64 < 2^24 and the fp32 accumulation is exact.
The fp64 reference rounded once then fixes every output bit.
"""

import torch

from _exact_agg import (F64, N_SEG, TRAILING, gen, ints, layout, put,
                        same)
from hydragnn_amd.ops.gather_mul import (SegmentPlan, gather_mul,
                                         gather_mul_sum, path_counts,
                                         reset_path_counts)

__all__ = ["SegmentPlan", "gather_mul", "gather_mul_sum", "path_counts",
           "reset_path_counts"]

LAYOUTS = ("gaps", "one_row", "single", "long")
ROUTES = ("sorted", "perm")
M_SRC = 37           # rows of the gathered operand


# ---------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------
def ref_gms(x, w, src, dst, n):
    prod = x.to(F64)[src] * w.to(F64)
    return torch.zeros((n,) + prod.shape[1:], dtype=F64).index_add_(
        0, dst, prod)


def ref_gm(a, b, src, dst):
    return a.to(F64)[src] * b.to(F64)[dst]


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
def int_case(name, trailing, route, lo=-8, hi=8):
    """x [M_SRC, ...], w [E, ...], b [N_SEG, ...] integers; src [E] into
    M_SRC rows, dst [E] in the layout `name` over N_SEG rows, sorted
    (with the edges reordered to match) on the sorted route."""
    g = gen("gather_mul", name, trailing)
    dst = layout(name, g)
    n_edges = dst.numel()
    src = torch.randint(0, M_SRC, (n_edges,), generator=g)
    x = ints(g, lo, hi, M_SRC, *trailing)
    w = ints(g, lo, hi, n_edges, *trailing)
    b = ints(g, lo, hi, N_SEG, *trailing)
    if route == "sorted":
        o = torch.argsort(dst, stable=True)
        src, dst, w = src[o], dst[o], w[o]
    return x, w, b, src, dst


def plans(src, dst, m, n, dev, route):
    return (SegmentPlan.from_index(put(src, dev), m),
            SegmentPlan.from_index(put(dst, dev), n,
                                   sorted_index=(route == "sorted")))


def off_by_one(t, dev, dtype):
    """`t` on the device as a contiguous view that starts one element
    past a 16-byte boundary."""
    flat = torch.zeros(t.numel() + 1, dtype=dtype, device=dev)
    view = flat[1:].view(t.shape)
    view.copy_(t.to(dtype))
    assert view.data_ptr() % 16 == view.element_size()
    return view


def bounded_case(dtype, trailing):
    """Non-negative operands already rounded to `dtype`, rows of 0 to
    64 entries in shuffled order: no cancellation, so the fp32
    accumulation error, at most 64 * 2^-24 relative, is far below half
    an ulp of a half-type output and one final rounding lands within
    one ulp of the fp64 sum."""
    g = gen("gather_mul_bounded", dtype, trailing)
    lens = torch.randint(0, 65, (N_SEG,), generator=g)
    lens[3], lens[4] = 64, 0
    dst = torch.repeat_interleave(torch.arange(N_SEG), lens)
    dst = dst[torch.randperm(dst.numel(), generator=g)]
    src = torch.randint(0, M_SRC, (dst.numel(),), generator=g)
    x = torch.rand(M_SRC, *trailing, generator=g, dtype=F64).to(dtype)
    w = torch.rand(dst.numel(), *trailing, generator=g, dtype=F64).to(dtype)
    return x, w, src, dst


CLOSURE_M = 30       # gathered rows, 3 edges each
CLOSURE_ROWS = 30    # rows 4 .. 33 of N_SEG hold 3 edges each


def closure_case():
    """Integers in [-4, 4]; every row of either grouping holds 3 edges.
    Rows of up to 16 would keep every fp32 partial sum of the chain an
    integer below 2^24; 3 also keeps the second order, which grows
    with the square of the row length, inside f16's range (the tests
    assert it on the result)."""
    g = gen("gather_mul_closure")
    n_edges = 3 * CLOSURE_M
    src = (torch.arange(n_edges) % CLOSURE_M)[
        torch.randperm(n_edges, generator=g)]
    dst = (4 + torch.arange(n_edges) % CLOSURE_ROWS)[
        torch.randperm(n_edges, generator=g)]
    x = ints(g, -4, 4, CLOSURE_M, 5)
    w = ints(g, -4, 4, n_edges, 5)
    return x, w, src, dst


def closure_chain(x, w, src_plan, dst_plan):
    """First-order gradients of E = |out|^2 / 2 and the force-style
    second order: the gradients of (|dE/dx|^2 + |dE/dw|^2) / 2 with
    respect to x and w.  Every reduction whose value matters is one of
    the ops; the `.sum()`s only seed cotangents of ones.

    Launches, by the closure table: the forward is one sum; its
    backward one sum (dx) and one product (dw); the second order
    differentiates that sum (one sum, one product) and that product
    (two sums), and passes through the forward's backward once more
    (one sum, one product): 6 sums and 3 products."""
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    out = gather_mul_sum(x, w, src_plan, dst_plan)
    energy = 0.5 * (out * out).sum()
    dx, dw = torch.autograd.grad(energy, (x, w), create_graph=True)
    r = 0.5 * ((dx * dx).sum() + (dw * dw).sum())
    hx, hw = torch.autograd.grad(r, (x, w))
    return [t.detach() for t in (out, dx, dw, hx, hw)]


CLOSURE_LAUNCHES = {"sum": 6, "mul": 3}


# ---------------------------------------------------------------------------
# checks shared by the CPU and the device tests
# ---------------------------------------------------------------------------
def check_int(dev, dtype, route, name, trailings=TRAILING):
    for trailing in trailings:
        x, w, b, src, dst = int_case(name, trailing, route)
        sp, dp = plans(src, dst, M_SRC, N_SEG, dev, route)
        out = gather_mul_sum(put(x, dev, dtype), put(w, dev, dtype), sp, dp)
        assert same(out, ref_gms(x, w, src, dst, N_SEG), dtype), \
            f"gather_mul_sum {dtype} {route} {name} {trailing}"
        prod = gather_mul(put(x, dev, dtype), put(b, dev, dtype), sp, dp)
        assert same(prod, ref_gm(x, b, src, dst), dtype), \
            f"gather_mul {dtype} {route} {name} {trailing}"


def check_empty(dev, dtype):
    """Empty rows give 0; E = 0 gives zeros / an empty product; size = 0
    gives an empty sum; the identity plan sums nothing."""
    none = torch.zeros(0, dtype=torch.long)
    x = put(ints(gen("gm_empty"), -8, 8, M_SRC, 5), dev, dtype)
    sp, dp = plans(none, none, M_SRC, N_SEG, dev, "perm")
    w0 = put(torch.zeros(0, 5), dev, dtype)
    out = gather_mul_sum(x, w0, sp, dp)
    assert out.dtype == dtype and out.shape == (N_SEG, 5)
    assert not out.cpu().any()
    b = put(torch.ones(N_SEG, 5), dev, dtype)
    assert gather_mul(x, b, sp, dp).shape == (0, 5)
    # size = 0 on the summed side
    src = torch.tensor([1, 2, 3])
    sp, dp = plans(src, torch.zeros(3, dtype=torch.long), M_SRC, 0, dev,
                   "perm")
    out = gather_mul_sum(x, put(torch.ones(3, 5), dev, dtype), sp, dp)
    assert out.shape == (0, 5) and out.dtype == dtype
    # identity on the gathered side: out[i] = sum_{dst[e] = i} m[e] w[e]
    xi, w, _, _, dst = int_case("gaps", (3,), "perm")
    m = ints(gen("gm_identity"), -8, 8, dst.numel(), 3)
    ident = SegmentPlan.identity(dst.numel(), dev)
    assert ident.csr()[0] is None
    assert torch.equal(ident.csr()[1].cpu(), torch.arange(dst.numel() + 1))
    assert torch.equal(ident.index.cpu(), torch.arange(dst.numel()))
    dp = SegmentPlan.from_index(put(dst, dev), N_SEG)
    out = gather_mul_sum(put(m, dev, dtype), put(w, dev, dtype), ident, dp)
    assert same(out, ref_gms(m, w, torch.arange(dst.numel()), dst, N_SEG),
                dtype)
    # identity on the summed side is the product itself
    sp = SegmentPlan.from_index(put(torch.arange(dst.numel()) % M_SRC, dev),
                                M_SRC)
    xs = ints(gen("gm_identity_x"), -8, 8, M_SRC, 3)
    out = gather_mul_sum(put(xs, dev, dtype), put(w, dev, dtype), sp, ident)
    assert same(out, xs[sp.index.cpu()] * w, dtype)


def model_config(mpnn_type, mlip=True, radius=2.5):
    """A 2-layer stack: an MLIP (energy + forces from a node head), or
    a graph-head regression."""
    from deterministic_graph_data import base_config
    config = base_config(mpnn_type, heads=("node",) if mlip else ("graph",),
                         num_epoch=1, hidden_dim=32, lr=0.005, batch_size=4)
    arch = config["NeuralNetwork"]["Architecture"]
    arch.update({"radius": radius, "equivariance": False,
                 "num_conv_layers": 2})
    if mlip:
        arch.update({"enable_interatomic_potential": True,
                     "energy_weight": 1.0, "energy_peratom_weight": 0.0,
                     "force_weight": 10.0})
    if mpnn_type == "DimeNet":
        arch.update({"num_radial": 6, "num_spherical": 7,
                     "basis_emb_size": 8, "int_emb_size": 64,
                     "out_emb_size": 128, "num_before_skip": 1,
                     "num_after_skip": 2})
    config["NeuralNetwork"]["Variables_of_interest"]["output_dim"] = [1]
    return config


def build_model(mpnn_type, dataset, seed=11, **kwargs):
    from hydragnn_amd.models import create_model_config
    from hydragnn_amd.preprocess import create_dataloaders
    from hydragnn_amd.utils.config import update_config
    config = model_config(mpnn_type, **kwargs)
    loaders = create_dataloaders(dataset, dataset, dataset, 4,
                                 config=config)
    config = update_config(config, *loaders)
    torch.manual_seed(seed)
    return create_model_config(config["NeuralNetwork"], use_gpu=False)


def double_batch(batch):
    for k, v in batch._store.items():
        if torch.is_tensor(v) and v.is_floating_point():
            batch._store[k] = v.double()
    return batch


def energy_force_step(model, batch):
    """(outputs, parameter gradients) of one energy + forces step, as
    fp64 CPU tensors."""
    model.zero_grad(set_to_none=True)
    batch.pos.requires_grad_(True)
    pred = model(batch)
    loss, _ = model.energy_force_loss(pred, batch, create_graph=True)
    loss.backward()
    outs = [p.detach().double().cpu() for p in pred]
    return outs, {k: p.grad.detach().double().cpu()
                  for k, p in model.named_parameters()
                  if p.grad is not None}


def graph_step(model, batch):
    """(outputs, parameter gradients) of one forward + backward of the
    graph-head loss, as fp64 CPU tensors."""
    from hydragnn_amd.train import get_head_indices
    model.zero_grad(set_to_none=True)
    pred = model(batch)
    loss, _ = model.loss(pred, batch.y, get_head_indices(model, batch))
    loss.backward()
    outs = [p.detach().double().cpu() for p in pred]
    return outs, {k: p.grad.detach().double().cpu()
                  for k, p in model.named_parameters()
                  if p.grad is not None}


def rel_err(got, ref):
    """Worst |got - ref| / max|ref| over a dict or list of tensors,
    tensor by tensor.  A tensor that is zero analytically (the bias in
    front of a normalisation: its gradient is the round-off left by
    cancelling terms of the size of the other gradients, 1e-13 here) has
    no scale of its own; one whose reference stays below 1e-9 of the
    largest tensor's is measured against that largest scale instead."""
    pairs = ([(got[k], ref[k]) for k in ref] if isinstance(ref, dict)
             else list(zip(got, ref)))
    top = max(float(b.abs().max()) for _, b in pairs)
    worst = 0.0
    for a, b in pairs:
        scale = float(b.abs().max())
        if scale < 1e-9 * top:
            scale = top
        worst = max(worst, float((a - b).abs().max()) / max(scale, 1e-300))
    return worst
