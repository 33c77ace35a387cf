"""Second order of segment-varlen attention on the device: the
``varlen_attention_bwd2`` kernels and the Function pair's double
backward around them.

No absolute bound is derived for these sums.  The criterion throughout:
against fp64 truth on the same values, the kernel route's max-abs error
in each gradient is at most twice that of the torch second-order route
(``HYDRAGNN_VARLEN_ATTN_BWD2=0``) in the same dtype on the same inputs;
the factor 2 allows for a different summation order and nothing more.
Both errors are printed.

Segment sizes are built from the tiling of the second-order instance
under test (T tile rows, B rows per workgroup pass), so one batch
crosses the single-row and the empty segment, the exact-tile and tile+1
boundaries, the more-rows-than-threads loop and three tiles."""

import copy
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

from hydragnn_amd.ops import get_extension  # noqa: E402
from hydragnn_amd.ops.varlen_attn import (  # noqa: E402
    _VarlenAttnBwd, torch_varlen_attention, torch_varlen_attention_bwd2,
    torch_varlen_attention_fwd, varlen_attention_fn, varlen_tiling2)

H = 3
NAMES = ("gQ", "gK", "gV", "gdO")


def _sizes(dh):
    T, B = varlen_tiling2(dh)
    return [1, 0, T - 1, T, T + 1, B + 1, 2 * T + 3]


def _batch(sizes):
    s = torch.tensor(sizes)
    ptr = torch.zeros(len(sizes) + 1, dtype=torch.long)
    ptr[1:] = s.cumsum(0)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), s)
    return ptr.cuda(), batch.cuda()


class _torch_route:
    """The parent's second-order route, for the duration of a block."""

    def __enter__(self):
        os.environ["HYDRAGNN_VARLEN_ATTN_BWD2"] = "0"

    def __exit__(self, *exc):
        os.environ.pop("HYDRAGNN_VARLEN_ATTN_BWD2")


_CASES = {}


def _case(dtype, dh, sizes=None):
    """Unit-normal operands and cotangents in ``dtype``, the forward's
    (O, LSE) from the kernel, and the fp64 truth of the four
    second-order gradients, computed once per (dtype, dh, sizes)."""
    key = (dtype, dh, None if sizes is None else tuple(sizes))
    if key not in _CASES:
        torch.manual_seed(2000 + dh)
        sizes = _sizes(dh) if sizes is None else sizes
        ptr, batch = _batch(sizes)
        N = sum(sizes)
        c = {n: torch.randn(N, H, dh, device="cuda", dtype=dtype)
             for n in ("q", "k", "v", "g", "cq", "ck", "cv")}
        d = {n: t.double() for n, t in c.items()}
        out, lse = torch_varlen_attention_fwd(d["q"], d["k"], d["v"], ptr)
        truth = torch_varlen_attention_bwd2(
            d["q"], d["k"], d["v"], out, lse, d["g"], d["cq"], d["ck"],
            d["cv"], ptr)
        ext = get_extension(required=True)
        c["out"], c["lse"] = ext.varlen_attention_fwd(
            c["q"], c["k"], c["v"], ptr)
        c.update(ptr=ptr, batch=batch, truth=truth)
        _CASES[key] = c
    return _CASES[key]


def _err(a, b):
    return (a.double() - b).abs().max().item()


def _kernel(c, ptr=None):
    ext = get_extension(required=True)
    return ext.varlen_attention_bwd2(
        c["q"], c["k"], c["v"], c["out"], c["lse"], c["g"], c["cq"],
        c["ck"], c["cv"], c["ptr"] if ptr is None else ptr)


def _function_node(c):
    """The four gradients through _VarlenAttnBwd's backward, on
    whichever route the environment selects."""
    x = [c[n].clone().requires_grad_(True) for n in ("q", "k", "v", "g")]
    first = _VarlenAttnBwd.apply(x[0], x[1], x[2], c["out"], c["lse"],
                                 x[3], c["ptr"], c["batch"])
    return torch.autograd.grad(first, x, (c["cq"], c["ck"], c["cv"]))


def _no_worse(tag, got, ref, truth):
    for name, a, b, t in zip(NAMES, got, ref, truth):
        assert a.dtype == b.dtype and torch.isfinite(a).all()
        ea, eb = _err(a, t), _err(b, t)
        print(f"{tag} {name}: kernel {ea:.3e} torch route {eb:.3e}")
        assert ea <= 2 * eb, (tag, name, ea, eb)


@pytest.mark.parametrize("dtype,dh", [
    (torch.float32, 12), (torch.float32, 64), (torch.float32, 128),
    (torch.bfloat16, 16), (torch.bfloat16, 64), (torch.bfloat16, 128)])
def test_entry_point_no_worse_than_torch_route(dtype, dh):
    c = _case(dtype, dh)
    got = _kernel(c)
    assert all(g.dtype == dtype and g.shape == c["q"].shape for g in got)
    with _torch_route():
        ref = _function_node(c)
    tag = f"{'fp32' if dtype == torch.float32 else 'bf16'} dh={dh}"
    _no_worse(tag, got, ref, c["truth"])
    # the Function node on its default route runs the same kernels
    for a, b in zip(_function_node(c), got):
        assert torch.equal(a, b)


def _force_style(fn, q, k, v, w):
    x = [t.clone().requires_grad_(True) for t in (q, k, v)]
    first = torch.autograd.grad((fn(*x) * w).sum(), x, create_graph=True)
    loss = sum(g.square().sum() for g in first)
    return torch.autograd.grad(loss, x)


@pytest.mark.parametrize("dtype,dh", [(torch.float32, 12),
                                      (torch.bfloat16, 16)])
def test_force_style_step_without_host_sync(dtype, dh):
    c = _case(dtype, dh)
    q, k, v, w = c["q"], c["k"], c["v"], c["g"]

    def fn(a, b, d):
        return varlen_attention_fn(a, b, d, c["ptr"], c["batch"])

    truth = _force_style(
        lambda a, b, d: torch_varlen_attention(a, b, d, c["batch"]),
        q.double(), k.double(), v.double(), w.double())
    with _torch_route():
        ref = _force_style(fn, q, k, v, w)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = _force_style(fn, q, k, v, w)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    _no_worse(f"force-style dh={dh}", got, ref, truth)


@pytest.mark.parametrize("dh", [12, 128])
def test_long_segment_split_over_workgroups(dh):
    """A segment of six row chunks in a batch whose mean length makes
    the launcher deal the chunks to four workgroups per (graph, head).
    The split only moves rows between workgroups, so the same segment
    among enough empty graphs to be launched unsplit gives the same
    bits, and so does a second run."""
    _, B = varlen_tiling2(dh)
    n = 5 * B + 3
    c = _case(torch.float32, dh, [0, n])
    split = _kernel(c)
    with _torch_route():
        ref = _function_node(c)
    _no_worse(f"long dh={dh}", split, ref, c["truth"])
    ptr1 = torch.tensor([0] * 8 + [n], device="cuda")
    for a, b, again in zip(split, _kernel(c, ptr1), _kernel(c)):
        assert torch.equal(a, b)
        assert torch.equal(a, again)


def test_noncontiguous_operands():
    """q/k/v as unbind views of a packed [N, 3, H, dh] tensor (as GPS
    produces them) and a non-contiguous cotangent: the same values
    reach the same kernels, so the same bits come back."""
    dh = 12
    c = _case(torch.float32, dh)

    def fn(a, b, d):
        return varlen_attention_fn(a, b, d, c["ptr"], c["batch"])

    want = torch.stack(_force_style(fn, c["q"], c["k"], c["v"], c["g"]),
                       dim=1)
    packed = torch.stack([c["q"], c["k"], c["v"]], dim=1) \
        .requires_grad_(True)
    q, k, v = packed.unbind(dim=1)
    w = c["g"].transpose(0, 1).contiguous().transpose(0, 1)
    assert not q.is_contiguous() and not w.is_contiguous()
    (first,) = torch.autograd.grad(fn(q, k, v), packed, w,
                                   create_graph=True)
    (got,) = torch.autograd.grad(first.square().sum(), packed)
    assert torch.equal(got, want)


def test_force_style_step_graph_capture():
    """The force-style step captured in a device graph after a warm-up
    on a side stream; its replay equals eager bit for bit."""
    from hydragnn_amd.ops.scatter import _rowptr_from_sorted
    torch.manual_seed(0)
    sizes = [5, 1, 37, 12, 128]
    batch = torch.repeat_interleave(
        torch.arange(len(sizes)), torch.tensor(sizes)).to("cuda")
    ptr = _rowptr_from_sorted(batch, len(sizes))
    N, dh = sum(sizes), 16
    q, k, v = (torch.randn(N, 4, dh, device="cuda").requires_grad_(True)
               for _ in range(3))
    w = torch.randn(N, 4, dh, device="cuda")

    def step():
        out = varlen_attention_fn(q, k, v, ptr, batch)
        first = torch.autograd.grad((out * w).sum(), (q, k, v),
                                    create_graph=True)
        loss = sum(g.square().sum() for g in first)
        return torch.autograd.grad(loss, (q, k, v))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            eager = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, eager):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)


def test_gps_layer_force_style_parameter_gradients():
    """HydraGPSConv(64, heads=4) on features that depend on a position
    leaf, graphs of 1, 0, 40 and 130 nodes: parameter gradients of a
    force-style loss with the kernel route and with the torch route,
    each against the same layer in fp64 on the CPU."""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    from hydragnn_amd.globalatt import HydraGPSConv
    torch.manual_seed(0)
    layer = HydraGPSConv(64, conv=None, heads=4).eval()
    sizes = torch.tensor([1, 0, 40, 130])
    batch = torch.repeat_interleave(torch.arange(4), sizes)
    pos0 = torch.randn(int(sizes.sum()), 3, dtype=torch.float64)
    proj = torch.randn(3, 64, dtype=torch.float64)

    def grads(m, batch, dtype, device):
        m.zero_grad()
        pos = pos0.to(device=device, dtype=dtype).requires_grad_(True)
        x = torch.sin(pos @ proj.to(device=device, dtype=dtype))
        out, _ = m(x, None, batch=batch.to(device))
        (force,) = torch.autograd.grad(out.square().sum(), pos,
                                       create_graph=True)
        force.square().sum().backward()
        return {n: p.grad.detach().clone()
                for n, p in m.named_parameters() if p.grad is not None}

    # the CPU layer takes the dense-batch path; only the math backend
    # of its attention differentiates twice
    with sdpa_kernel(SDPBackend.MATH):
        truth = grads(copy.deepcopy(layer).double(), batch,
                      torch.float64, "cpu")
    dev = copy.deepcopy(layer).to("cuda")
    got = grads(dev, batch, torch.float32, "cuda")
    with _torch_route():
        ref = grads(dev, batch, torch.float32, "cuda")
    assert got.keys() == truth.keys() == ref.keys()
    assert "attn.in_proj_weight" in got
    for n in got:
        ea = _err(got[n].cpu(), truth[n])
        eb = _err(ref[n].cpu(), truth[n])
        print(f"layer {n}: kernel {ea:.3e} torch route {eb:.3e}")
        assert torch.isfinite(got[n]).all()
        assert ea <= 2 * eb, (n, ea, eb)
