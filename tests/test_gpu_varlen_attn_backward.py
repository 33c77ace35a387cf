"""Segment-varlen attention on the device: forward with LSE, the two
backward kernels, and the autograd Function pair around them, against
the torch reference evaluated in fp64 on the same values.

Segment sizes are built from the tiling of the instance under test
(T tile rows, B rows per workgroup pass, both read from the extension)
so that one batch crosses the single-row and the empty segment, the
exact-tile and tile+1 boundaries, the more-rows-than-threads loop and
three tiles."""

import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

from hydragnn_amd.ops import get_extension  # noqa: E402
from hydragnn_amd.ops.varlen_attn import (  # noqa: E402
    torch_varlen_attention, varlen_attention, varlen_attention_fn,
    varlen_tiling)

H = 3


def _sizes(dh):
    T, B = varlen_tiling(dh)
    return [1, 0, T - 1, T, T + 1, B + 1, 2 * T + 3]


def _batch(sizes):
    s = torch.tensor(sizes)
    ptr = torch.zeros(len(sizes) + 1, dtype=torch.long)
    ptr[1:] = s.cumsum(0)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), s)
    return ptr.cuda(), batch.cuda()


_CASES = {}


def _case(dtype, dh, sizes=None):
    """Inputs (unit normal q/k/v, normal cotangent w) in ``dtype`` and
    the fp64 truth for them, computed once per (dtype, dh, sizes)."""
    key = (dtype, dh, None if sizes is None else tuple(sizes))
    if key not in _CASES:
        torch.manual_seed(1000 + dh)
        sizes = _sizes(dh) if sizes is None else sizes
        ptr, batch = _batch(sizes)
        N = sum(sizes)
        q, k, v, w = (torch.randn(N, H, dh, device="cuda", dtype=dtype)
                      for _ in range(4))
        qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
        out = torch_varlen_attention(qd, kd, vd, batch)
        dq, dk, dv = torch.autograd.grad(out, (qd, kd, vd), w.double())
        lse = torch.empty(N, H, device="cuda", dtype=torch.float64)
        p = ptr.tolist()
        for lo, hi in zip(p[:-1], p[1:]):
            if hi > lo:
                s = torch.einsum("ihd,jhd->hij", qd[lo:hi], kd[lo:hi]) \
                    / math.sqrt(dh)
                lse[lo:hi] = torch.logsumexp(s, -1).transpose(0, 1)
        _CASES[key] = dict(
            q=q, k=k, v=v, w=w, ptr=ptr, batch=batch,
            out=out.detach(), lse=lse.detach(), grads=(dq, dk, dv))
    return _CASES[key]


def _err(a, b):
    return (a.double() - b).abs().max().item()


def _fn_grads(c):
    x = [c[n].clone().requires_grad_(True) for n in "qkv"]
    out = varlen_attention_fn(*x, c["ptr"], c["batch"])
    return torch.autograd.grad(out, x, c["w"])


@pytest.mark.parametrize("dh", [12, 64, 128])
def test_fp32_forward_lse_and_backward(dh):
    c = _case(torch.float32, dh)
    ext = get_extension(required=True)
    out, lse = ext.varlen_attention_fwd(c["q"], c["k"], c["v"], c["ptr"])
    assert lse.dtype == torch.float32 and lse.shape == c["lse"].shape
    e_out, e_lse = _err(out, c["out"]), _err(lse, c["lse"])
    grads = ext.varlen_attention_bwd(c["q"], c["k"], c["v"], out, lse,
                                     c["w"], c["ptr"])
    e_g = [_err(a, b) for a, b in zip(grads, c["grads"])]
    print(f"fp32 dh={dh}: O {e_out:.2e} LSE {e_lse:.2e} "
          f"dQ/dK/dV {e_g[0]:.2e} {e_g[1]:.2e} {e_g[2]:.2e}")
    assert e_out < 1e-5 and e_lse < 1e-5
    assert max(e_g) < 1e-4
    # the same through the Function pair
    for a, b in zip(_fn_grads(c), c["grads"]):
        assert _err(a, b) < 1e-4


@pytest.mark.parametrize("dh", [16, 64, 128])
def test_bf16_backward_no_worse_than_recompute(dh):
    """bf16: forward at the project's 2e-2; each gradient's max-abs
    error against fp64 truth at most twice the recompute backward's
    (HYDRAGNN_VARLEN_ATTN_BWD=0) on the same inputs.  Both errors are
    printed."""
    c = _case(torch.bfloat16, dh)
    ext = get_extension(required=True)
    out, lse = ext.varlen_attention_fwd(c["q"], c["k"], c["v"], c["ptr"])
    assert out.dtype == torch.bfloat16 and lse.dtype == torch.float32
    assert _err(out, c["out"]) < 2e-2
    assert _err(lse, c["lse"]) < 2e-2
    kern = _fn_grads(c)
    os.environ["HYDRAGNN_VARLEN_ATTN_BWD"] = "0"
    try:
        reco = _fn_grads(c)
    finally:
        os.environ.pop("HYDRAGNN_VARLEN_ATTN_BWD")
    for name, a, b, t in zip(("dQ", "dK", "dV"), kern, reco, c["grads"]):
        assert a.dtype == torch.bfloat16
        ea, eb = _err(a, t), _err(b, t)
        print(f"bf16 dh={dh} {name}: kernel {ea:.3e} recompute {eb:.3e}")
        assert ea <= 2 * eb, (name, ea, eb)


@pytest.mark.parametrize("dh", [12, 128])
def test_long_segment_split_over_workgroups(dh):
    """A segment of six row chunks in a batch whose mean length makes
    the launcher deal the chunks to four workgroups per (graph, head):
    two get two chunks, two get one.  Same bounds as above; and since
    the split only moves rows between workgroups, the same segment
    among enough empty graphs to be launched unsplit gives the same
    bits."""
    _, B = varlen_tiling(dh)
    n = 5 * B + 3
    c = _case(torch.float32, dh, [0, n])
    ext = get_extension(required=True)

    def run(ptr):
        out, lse = ext.varlen_attention_fwd(c["q"], c["k"], c["v"], ptr)
        return (out, lse) + tuple(ext.varlen_attention_bwd(
            c["q"], c["k"], c["v"], out, lse, c["w"], ptr))

    split = run(c["ptr"])
    assert _err(split[0], c["out"]) < 1e-5
    assert _err(split[1], c["lse"]) < 1e-5
    for a, b in zip(split[2:], c["grads"]):
        assert _err(a, b) < 1e-4
    ptr1 = torch.tensor([0] * 8 + [n], device="cuda")
    for a, b in zip(split, run(ptr1)):
        assert torch.equal(a, b)


def test_backward_bitwise_reproducible():
    c = _case(torch.bfloat16, 64)
    a, b = _fn_grads(c), _fn_grads(c)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_noncontiguous_operands():
    """q/k/v as unbind views of a packed [N, 3, H, dh] tensor (as GPS
    produces them) and a non-contiguous cotangent."""
    dh = 12
    c = _case(torch.float32, dh)
    packed = torch.stack([c["q"], c["k"], c["v"]], dim=1) \
        .requires_grad_(True)
    q, k, v = packed.unbind(dim=1)
    assert not q.is_contiguous()
    out = varlen_attention_fn(q, k, v, c["ptr"], c["batch"])
    w = c["w"].transpose(0, 1).contiguous().transpose(0, 1)
    assert not w.is_contiguous()
    (g,) = torch.autograd.grad(out, packed, w)
    want = torch.stack(c["grads"], dim=1)
    assert _err(g, want) < 1e-4


def test_forward_backward_without_host_sync():
    c = _case(torch.float32, 12)
    x = [c[n].clone().requires_grad_(True) for n in "qkv"]
    w = c["w"]
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = varlen_attention_fn(*x, c["ptr"], c["batch"])
        grads = torch.autograd.grad(out, x, w)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    for a, b in zip(grads, c["grads"]):
        assert _err(a, b) < 1e-4


@pytest.mark.parametrize("channels,heads", [(128, 1), (96, 4)])
def test_gps_module_wide_heads_match_dense(channels, heads):
    """HydraGPSConv with head_dim 128 and 24: output and every
    parameter gradient with the kernel path on vs the dense path."""
    from hydragnn_amd.globalatt import HydraGPSConv
    torch.manual_seed(0)
    m = HydraGPSConv(channels, conv=None, heads=heads).to("cuda").eval()
    x = torch.randn(50, channels, device="cuda")
    batch = torch.repeat_interleave(
        torch.arange(5), torch.tensor([3, 20, 7, 12, 8])).to("cuda")
    with torch.no_grad():
        assert m._try_varlen_attention(x, batch) is not None

    def run():
        m.zero_grad()
        out, _ = m(x, None, batch=batch)
        out.square().mean().backward()
        return out.detach(), {n: p.grad.clone()
                              for n, p in m.named_parameters()
                              if p.grad is not None}

    out_v, g_v = run()
    os.environ["HYDRAGNN_VARLEN_ATTN"] = "0"
    try:
        out_d, g_d = run()
    finally:
        os.environ.pop("HYDRAGNN_VARLEN_ATTN")
    assert (out_v - out_d).abs().max() < 1e-4
    assert g_v.keys() == g_d.keys() and "attn.in_proj_weight" in g_v
    for n in g_v:
        assert (g_v[n] - g_d[n]).abs().max() < 1e-4, n


@pytest.mark.parametrize("wrt", ["k", "v"])
def test_second_order_on_device(wrt):
    """The second-order half of test_varlen_attention_matches_dense
    (same shapes and tolerances) for k and v."""
    from hydragnn_amd.ops.scatter import _rowptr_from_sorted
    torch.manual_seed(0)
    sizes = [5, 1, 37, 12, 128]
    batch = torch.repeat_interleave(
        torch.arange(len(sizes)), torch.tensor(sizes)).to("cuda")
    ptr = _rowptr_from_sorted(batch, len(sizes))
    N, dh = int(sum(sizes)), 16
    qkv = {n: torch.randn(N, 4, dh, device="cuda") for n in "qkv"}

    def both(fn):
        a = dict(qkv)
        x = a[wrt] = qkv[wrt].clone().requires_grad_(True)
        g = torch.autograd.grad(fn(a["q"], a["k"], a["v"]).square().sum(),
                                x, create_graph=True)[0]
        return g, torch.autograd.grad(g.square().sum(), x)[0]

    g, gg = both(lambda q, k, v: varlen_attention(q, k, v, ptr, batch))
    rg, rgg = both(lambda q, k, v: torch_varlen_attention(q, k, v, batch))
    assert (g - rg).abs().max() < 1e-4
    assert (gg - rgg).abs().max() < 1e-3
