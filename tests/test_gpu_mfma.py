"""MFMA linear kernel numerics vs torch.matmul (asymmetric operands —
transpose-detecting per the CDNA4 guide) + gradient parity + timing."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

from hydragnn_amd.ops import get_extension  # noqa: E402
from hydragnn_amd.ops.mfma_linear import (  # noqa: E402
    MFMALinear, _MFMAMatmul,
)


def _asym(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    # asymmetric, non-uniform magnitudes: catches transposed layouts
    t = torch.randn(*shape, generator=g)
    t += torch.arange(shape[-1]).float() * 0.01
    return t.to("cuda", torch.bfloat16)


@pytest.mark.parametrize("M,N,K", [(512, 64, 64), (1000, 128, 64),
                                   (4096, 320, 64), (300, 64, 320)])
@pytest.mark.parametrize("trans_b", [True, False])
def test_mfma_matmul_matches_torch(M, N, K, trans_b):
    ext = get_extension(required=True)
    A = _asym((M, K), 1)
    B = _asym((N, K) if trans_b else (K, N), 2)
    out = ext.mfma_linear(A, B, None, trans_b)
    ref = (A.float() @ (B.t() if trans_b else B).float())
    err = (out.float() - ref).abs().max() / ref.abs().max().clamp(min=1)
    assert err < 2e-2, f"rel err {err:.3e}"
    # tighter check vs bf16 torch matmul
    ref_bf = A @ (B.t() if trans_b else B)
    err2 = (out.float() - ref_bf.float()).abs().max()
    assert err2 < 0.15 * ref.abs().max(), err2


def test_mfma_matmul_bias():
    ext = get_extension(required=True)
    A = _asym((512, 64), 3)
    B = _asym((128, 64), 4)
    bias = torch.randn(128, device="cuda")
    out = ext.mfma_linear(A, B, bias, True)
    ref = A.float() @ B.t().float() + bias
    assert (out.float() - ref).abs().max() < 0.15 * ref.abs().max()
    # that bound is wider than max|bias|: a dropped bias must not pass
    # (bit-exact bias cases: test_gpu_linear_exact.py)
    err = (out.float() - ref).abs()
    err_nobias = (out.float() - (ref - bias)).abs()
    assert err.max() < err_nobias.max()


def test_mfma_linear_grads_match_reference():
    torch.manual_seed(0)
    lin = MFMALinear(64, 128).cuda()
    ref = torch.nn.Linear(64, 128).cuda()
    ref.load_state_dict(lin.state_dict())
    x = _asym((2048, 64), 5).requires_grad_(True)
    x2 = x.detach().clone().requires_grad_(True)
    y = lin(x)
    y2 = ref(x2.float()).to(torch.bfloat16)
    assert (y.float() - y2.float()).abs().max() < 0.2
    g1 = torch.autograd.grad((y.float() ** 2).sum(), (x, lin.weight),
                             create_graph=True)
    g2 = torch.autograd.grad((y2.float() ** 2).sum(), (x2, ref.weight),
                             create_graph=True)
    for a, b in zip(g1, g2):
        scale = b.abs().max().clamp(min=1)
        assert ((a.float() - b.float()).abs().max() / scale) < 5e-2
    # second order flows
    h = torch.autograd.grad(g1[0].float().pow(2).sum(), x)
    assert torch.isfinite(h[0].float()).all()


def test_mfma_throughput_beats_blaslt():
    """A/B on the radial-MLP shape within one process."""
    import time
    ext = get_extension(required=True)
    M, N, K = 200_000, 64, 64
    A = torch.randn(M, K, device="cuda").bfloat16()
    W = torch.randn(N, K, device="cuda").bfloat16()

    def bench(fn, iters=20):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e6

    t_mfma = bench(lambda: ext.mfma_linear(A, W, None, True))
    t_blas = bench(lambda: A @ W.t())
    if t_mfma >= t_blas * 1.5:
        # one retry after clearing allocator state another test may
        # have left behind (graph pools / cross-stream blocks)
        torch.cuda.empty_cache()
        t_mfma = bench(lambda: ext.mfma_linear(A, W, None, True))
        t_blas = bench(lambda: A @ W.t())
    print(f"mfma {t_mfma:.1f}us vs hipBLASLt {t_blas:.1f}us")
    assert t_mfma < t_blas * 1.5, (t_mfma, t_blas)


def test_hipgraph_capture_matches_eager():
    """Guard against silent capture corruption: the captured step's
    losses track an eager run of the same seed/model/batch."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    import bench as bench_mod

    losses = {}
    for mode in ("eager", "graph"):
        os.environ["HYDRAGNN_HIPGRAPH"] = "0" if mode == "eager" else "1"
        torch.manual_seed(123)
        model, batch, step = bench_mod.build_model_and_batch(
            device="cuda:0", local_batch=16, seed=99)
        n = 9 if mode == "eager" else 5
        ls = []
        for _ in range(n):
            ls.append(float(step().detach().float().cpu()))
        losses[mode] = ls
        del model, batch, step
        torch.cuda.empty_cache()
    os.environ.pop("HYDRAGNN_HIPGRAPH", None)
    # graph mode ran 3 side-stream warmups + 1 sanity replay before the
    # measured loop, so its 5 losses align with eager steps 5..9
    for a, b in zip(losses["eager"][4:], losses["graph"]):
        assert abs(a - b) / max(abs(a), 1e-6) < 0.08, losses


def _irreps_ref(x, W, lmap, bias=None):
    W_m = W[lmap]  # [D, Cin, Cout]
    out = torch.bmm(x.permute(2, 0, 1), W_m).permute(1, 2, 0)
    if bias is not None:
        out = torch.cat([out[:, :, :1] + bias.view(1, -1, 1),
                         out[:, :, 1:]], dim=-1)
    return out.contiguous()


@pytest.mark.parametrize("N,Cin,Cout,lmax", [(777, 64, 64, 2),
                                             (1024, 64, 128, 1),
                                             (300, 96, 64, 3)])
def test_irreps_linear_matches_bmm(N, Cin, Cout, lmax):
    from hydragnn_amd.ops.irreps_linear import irreps_linear
    torch.manual_seed(0)
    D = (lmax + 1) ** 2
    lmap = torch.cat([torch.full((2 * l + 1,), l, dtype=torch.long)
                      for l in range(lmax + 1)]).to("cuda")
    x = _asym((N, Cin, D), 1).contiguous()
    W = (_asym((lmax + 1, Cin, Cout), 2) * 0.2).contiguous()
    bias = torch.randn(Cout, device="cuda").float()
    out = irreps_linear(x, W, lmap, bias)
    ref = _irreps_ref(x.float(), W.float(), lmap, bias)
    rel = (out.float() - ref).abs().max() / ref.abs().max()
    assert rel < 2e-2, f"rel {rel:.3e}"
    # fused residual epilogue
    res = _asym((N, Cout, D), 7).contiguous()
    out2 = irreps_linear(x, W, lmap, bias, add=res)
    rel2 = ((out2.float() - (ref + res.float())).abs().max()
            / ref.abs().max())
    assert rel2 < 2e-2, f"residual rel {rel2:.3e}"


def test_irreps_linear_grads_match_reference():
    from hydragnn_amd.ops.irreps_linear import irreps_linear
    torch.manual_seed(0)
    N, C, lmax = 500, 64, 2
    D = (lmax + 1) ** 2
    lmap = torch.cat([torch.full((2 * l + 1,), l, dtype=torch.long)
                      for l in range(lmax + 1)]).to("cuda")
    x = (_asym((N, C, D), 3) * 0.3).contiguous().requires_grad_(True)
    W = (_asym((lmax + 1, C, C), 4) * 0.2).contiguous().requires_grad_(True)
    out = irreps_linear(x, W, lmap)
    gx, gw = torch.autograd.grad(out.square().sum(), (x, W),
                                 create_graph=True)
    xr = x.detach().float().requires_grad_(True)
    Wr = W.detach().float().requires_grad_(True)
    refout = _irreps_ref(xr, Wr, lmap)
    gxr, gwr = torch.autograd.grad(refout.square().sum(), (xr, Wr),
                                   create_graph=True)
    for a, b, tol, name in [(gx.float(), gxr, 5e-2, "gx"),
                            (gw.float(), gwr, 5e-2, "gw")]:
        rel = (a - b).abs().max() / (b.abs().max() + 1e-9)
        assert rel < tol, f"{name} rel {rel:.3e}"
    # second order through gx
    ggx = torch.autograd.grad(gx.square().sum(), x)[0]
    ggxr = torch.autograd.grad(gxr.square().sum(), xr)[0]
    rel = (ggx.float() - ggxr).abs().max() / (ggxr.abs().max() + 1e-9)
    assert rel < 1e-1, f"second order rel {rel:.3e}"


@pytest.mark.parametrize("M,N,K", [(21504, 1, 64), (1000, 4, 64),
                                   (512, 8, 128)])
def test_gemv_small_n_matches_torch(M, N, K):
    ext = get_extension(required=True)
    A = _asym((M, K), 3)
    W = _asym((N, K), 4)
    bias = torch.randn(N, device="cuda")
    out = ext.gemv_small_n(A, W, bias)
    ref = A.float() @ W.t().float() + bias
    err = (out.float() - ref).abs().max() / ref.abs().max().clamp(min=1)
    assert err < 2e-2, f"rel err {err:.3e}"


def test_gemv_linear_grads_match_fp32():
    """MFMALinear's narrow-output dispatch: fwd + double backward vs a
    plain fp32 nn.Linear reference."""
    torch.manual_seed(0)
    M, K = 4096, 64
    lin = MFMALinear(K, 1).to("cuda", torch.bfloat16)
    ref = torch.nn.Linear(K, 1).to("cuda")
    with torch.no_grad():
        ref.weight.copy_(lin.weight.float())
        ref.bias.copy_(lin.bias.float())
    x = (torch.randn(M, K) * 0.5).to("cuda", torch.bfloat16)
    x1 = x.clone().requires_grad_(True)
    x2 = x.float().clone().requires_grad_(True)

    y1 = lin(x1)
    # double-backward shape: grad wrt x then loss on that grad
    g1 = torch.autograd.grad(y1.sum(), x1, create_graph=True)[0]
    loss1 = (g1.float() ** 2).sum() + y1.float().sum()
    loss1.backward()

    y2 = ref(x2)
    g2 = torch.autograd.grad(y2.sum(), x2, create_graph=True)[0]
    loss2 = (g2 ** 2).sum() + y2.sum()
    loss2.backward()

    assert torch.allclose(y1.float(), y2, rtol=5e-2, atol=5e-2)
    assert torch.allclose(lin.weight.grad.float(),
                          ref.weight.grad, rtol=5e-2, atol=1.0)
    assert torch.allclose(x1.grad.float(), x2.grad,
                          rtol=5e-2, atol=5e-2)


@pytest.mark.parametrize("M,N,K", [(512, 128, 64), (512, 64, 128)])
def test_mfma_second_order_weight_grad(M, N, K):
    """Second-order weight gradient through _MFMAMatmul (the force
    double-backward path) vs fp32 autograd — NON-square shapes so a
    transposed result cannot hide (r2 regression test: the old
    trans_b=False path returned g^T A instead of A^T g)."""
    torch.manual_seed(0)
    x = (_asym((M, K), 11) * 0.2).requires_grad_(True)
    w = (_asym((N, K), 12) * 0.2).requires_grad_(True)
    y = _MFMAMatmul.apply(x, w, True)       # x @ w^T
    gx = torch.autograd.grad(y.float().square().sum(), x,
                             create_graph=True)[0]
    # second backward: gradient of ||gx||^2 w.r.t. w exercises the
    # trans_b=False gB path
    gw2 = torch.autograd.grad(gx.float().square().sum(), w)[0]

    xr = x.detach().float().requires_grad_(True)
    wr = w.detach().float().requires_grad_(True)
    yr = xr @ wr.t()
    gxr = torch.autograd.grad(yr.square().sum(), xr,
                              create_graph=True)[0]
    gw2r = torch.autograd.grad(gxr.square().sum(), wr)[0]
    rel = (gw2.float() - gw2r).abs().max() / gw2r.abs().max().clamp(min=1e-6)
    assert rel < 5e-2, f"rel {rel:.3e}"
