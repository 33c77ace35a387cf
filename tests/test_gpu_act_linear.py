"""act_linear on the HIP kernels (csrc/act_linear.hip): the weight-gradient
plumbing bit for bit on integer data, the activation and its two
derivatives over every finite bf16 input, each primitive against its
torch double, closure of the flagship pattern on the kernels, and capture
(helpers and bounds: _exact_act_linear.py)."""

import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact_act_linear as X  # noqa: E402
from _exact_act_linear import BF, F32, F64  # noqa: E402
from hydragnn_amd.ops import act_linear as al  # noqa: E402
from hydragnn_amd.ops._extension import get_extension  # noqa: E402

DEV = torch.device("cuda:0")
# the flagship's three shapes and its five-path layer; K > 64 for the
# multi-stage K loop of the forward and dgrad_dg GEMMs, the u phi' prologue
# past the first stage and more than one n tile of the two dgrad GEMMs
SHAPES = [(64, 64), (128, 64), (256, 64), (320, 64), (64, 256), (128, 128)]


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    monkeypatch.delenv("HYDRAGNN_ACT_LINEAR", raising=False)
    monkeypatch.delenv("HYDRAGNN_AMD_FORCE_EAGER", raising=False)
    al.reset_path_counts()


def _ext():
    return get_extension(required=True)


# ---------------------------------------------------------------------------
# 1. GEMM plumbing, bit-exact
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(64, 64), (128, 64), (256, 64), (64, 256),
                                 (320, 64)])
@pytest.mark.parametrize("E", [256, 257, 385, 700, 0])
def test_wgrad_plumbing_is_exact(E, N, K):
    """Integer operands in [-4, 4]: every product and every fp32 partial
    sum is an integer below 2^24, so the kernel's only rounding is the
    final store and the answer is the fp64 one rounded once."""
    gen = torch.Generator().manual_seed(1000 * E + N + K)
    g = X.ints(gen, -4, 4, E, N)
    x = X.ints(gen, -4, 4, E, K)
    gW, gb = _ext().act_linear_wgrad(g.to(DEV, BF), x.to(DEV, BF), None,
                                     False, True)
    ref_W, ref_b = g.t() @ x, g.sum(0)
    assert ref_W.abs().max() < 2 ** 24 if E else True
    assert gW.shape == (N, K) and gb.shape == (N,)
    assert torch.equal(gW.cpu(), ref_W.to(F32).to(BF))
    assert torch.equal(gb.cpu(), ref_b.to(F32).to(BF))


def test_wgrad_chunks_depend_on_E_alone():
    ext = _ext()
    # 700 rows: three chunks of 256, 256 and a ragged 188
    assert ext.act_linear_wgrad_chunks(700) == 3
    assert ext.act_linear_wgrad_chunks(256) == 1
    assert ext.act_linear_wgrad_chunks(257) == 2
    # the flagship's batch-1024 edge count: 473 chunks of 704 rows
    assert ext.act_linear_wgrad_chunks(332668) == 473


# ---------------------------------------------------------------------------
# 2. activation functions, exhaustive
# ---------------------------------------------------------------------------
N_EX = K_EX = 64


@pytest.fixture(scope="module")
def exhaustive():
    hv = X.all_finite_bf16()
    assert hv.numel() == 65280
    n = torch.arange(N_EX)
    sW = 2.0 ** -(n % 4).to(F64)                 # W[n, (n+1)%64] = sW[n]
    W = torch.zeros(N_EX, K_EX, dtype=F64)
    W[n, (n + 1) % K_EX] = sW
    assert not torch.equal(W, W.t())
    sg = 2.0 ** ((n % 3) - 1).to(F64)            # g[e, n]
    su = 2.0 ** ((torch.arange(K_EX) % 3) - 1).to(F64)   # u[e, k]
    return dict(
        hv=hv, h64=hv.to(F64),
        h=hv[:, None].expand(-1, K_EX).contiguous().to(DEV),
        W=W.to(DEV, BF), sW=sW, sg=sg, su=su,
        g=sg.to(BF)[None, :].expand(hv.numel(), -1).contiguous().to(DEV),
        u=su.to(BF)[None, :].expand(hv.numel(), -1).contiguous().to(DEV))


def _check_exhaustive(got, ref, h64, scale, operand=None):
    """got, ref, h64, scale broadcast to got's shape.  ``operand``: the
    fp64 value a prologue rounds to bf16 and the exact multiplier that
    follows; an element outside the bound is excused where it equals the
    multiplier times a bf16 neighbour of the rounded operand."""
    got = got.cpu().to(F64)
    ok = X.exhaustive_ok(got, ref, h64, scale)
    if operand is None:
        assert bool(ok.all()), int((~ok).sum())
        return 0
    p64, mult = operand
    up, dn = X.bf16_neighbours(p64.to(BF))
    excused = ~ok & ((got == mult * up.to(F64)) | (got == mult * dn.to(F64)))
    assert bool((ok | excused).all()), int((~(ok | excused)).sum())
    assert int(excused.sum()) <= 1e-3 * got.numel(), int(excused.sum())
    return int(excused.sum())


def test_exhaustive_forward(exhaustive):
    x = exhaustive
    y = _ext().act_linear_fwd(x["h"], x["W"], None)
    p64 = X.phi(x["h64"])[:, None].expand(-1, N_EX)
    sW = x["sW"][None, :]
    _check_exhaustive(y, sW * p64, x["h64"][:, None], sW, (p64, sW))


def test_exhaustive_dgrad(exhaustive):
    x = exhaustive
    gh = _ext().act_linear_dgrad(x["g"], x["W"], x["h"])
    # column k receives row n = k - 1 of W
    src = (torch.arange(K_EX) - 1) % N_EX
    scale = (x["sg"] * x["sW"])[src][None, :]
    _check_exhaustive(gh, scale * X.dphi(x["h64"])[:, None],
                      x["h64"][:, None], scale)


def test_exhaustive_dgrad_dg(exhaustive):
    x = exhaustive
    dg = _ext().act_linear_dgrad_dg(x["u"], x["W"], x["h"])
    k = (torch.arange(N_EX) + 1) % K_EX
    p64 = x["su"][k][None, :] * X.dphi(x["h64"])[:, None]
    sW = x["sW"][None, :]
    _check_exhaustive(dg, sW * p64, x["h64"][:, None],
                      sW * x["su"][k][None, :], (p64, sW))


def test_exhaustive_dgrad_dh(exhaustive):
    x = exhaustive
    dh = _ext().act_linear_dgrad_dh(x["u"], x["g"], x["W"], x["h"])
    src = (torch.arange(K_EX) - 1) % N_EX
    scale = (x["su"] * (x["sg"] * x["sW"])[src])[None, :]
    _check_exhaustive(dh, scale * X.d2phi(x["h64"])[:, None],
                      x["h64"][:, None], scale)


@pytest.mark.parametrize("with_u", [False, True], ids=["phi", "u_dphi"])
def test_exhaustive_wgrad(exhaustive, with_u):
    """Row e = 64 n + k carries one input value at x[e, k] and a one-hot
    g[e, n], so gW[n, k] = g p(value) with every other term exactly 0."""
    hv = exhaustive["hv"]
    N, K = 256, 64
    rows = N * K
    e = torch.arange(rows)
    for lo in range(0, hv.numel(), rows):
        vals = torch.zeros(rows, dtype=BF)
        part = hv[lo:lo + rows]
        vals[:part.numel()] = part
        xh = torch.zeros(rows, K, dtype=BF)
        xh[e, e % K] = vals
        g = torch.zeros(rows, N, dtype=BF)
        g[e, e // K] = 0.5
        u = None
        if with_u:
            u = torch.zeros(rows, K, dtype=BF)
            u[e, e % K] = 2.0
        gW, _ = _ext().act_linear_wgrad(
            g.to(DEV), xh.to(DEV), None if u is None else u.to(DEV), True,
            False)
        v64 = vals.to(F64).view(N, K)
        p64 = 2.0 * X.dphi(v64) if with_u else X.phi(v64)
        half = torch.full_like(p64, 0.5)
        _check_exhaustive(gW, 0.5 * p64, v64, 1.0 if with_u else 0.5,
                          (p64, half))


# ---------------------------------------------------------------------------
# 3. whole primitives against their doubles
# ---------------------------------------------------------------------------
E_RND = 385


def _random(N, K, seed=0):
    gen = torch.Generator().manual_seed(seed + N + K)

    def rnd(*shape, s=1.0):
        return (s * torch.randn(*shape, generator=gen)).to(DEV, BF)
    return dict(h=rnd(E_RND, K, s=2.0), W=rnd(N, K, s=0.125), b=rnd(N),
                g=rnd(E_RND, N), u=rnd(E_RND, K))


def _sum_abs(kind, h, W, b=None, g=None, u=None):
    """(sum |a_i b_i| in fp64, contraction length) of one primitive."""
    a = lambda t: t.to(F64).abs()  # noqa: E731
    hf = h.to(F32)
    if kind == "fwd":
        p = al._phi(hf).to(BF)
        s = a(p) @ a(W).t()
        return (s + a(b) if b is not None else s), W.shape[1]
    if kind == "dgrad":
        return (a(g) @ a(W)) * a(al._dphi(hf)), W.shape[0]
    if kind == "dgrad_dg":
        p = (u.to(F32) * al._dphi(hf)).to(BF)
        return a(p) @ a(W).t(), W.shape[1]
    if kind == "dgrad_dh":
        return a(u) * (a(g) @ a(W)) * a(al._d2phi(hf)), W.shape[0]
    if kind == "wgrad":
        p = al._phi(hf).to(BF) if u is None \
            else (u.to(F32) * al._dphi(hf)).to(BF)
        return a(g).t() @ a(p), h.shape[0]
    assert kind == "bgrad"
    return a(g).sum(0), h.shape[0]


def _within(got, want, sum_abs, k_len):
    err = (got.to(F64) - want.to(F64)).abs()
    bound = X.random_bound(want, k_len, sum_abs)
    assert got.shape == want.shape
    assert bool((err <= bound).all()), float((err - bound).max())


@pytest.mark.parametrize("N,K", SHAPES)
def test_primitives_match_their_doubles(N, K):
    t = _random(N, K)
    h, W, b, g, u = t["h"], t["W"], t["b"], t["g"], t["u"]
    ext = _ext()
    _within(ext.act_linear_fwd(h, W, b), al.torch_act_linear(h, W, b),
            *_sum_abs("fwd", h, W, b))
    _within(ext.act_linear_fwd(h, W, None), al.torch_act_linear(h, W),
            *_sum_abs("fwd", h, W))
    _within(ext.act_linear_dgrad(g, W, h), al.torch_dgrad(g, W, h),
            *_sum_abs("dgrad", h, W, g=g))
    _within(ext.act_linear_dgrad_dg(u, W, h), al.torch_dgrad_dg(u, W, h),
            *_sum_abs("dgrad_dg", h, W, u=u))
    _within(ext.act_linear_dgrad_dh(u, g, W, h),
            al.torch_dgrad_dh(u, g, W, h),
            *_sum_abs("dgrad_dh", h, W, g=g, u=u))
    gW, gb = ext.act_linear_wgrad(g, h, None, True, True)
    wW, wb = al.torch_wgrad(g, h, None, True)
    _within(gW, wW, *_sum_abs("wgrad", h, W, g=g))
    _within(gb, wb, *_sum_abs("bgrad", h, W, g=g))
    gW, gb = ext.act_linear_wgrad(g, h, u, True, False)
    assert gb.numel() == 0
    _within(gW, al.torch_wgrad(g, h, u)[0],
            *_sum_abs("wgrad", h, W, g=g, u=u))


# ---------------------------------------------------------------------------
# 4. closure
# ---------------------------------------------------------------------------
def _closure_grads(t):
    """First-order grads of e = <act_linear(h, W, b), r> w.r.t. (h, W, b)
    and grads of <gh, c> w.r.t. (h, W, r): each one primitive's output."""
    h, W, b, r = (t[k].detach().requires_grad_() for k in "hWbg")
    e = (al.act_linear(h, W, b) * r).sum()
    first = torch.autograd.grad(e, (h, W, b), retain_graph=True)
    (gh,) = torch.autograd.grad(e, h, create_graph=True)
    second = torch.autograd.grad((gh * t["u"]).sum(), (h, W, r))
    return first + second


def test_flagship_pattern_stays_on_the_kernels(monkeypatch):
    N, K = 128, 64
    t = _random(N, K, seed=5)
    got = _closure_grads(t)
    counts = al.path_counts()
    assert counts["composition"] == 0, counts
    assert counts == {"act_linear": 1, "dgrad": 2, "wgrad": 2,
                      "dgrad_dg": 1, "dgrad_dh": 1, "composition": 0}
    monkeypatch.setenv("HYDRAGNN_AMD_FORCE_EAGER", "1")
    want = _closure_grads(t)
    monkeypatch.delenv("HYDRAGNN_AMD_FORCE_EAGER")
    h, W, g, u = t["h"], t["W"], t["g"], t["u"]
    kinds = [("dgrad", dict(g=g)), ("wgrad", dict(g=g)),
             ("bgrad", dict(g=g)), ("dgrad_dh", dict(g=g, u=u)),
             ("wgrad", dict(g=g, u=u)), ("dgrad_dg", dict(u=u))]
    for a, b_, (kind, kw) in zip(got, want, kinds):
        _within(a, b_, *_sum_abs(kind, h, W, **kw))
    # the switch: no kernel of this family runs
    al.reset_path_counts()
    monkeypatch.setenv("HYDRAGNN_ACT_LINEAR", "0")
    _closure_grads(t)
    counts = al.path_counts()
    assert counts["composition"] > 0
    assert all(v == 0 for k, v in counts.items() if k != "composition")


def test_force_pass_skips_the_weight_gradient():
    t = _random(64, 64, seed=6)
    h, W, b = (t[k].detach().requires_grad_() for k in "hWb")
    e = (al.act_linear(h, W, b) * t["g"]).sum()
    torch.autograd.grad(e, h, create_graph=True)
    counts = al.path_counts()
    assert counts["wgrad"] == 0 and counts["composition"] == 0, counts


# ---------------------------------------------------------------------------
# 5. capture
# ---------------------------------------------------------------------------
def test_capture_replays_bit_equal_to_eager():
    N, K = 128, 64
    t = _random(N, K, seed=7)
    h, W, b = (t[k].detach().requires_grad_() for k in "hWb")
    r = t["g"]

    def run():
        _, first, second = X.flagship(al.act_linear, h, W, b, r)
        return first + second

    eager = [x.clone() for x in run()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        static = run()
    for _ in range(2):
        for x in static:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b_ in zip(static, eager):
            assert torch.equal(a, b_)
    assert al.path_counts()["composition"] == 0
