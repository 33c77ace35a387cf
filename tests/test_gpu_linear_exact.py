"""Bit-exact tests of the bf16 linear kernels (`mfma_linear_kernel`,
`gemv_small_n_kernel`, `irreps_linear_kernel<TRANS_W>`,
`irreps_linear_gw_kernel`) and of the Python dispatch around them.

Operands are seeded integers in [-4, 4] (bias and residual in [-8, 8]):
every product and fp32 partial sum is an exact integer whatever the
accumulation order, so the only rounding is the round-to-nearest-even
store to bf16 and the fp64 CPU reference fixes every output bit.  A
wrong tile, a transposed fragment, a wrong l slice, a dropped bias or a
dropped residual changes bits.  The kernel-level cases call the
extension entry points directly, which take fewer rows than the Python
dispatch does.

Dispatch-level cases differentiate with cotangents, as
test_linear_autograd_closure.py does, so no rounded output feeds
another product.  With 300 rows the split-K weight gradient does not
split: every result is rounded once -> exact.  For irreps shapes whose
backward leaves the kernels (bf16 bmm + fold), the cotangent has four
nonzero rows so that every intermediate is an integer <= 256 (asserted
on the reference) -> exact as well.  No case uses an error bound.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

from _exact_linear import (  # noqa: E402
    BF, F32, F64, fold_exact, fwd_envelope, gw_envelope, ints,
    irreps_formula, leaf, lmap_for, same, sparse_rows,
)
from hydragnn_amd.ops import get_extension  # noqa: E402
from hydragnn_amd.ops.mfma_linear import MFMALinear  # noqa: E402

DEV = "cuda"


def _dev(t, dtype=BF):
    return t.to(device=DEV, dtype=dtype).contiguous()


def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1009 + int(k) + 1
    return torch.Generator().manual_seed(seed)


def _exact(out, ref):
    assert out.dtype == BF
    assert ref.abs().max() < 2 ** 24
    assert torch.equal(out.cpu(), ref.to(F32).to(BF))


# ---------------------------------------------------------------------------
# A. kernel level
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [32, 64, 96])
@pytest.mark.parametrize("N", [64, 128, 192])
@pytest.mark.parametrize("M", [1, 127, 128, 129, 300])
def test_mfma_linear_exact(M, N, K):
    ext = get_extension(required=True)
    gen = _gen(M, N, K)
    A = ints(gen, -4, 4, M, K)
    B = ints(gen, -4, 4, N, K)            # [N, K]; B^T for trans_b=False
    bias = ints(gen, -8, 8, N)
    for trans_b in (True, False):
        Bd = _dev(B if trans_b else B.t())
        for b in (None, bias):
            out = ext.mfma_linear(_dev(A), Bd,
                                  None if b is None else _dev(b, F32),
                                  trans_b)
            ref = A @ B.t() + (0 if b is None else b)
            _exact(out, ref)


def test_mfma_linear_empty():
    ext = get_extension(required=True)
    out = ext.mfma_linear(torch.zeros(0, 64, device=DEV, dtype=BF),
                          torch.zeros(128, 64, device=DEV, dtype=BF),
                          None, True)
    assert out.shape == (0, 128) and out.dtype == BF


@pytest.mark.parametrize("K", [8, 16, 64, 72, 128])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 257])
@pytest.mark.parametrize("N", range(1, 9))
def test_gemv_small_n_exact(N, M, K):
    ext = get_extension(required=True)
    gen = _gen(N, M, K)
    A = ints(gen, -4, 4, M, K)
    W = ints(gen, -4, 4, N, K)
    bias = ints(gen, -8, 8, N)
    for b in (None, bias):
        out = ext.gemv_small_n(_dev(A), _dev(W),
                               None if b is None else _dev(b, F32))
        _exact(out, A @ W.t() + (0 if b is None else b))


_IRREPS_FWD = [(ci, co, lmax)
               for ci, co in ((32, 64), (64, 64), (96, 64), (64, 128))
               for lmax in range(4)
               if fwd_envelope(ci, co, (lmax + 1) ** 2, lmax + 1)]


@pytest.mark.parametrize("trans_w", [False, True])
@pytest.mark.parametrize("c_in,c_out,lmax", _IRREPS_FWD)
@pytest.mark.parametrize("N", [1, 31, 32, 33, 100])
def test_irreps_linear_exact(N, c_in, c_out, lmax, trans_w):
    ext = get_extension(required=True)
    d, n_l = (lmax + 1) ** 2, lmax + 1
    gen = _gen(N, c_in, c_out, lmax, trans_w)
    lmap = lmap_for(lmax)
    x = ints(gen, -4, 4, N, c_in, d)
    W = ints(gen, -4, 4, n_l, c_in, c_out)
    bias = ints(gen, -8, 8, c_out)
    add = ints(gen, -8, 8, N, c_out, d)
    xd = _dev(x)
    Wd = _dev(W.transpose(1, 2) if trans_w else W)   # [L, Cout, Cin]
    lmap_d = lmap.to(DEV)
    for b in (None, bias):
        for a in (None, add):
            out = ext.irreps_linear(
                xd, Wd, lmap_d, None if b is None else _dev(b, F32),
                trans_w, None if a is None else _dev(a))
            _exact(out, irreps_formula(x, W, lmap, b, a))


def _gw_case(N, c_in, c_out, lmax, nblocks):
    ext = get_extension(required=True)
    d, n_l = (lmax + 1) ** 2, lmax + 1
    assert gw_envelope(c_in, c_out, d, n_l)
    gen = _gen(N, c_in, c_out, lmax, nblocks)
    lmap = lmap_for(lmax)
    x = ints(gen, -4, 4, N, c_in, d)
    g = ints(gen, -4, 4, N, c_out, d)
    parts = ext.irreps_linear_gw(_dev(x), _dev(g), lmap.to(DEV), n_l,
                                 nblocks)
    assert parts.shape == (nblocks, n_l, c_in, c_out)
    assert parts.dtype == F32
    gw_m = torch.einsum("nim,nom->mio", x, g)
    ref = torch.zeros(n_l, c_in, c_out, dtype=F64).index_add_(
        0, lmap, gw_m)
    assert ref.abs().max() < 2 ** 24
    assert torch.equal(parts.sum(0).double().cpu(), ref)


_GW_CH = [(32, 32), (32, 64), (64, 32), (64, 64), (16, 64)]


@pytest.mark.parametrize("lmax", range(4))
@pytest.mark.parametrize("c_in,c_out", _GW_CH)
@pytest.mark.parametrize("N", [1, 32, 33, 101])
def test_irreps_linear_gw_exact(N, c_in, c_out, lmax):
    """One block per 32-row tile."""
    _gw_case(N, c_in, c_out, lmax, (N + 31) // 32)


@pytest.mark.parametrize("lmax", range(4))
@pytest.mark.parametrize("c_in,c_out", _GW_CH)
def test_irreps_linear_gw_persistent_stride(c_in, c_out, lmax):
    """Two persistent blocks striding six tiles (the last one partial):
    an odd count would leave the blocks uneven as well."""
    _gw_case(161, c_in, c_out, lmax, 2)


# ---------------------------------------------------------------------------
# D. Python dispatch on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [(64, 128), (128, 64), (64, 1),
                                        (64, 4)])
@pytest.mark.parametrize("w_dtype,x_dtype", [(F32, BF), (F32, F32),
                                             (BF, BF)],
                         ids=["autocast-xbf", "autocast-x32", "bf16"])
def test_mfma_linear_module_closure(w_dtype, x_dtype, n_in, n_out):
    """`MFMALinear` on the real kernels keeps every first- and
    second-order term, the weight term of d(dE/dx)/dW included, for
    fp32 parameters under bf16 autocast and for bf16 parameters."""
    rows = 300        # split-K factor 1: each result is rounded once
    gen = _gen(n_in, n_out)
    xi = ints(gen, -4, 4, rows, n_in)
    wi = ints(gen, -4, 4, n_out, n_in)
    bi = ints(gen, -8, 8, n_out)
    ci = ints(gen, -4, 4, rows, n_out)
    c2i = ints(gen, -4, 4, rows, n_in)
    c3i = ints(gen, -4, 4, n_out, n_in)

    lin = MFMALinear(n_in, n_out).to(DEV, w_dtype)
    with torch.no_grad():
        lin.weight.copy_(wi)
        lin.bias.copy_(bi)
    w, b = lin.weight, lin.bias
    x, c = leaf(xi, x_dtype, DEV), leaf(ci, BF, DEV)
    xr, wr, br, cr = (leaf(t, F64) for t in (xi, wi, bi, ci))

    with torch.autocast("cuda", dtype=BF, enabled=w_dtype == F32):
        out = lin(x)
    ref = xr @ wr.t() + br
    assert out.dtype == BF and same(out, ref)
    # the HIP route, not the library fallback, produced `out`
    assert type(out.grad_fn).__name__ in ("_MFMALinearFnBackward",
                                          "_GemvLinearFnBackward")

    gx, gw, gb = torch.autograd.grad(out, (x, w, b), grad_outputs=c,
                                     create_graph=True)
    gxr, gwr, gbr = torch.autograd.grad(ref, (xr, wr, br),
                                        grad_outputs=cr,
                                        create_graph=True)
    assert same(gx, gxr), "d out / d x"
    assert same(gw, gwr), "d out / d weight"
    assert same(gb, gbr, store=w_dtype), "d out / d bias"

    assert gx.requires_grad, "gx is a constant: weight term dropped"
    gw2, gc = torch.autograd.grad(
        gx, (w, c), grad_outputs=c2i.to(DEV, gx.dtype),
        retain_graph=True)
    gw2r, gcr = torch.autograd.grad(gxr, (wr, cr), grad_outputs=c2i)
    assert same(gw2, gw2r), "d gx / d weight"
    assert same(gc, gcr), "d gx / d cotangent"

    gx2, gc2 = torch.autograd.grad(
        gw, (x, c), grad_outputs=c3i.to(DEV, gw.dtype))
    gx2r, gc2r = torch.autograd.grad(gwr, (xr, cr), grad_outputs=c3i)
    assert same(gx2, gx2r), "d gw / d x"
    assert same(gc2, gc2r), "d gw / d cotangent"


@pytest.mark.parametrize("c_in,c_out,lmax", [(32, 64, 1), (64, 128, 3),
                                             (96, 64, 2), (64, 64, 2)])
def test_irreps_linear_module_closure(c_in, c_out, lmax):
    """`IrrepsLinear` (bf16, bias and fused residual) forward and both
    gradient orders; three of the shapes leave the kernels on one
    backward route, the fourth is the flagship's all-kernel shape."""
    from hydragnn_amd.models.mace.o3 import IrrepsLinear
    from hydragnn_amd.ops.irreps_linear import irreps_linear_eligible
    n, d, n_l = 100, (lmax + 1) ** 2, lmax + 1
    lmap = lmap_for(lmax)
    gen = _gen(c_in, c_out, lmax)
    xi = ints(gen, -4, 4, n, c_in, d)
    Wi = ints(gen, -4, 4, n_l, c_in, c_out)
    bi = ints(gen, -8, 8, c_out)
    ai = ints(gen, -8, 8, n, c_out, d)
    ci = ints(gen, -4, 4, n, c_out, d)
    c2i = ints(gen, -4, 4, n, c_in, d)
    c3i = ints(gen, -4, 4, n_l, c_in, c_out)
    if not (gw_envelope(c_in, c_out, d, n_l)
            and fwd_envelope(c_out, c_in, d, n_l)):
        ci = sparse_rows(ci, torch.tensor([0, 33, 66, 99]))
        assert fold_exact(xi, ci, lmap)
        assert fold_exact(c2i, ci, lmap)

    lin = IrrepsLinear(c_in, c_out, lmax, bias=True).to(DEV, BF)
    with torch.no_grad():
        lin.weight.copy_(Wi)
        lin.bias.copy_(bi)
    W, b = lin.weight, lin.bias
    x, a, c = (leaf(t, BF, DEV) for t in (xi, ai, ci))
    xr, Wr, br, ar, cr = (leaf(t, F64) for t in (xi, Wi, bi, ai, ci))

    assert irreps_linear_eligible(x, W)
    out = lin(x, add=a)
    ref = irreps_formula(xr, Wr, lmap, br, ar)
    assert same(out, ref)
    assert type(out.grad_fn).__name__ == "_IrrepsLinearFnBackward"

    gx, gW, gb, ga = torch.autograd.grad(out, (x, W, b, a),
                                         grad_outputs=c,
                                         create_graph=True)
    gxr, gWr, gbr, gar = torch.autograd.grad(ref, (xr, Wr, br, ar),
                                             grad_outputs=cr,
                                             create_graph=True)
    assert same(gx, gxr), "d out / d x"
    assert same(gW, gWr), "d out / d W"
    assert same(gb, gbr), "d out / d bias"
    assert same(ga, gar), "d out / d add"

    gW2, gc = torch.autograd.grad(gx, (W, c),
                                  grad_outputs=c2i.to(DEV, BF),
                                  retain_graph=True)
    gW2r, gcr = torch.autograd.grad(gxr, (Wr, cr), grad_outputs=c2i)
    assert same(gW2, gW2r), "d gX / d W"
    assert same(gc, gcr), "d gX / d cotangent"

    gx2, gc2 = torch.autograd.grad(gW, (x, c),
                                   grad_outputs=c3i.to(DEV, BF))
    gx2r, gc2r = torch.autograd.grad(gWr, (xr, cr), grad_outputs=c3i)
    assert same(gx2, gx2r), "d gW / d x"
    assert same(gc2, gc2r), "d gW / d cotangent"
