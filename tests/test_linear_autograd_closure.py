"""Autograd closure of the bf16 linear family, without a GPU.

`get_extension` is replaced by a pure-torch double of the four entry
points (`mfma_linear`, `gemv_small_n`, `irreps_linear`,
`irreps_linear_gw`).  The double computes in fp64, stores bf16 (fp32
partials for the weight gradient) and raises for exactly the shapes the
C++ host checks reject, so a backward that re-enters a kernel outside
its envelope fails here as it would on the device.

All operands and cotangents are small integers: every product and every
partial sum is an exactly representable integer, so each result is
known bit for bit up to the one round-to-nearest-even store to bf16.
Gradients are taken with cotangents (never a loss on a kernel output),
so no rounded output feeds another product, and every comparison is
`torch.equal` against fp64 autograd on the plain formula after the same
final cast.

Where a route sums in bf16 more than once (the split-K weight gradient
when it splits, the bmm + fold weight-gradient fallback of the irreps
linear, and autograd's own fold of a gathered weight), the cotangent is
made sparse enough that every intermediate is an integer of magnitude
<= 256, which bf16 holds exactly; the test asserts that on the
reference.  No test here uses an error bound.
"""

import functools
import importlib

import pytest
import torch

from _exact_linear import (
    BF, F32, F64, fold_exact, fwd_envelope, gw_envelope, ints,
    irreps_formula, leaf, lmap_for, same, sparse_rows,
    splitk_partials_exact,
)

# (`hydragnn_amd.ops.irreps_linear` the attribute is the function)
ml = importlib.import_module("hydragnn_amd.ops.mfma_linear")
il = importlib.import_module("hydragnn_amd.ops.irreps_linear")


def _check(cond, msg):
    if not cond:
        raise RuntimeError(msg)


class _ExtDouble:
    """fp64 stand-in for `_hip_ops` on CPU tensors.  Like the compiled
    entry points it records no autograd graph."""

    @staticmethod
    def _bf16_contig(*ts):
        for t in ts:
            _check(t.dtype == BF and t.is_contiguous(),
                   "operand must be contiguous bf16")

    @torch.no_grad()
    def mfma_linear(self, A, B, bias, trans_b):
        self._bf16_contig(A, B)
        K = A.shape[1]
        N, Kb = (B.shape[0], B.shape[1]) if trans_b else \
            (B.shape[1], B.shape[0])
        _check(K == Kb, "inner dims mismatch")
        _check(K % 32 == 0 and N % 64 == 0,
               "mfma_linear needs K % 32 == 0 and N % 64 == 0")
        out = A.to(F64) @ (B.to(F64).t() if trans_b else B.to(F64))
        if bias is not None:
            out = out + bias.to(F32).to(F64)
        return out.to(BF)

    @torch.no_grad()
    def gemv_small_n(self, A, W, bias):
        self._bf16_contig(A, W)
        _check(W.shape[1] == A.shape[1], "inner dims mismatch")
        _check(1 <= W.shape[0] <= 8, "gemv_small_n needs 1 <= N <= 8")
        _check(A.shape[1] % 8 == 0, "gemv_small_n needs K % 8 == 0")
        out = A.to(F64) @ W.to(F64).t()
        if bias is not None:
            out = out + bias.to(F32).to(F64)
        return out.to(BF)

    @torch.no_grad()
    def irreps_linear(self, X, W, lmap, bias, trans_w, add):
        self._bf16_contig(X, W)
        n_l = W.shape[0]
        c_in, d = X.shape[1], X.shape[2]
        c_out, c_w = (W.shape[1], W.shape[2]) if trans_w else \
            (W.shape[2], W.shape[1])
        _check(c_in == c_w, "channel mismatch")
        _check(lmap.numel() == d, "lmap length")
        _check(fwd_envelope(c_in, c_out, d, n_l),
               "irreps_linear shape envelope / LDS budget")
        Wk = (W.transpose(1, 2) if trans_w else W).to(F64)
        out = torch.einsum("nim,mio->nom", X.to(F64), Wk[lmap])
        if bias is not None:
            out[:, :, 0] += bias.to(F32).to(F64)
        if add is not None:
            _check(add.shape == out.shape and add.dtype == BF,
                   "irreps_linear residual shape/dtype mismatch")
            out = out + add.to(F64)
        return out.to(BF)

    @torch.no_grad()
    def irreps_linear_gw(self, X, G, lmap, n_l, nblocks):
        self._bf16_contig(X, G)
        n, c_in, d = X.shape
        c_out = G.shape[1]
        _check(G.shape[0] == n and G.shape[2] == d, "row/D mismatch")
        _check(gw_envelope(c_in, c_out, d, n_l),
               "irreps_linear_gw shape envelope / LDS budget")
        parts = torch.zeros(nblocks, n_l, c_in, c_out, dtype=F64)
        # 32-row tiles strided over the persistent blocks
        block = (torch.arange(n) // 32) % nblocks
        for b in range(nblocks):
            sel = block == b
            if sel.any():
                gw_m = torch.bmm(X[sel].to(F64).permute(2, 1, 0),
                                 G[sel].to(F64).permute(2, 0, 1))
                parts[b].index_add_(0, lmap, gw_m)
        return parts.to(F32)


@pytest.fixture(autouse=True)
def _double(monkeypatch):
    ext = _ExtDouble()
    for mod in (ml, il):
        monkeypatch.setattr(mod, "get_extension",
                            lambda required=False: ext)


# ---------------------------------------------------------------------------
# MFMA and GEMV linears
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [300, 600])
@pytest.mark.parametrize("n_in", [64, 128])
@pytest.mark.parametrize("n_out", [1, 4, 64, 128])
@pytest.mark.parametrize("w_dtype,x_dtype", [(F32, BF), (F32, F32),
                                             (BF, BF)],
                         ids=["w32-xbf", "w32-x32", "wbf-xbf"])
def test_linear_closure(w_dtype, x_dtype, n_out, n_in, rows):
    """First and second order of the MFMA (n_out >= 64) and GEMV
    (n_out <= 8) linears; fp32 leaves are the `precision: bf16`
    autocast case.

    Rounding: with 300 rows the split-K factor is 1, every result is
    one fp32-accumulated product stored to bf16 once -> dense
    cotangent, exact.  With 600 rows the factor is 2 (on the device);
    the cotangent is nonzero on 16 rows only, so each chunk's weight
    gradient and their sum stay <= 256 (asserted) -> exact as well."""
    gen = torch.Generator().manual_seed(1000 * n_out + n_in + rows)
    entry = ml.mfma_linear_bf16 if n_out >= 64 else ml.gemv_linear_bf16
    xi = ints(gen, -4, 4, rows, n_in)
    wi = ints(gen, -4, 4, n_out, n_in)
    bi = ints(gen, -8, 8, n_out)
    ci = ints(gen, -4, 4, rows, n_out)      # cotangent of out
    c2i = ints(gen, -4, 4, rows, n_in)      # cotangent of gx
    c3i = ints(gen, -4, 4, n_out, n_in)     # cotangent of gw
    if rows >= 512:
        ci = sparse_rows(ci, torch.arange(16) * (rows // 16) + 3)
        assert splitk_partials_exact(ci, xi)
        assert splitk_partials_exact(ci, c2i)

    x, w, b = leaf(xi, x_dtype), leaf(wi, w_dtype), leaf(bi, w_dtype)
    c = leaf(ci, BF)
    xr, wr, br, cr = (leaf(t, F64) for t in (xi, wi, bi, ci))

    out = entry(x, w, b)
    ref = xr @ wr.t() + br
    assert out.dtype == BF and same(out, ref)

    gx, gw, gb = torch.autograd.grad(out, (x, w, b), grad_outputs=c,
                                     create_graph=True)
    gxr, gwr, gbr = torch.autograd.grad(ref, (xr, wr, br),
                                        grad_outputs=cr,
                                        create_graph=True)
    assert gx.dtype == x_dtype and gw.dtype == w_dtype
    assert same(gx, gxr), "d out / d x"
    assert same(gw, gwr), "d out / d weight"
    # the bias gradient is an fp32 column sum, stored in the bias dtype
    assert same(gb, gbr, store=w_dtype), "d out / d bias"

    # second order through gx: the weight term of the force loss
    assert gx.requires_grad, "gx is a constant: weight term dropped"
    gw2, gc = torch.autograd.grad(gx, (w, c),
                                  grad_outputs=c2i.to(gx.dtype),
                                  retain_graph=True)
    gw2r, gcr = torch.autograd.grad(gxr, (wr, cr), grad_outputs=c2i)
    assert same(gw2, gw2r), "d gx / d weight"
    assert same(gc, gcr), "d gx / d cotangent"

    # second order through gw
    assert gw.requires_grad, "gw is a constant"
    gx2, gc2 = torch.autograd.grad(gw, (x, c),
                                   grad_outputs=c3i.to(gw.dtype))
    gx2r, gc2r = torch.autograd.grad(gwr, (xr, cr), grad_outputs=c3i)
    assert same(gx2, gx2r), "d gw / d x"
    assert same(gc2, gc2r), "d gw / d cotangent"


# ---------------------------------------------------------------------------
# Irreps linear
# ---------------------------------------------------------------------------
_N = 100
_IRREPS_SHAPES = [
    (ci, co, lmax)
    for ci in (32, 64, 96, 128) for co in (64, 128, 192, 256)
    for lmax in range(4)
    if il.irreps_kernel_ok(_N, ci, co, (lmax + 1) ** 2, lmax + 1)]


@functools.lru_cache(maxsize=None)
def _irreps_case(c_in, c_out, lmax):
    """Forward and first order on the Function under test and on fp64
    autograd, shared by the tests below (graphs kept)."""
    d, n_l = (lmax + 1) ** 2, lmax + 1
    lmap = lmap_for(lmax)
    gen = torch.Generator().manual_seed(7919 * c_in + 31 * c_out + lmax)
    t = dict(x=ints(gen, -4, 4, _N, c_in, d),
             W=ints(gen, -4, 4, n_l, c_in, c_out),
             bias=ints(gen, -8, 8, c_out),
             add=ints(gen, -8, 8, _N, c_out, d),
             c=ints(gen, -4, 4, _N, c_out, d),
             c2=ints(gen, -4, 4, _N, c_in, d),
             c3=ints(gen, -4, 4, n_l, c_in, c_out))
    # dense cotangent only where every weight-gradient-like sum runs in
    # fp32 on a kernel; otherwise (bf16 bmm + fold) four nonzero rows,
    # one per 32-row tile, keep every intermediate <= 256
    dense = (gw_envelope(c_in, c_out, d, n_l)
             and fwd_envelope(c_out, c_in, d, n_l))
    if not dense:
        t["c"] = sparse_rows(t["c"], torch.tensor([0, 33, 66, 99]))
        assert fold_exact(t["x"], t["c"], lmap)
        assert fold_exact(t["c2"], t["c"], lmap)
    got = {k: leaf(t[k], F32 if k == "bias" else BF)
           for k in ("x", "W", "bias", "add", "c")}
    ref = {k: leaf(t[k], F64) for k in ("x", "W", "bias", "add", "c")}
    names = ("x", "W", "bias", "add")
    got["out"] = il.irreps_linear(got["x"], got["W"], lmap, got["bias"],
                                  add=got["add"])
    ref["out"] = irreps_formula(ref["x"], ref["W"], lmap, ref["bias"],
                                 ref["add"])
    for side in (got, ref):
        grads = torch.autograd.grad(
            side["out"], [side[k] for k in names],
            grad_outputs=side["c"], create_graph=True)
        side.update({"g" + k: g for k, g in zip(names, grads)})
    return t, got, ref


_irreps_ids = [f"{ci}-{co}-l{l}" for ci, co, l in _IRREPS_SHAPES]


@pytest.mark.parametrize("c_in,c_out,lmax", _IRREPS_SHAPES,
                         ids=_irreps_ids)
def test_irreps_forward_and_first_order(c_in, c_out, lmax):
    _, got, ref = _irreps_case(c_in, c_out, lmax)
    assert same(got["out"], ref["out"]), "forward (bias + add)"
    assert same(got["gx"], ref["gx"]), "d out / d x"
    assert same(got["gW"], ref["gW"]), "d out / d W"
    assert got["gbias"].dtype == F32
    assert same(got["gbias"], ref["gbias"]), "d out / d bias"
    assert same(got["gadd"], ref["gadd"]), "d out / d add"


@pytest.mark.parametrize("c_in,c_out,lmax", _IRREPS_SHAPES,
                         ids=_irreps_ids)
def test_irreps_second_order_through_gx(c_in, c_out, lmax):
    """d(gX)/dW — the term the force loss needs — and d(gX)/dc."""
    t, got, ref = _irreps_case(c_in, c_out, lmax)
    assert got["gx"].requires_grad, "gX is a constant"
    gW2, gc = torch.autograd.grad(got["gx"], (got["W"], got["c"]),
                                  grad_outputs=t["c2"].to(BF),
                                  retain_graph=True)
    gW2r, gcr = torch.autograd.grad(ref["gx"], (ref["W"], ref["c"]),
                                    grad_outputs=t["c2"],
                                    retain_graph=True)
    assert same(gW2, gW2r), "d gX / d W"
    assert same(gc, gcr), "d gX / d cotangent"


@pytest.mark.parametrize("c_in,c_out,lmax", _IRREPS_SHAPES,
                         ids=_irreps_ids)
def test_irreps_second_order_through_gw(c_in, c_out, lmax):
    """d(gW)/dx and d(gW)/dc: gW is bilinear in (x, c)."""
    t, got, ref = _irreps_case(c_in, c_out, lmax)
    assert got["gW"].requires_grad, "gW is a constant"
    gx2, gc2 = torch.autograd.grad(got["gW"], (got["x"], got["c"]),
                                   grad_outputs=t["c3"].to(BF),
                                   retain_graph=True)
    gx2r, gc2r = torch.autograd.grad(ref["gW"], (ref["x"], ref["c"]),
                                     grad_outputs=t["c3"],
                                     retain_graph=True)
    assert same(gx2, gx2r), "d gW / d x"
    assert same(gc2, gc2r), "d gW / d cotangent"


# ---------------------------------------------------------------------------
# Shape-only sweep: backward's routes stay inside the host envelopes
# ---------------------------------------------------------------------------
_SWEEP = [(ci, co, lmax)
          for ci in (32, 64, 96, 128, 160, 192, 256)
          for co in (64, 128, 192, 256) for lmax in range(4)]


def _mix_node(c_in, c_out, d, n_l, depth, bad):
    """A forward-map call [*, c_in, d] -> c_out as backward routes it:
    on the kernel (then inside its envelope, and so must its own
    backward be) or on the torch composition (autograd's, closed)."""
    if not il.irreps_fwd_kernel_ok(c_in, c_out, d, n_l):
        return
    if not fwd_envelope(c_in, c_out, d, n_l):
        bad.append(("irreps_linear", c_in, c_out, d, n_l))
    if depth:
        _mix_node(c_out, c_in, d, n_l, depth - 1, bad)        # gX
        _gw_node(c_in, c_out, d, n_l, depth - 1, bad)         # gW


def _gw_node(c_in, c_out, d, n_l, depth, bad):
    if not il.irreps_gw_kernel_ok(c_in, c_out, d, n_l):
        return
    if not gw_envelope(c_in, c_out, d, n_l):
        bad.append(("irreps_linear_gw", c_in, c_out, d, n_l))
    if depth:
        _mix_node(c_out, c_in, d, n_l, depth - 1, bad)        # d/dx
        _mix_node(c_in, c_out, d, n_l, depth - 1, bad)        # d/dg


@pytest.mark.parametrize("c_in,c_out,lmax", _SWEEP)
def test_irreps_routes_inside_envelopes(c_in, c_out, lmax):
    d, n_l = (lmax + 1) ** 2, lmax + 1
    # the gates agree with the C++ checks in both directions, so a
    # kernel is used wherever it can be
    assert il.irreps_fwd_kernel_ok(c_in, c_out, d, n_l) == \
        fwd_envelope(c_in, c_out, d, n_l)
    assert il.irreps_gw_kernel_ok(c_in, c_out, d, n_l) == \
        gw_envelope(c_in, c_out, d, n_l)
    assert il.irreps_kernel_ok(_N, c_in, c_out, d, n_l) == \
        fwd_envelope(c_in, c_out, d, n_l)
    bad = []
    _mix_node(c_in, c_out, d, n_l, 2, bad)
    assert not bad, f"routed to a kernel outside its envelope: {bad}"


def test_no_accepted_shape_needs_the_static_lds():
    """The kernels hold a static 64 B table besides the dynamic LDS the
    host sizes: an accepted shape must leave room for it."""
    for c_in in range(16, 513, 16):
        for c_out in range(16, 513, 16):
            for lmax in range(4):
                d, n_l = (lmax + 1) ** 2, lmax + 1
                if il.irreps_fwd_kernel_ok(c_in, c_out, d, n_l):
                    lds = (d * 32 * (c_in + 8)
                           + n_l * c_in * (c_out + 8)) * 2
                    assert lds + 64 <= 160 * 1024, (c_in, c_out, lmax)
                if il.irreps_gw_kernel_ok(c_in, c_out, d, n_l):
                    lds = d * 32 * (c_in + c_out + 16) * 2
                    assert lds + 64 <= 160 * 1024, (c_in, c_out, lmax)
