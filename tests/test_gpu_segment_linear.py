"""The segment linear-attention kernels of `csrc/segment_linear.hip`
(`seglin_outer_kernel`, `seglin_zsum_kernel`, `seglin_matvec_kernel`),
the autograd pair of `ops/segment_linear.py` and the Performer route of
`HydraGPSConv` on the device.

Exact checks use integer operands in [-2, 2]: every partial sum is an
integer far below 2^24, exact in fp32 in any order, so the fp64
reference (rounded once to the row dtype for row outputs) is the only
right answer and the comparison is `torch.equal`.  Checks on general
values carry a bound computed in the test from the reference of
absolute values: n_addends * u * sum|addend| per element, u the
accumulator's unit roundoff, plus one ulp of the output dtype where the
output is rounded to the row dtype.

Segment sizes come from `segment_linear_tiling`: one row, an empty
graph, both sides of the outer sum's row tile R, one row more than a
matvec pass Bw, and more than two tiles.
"""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

from hydragnn_amd.globalatt.gps import HydraGPSConv  # noqa: E402
from hydragnn_amd.ops import (  # noqa: E402
    get_extension, segment_matvec, segment_outer_sum)
from hydragnn_amd.ops.segment_linear import (  # noqa: E402
    acc_dtype, segment_linear_ok, segment_linear_stats,
    segment_linear_tiling, torch_segment_matvec, torch_segment_outer_sum)

DEV = "cuda"
H = 3
WIDTHS = [(1, 1), (3, 5), (64, 17), (64, 129), (128, 132)]
DTYPES = [torch.float32, torch.bfloat16, torch.float64]
U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}


def _ext():
    return get_extension(required=True)


def _sizes(a, b, dtype):
    R, Bw = segment_linear_tiling(a, b, dtype)
    return [1, 0, R - 1, R, R + 1, Bw + 1, 2 * R + 3]


def _segments(sizes):
    """(ptr, batch) on the CPU."""
    sizes = torch.tensor(sizes, dtype=torch.long)
    ptr = torch.zeros(len(sizes) + 1, dtype=torch.long)
    ptr[1:] = sizes.cumsum(0)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), sizes)
    return ptr, batch


def _ints(n, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, (n, H, w), generator=g).double()


def _normal(n, w, seed, dtype):
    """Unit-normal rows, rounded to `dtype` and kept as fp64."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, H, w, dtype=torch.float64, generator=g)
    return x.to(dtype).double()


def _counts():
    return dict(segment_linear_stats)


def _delta(before):
    return {k: segment_linear_stats[k] - before[k] for k in before}


# ---------------------------------------------------------------- exact

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("a,b", WIDTHS)
def test_exact_integers(a, b, dtype):
    assert segment_linear_ok(a, b, torch.empty(0, device=DEV, dtype=dtype))
    ptr, batch = _segments(_sizes(a, b, dtype))
    n = int(ptr[-1])
    A, B = _ints(n, a, 1), _ints(n, b, 2)
    K_ref = torch_segment_outer_sum(A, B, ptr, batch)
    dptr, dbatch = ptr.to(DEV), batch.to(DEV)
    before = _counts()
    K = segment_outer_sum(A.to(DEV, dtype), B.to(DEV, dtype), dptr, dbatch)
    assert K.dtype == acc_dtype(dtype)
    assert torch.equal(K.double().cpu(), K_ref)
    Kd = K_ref.to(DEV, acc_dtype(dtype))
    for trans, X in ((False, A), (True, B)):
        O = segment_matvec(X.to(DEV, dtype), Kd, dptr, dbatch, trans)
        O_ref = torch_segment_matvec(X, K_ref, ptr, batch, trans)
        assert O.dtype == dtype
        assert torch.equal(O.cpu(), O_ref.to(dtype))
    assert _delta(before) == {"outer": 1, "matvec": 2, "torch_outer": 0,
                              "torch_matvec": 0}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("a,b", [(3, 5), (64, 17), (128, 132)])
def test_row_split_does_not_matter_where_sums_are_exact(a, b, dtype):
    """z = 5 is more than the row tiles of any segment here, so some
    workgroups have no rows and write zero partials."""
    ptr, batch = _segments(_sizes(a, b, dtype))
    n = int(ptr[-1])
    A, B = _ints(n, a, 3), _ints(n, b, 4)
    K_ref = torch_segment_outer_sum(A, B, ptr, batch)
    dA, dB = A.to(DEV, dtype), B.to(DEV, dtype)
    dptr, dbatch = ptr.to(DEV), batch.to(DEV)
    Ks = [segment_outer_sum(dA, dB, dptr, dbatch, z=z) for z in (1, 2, 5)]
    for K in Ks:
        assert torch.equal(K, Ks[0])
        assert torch.equal(K.double().cpu(), K_ref)


# ---------------------------------------------------------- fixed order

@pytest.mark.parametrize("a,b", [(3, 5), (64, 17)])
def test_same_split_same_bits(a, b):
    ptr, batch = _segments(_sizes(a, b, torch.float32))
    n = int(ptr[-1])
    dA = _normal(n, a, 5, torch.float32).to(DEV, torch.float32)
    dB = _normal(n, b, 6, torch.float32).to(DEV, torch.float32)
    dptr, dbatch = ptr.to(DEV), batch.to(DEV)
    for z in (None, 1, 3):
        K1 = segment_outer_sum(dA, dB, dptr, dbatch, z=z)
        K2 = segment_outer_sum(dA, dB, dptr, dbatch, z=z)
        assert torch.equal(K1, K2)
    K = segment_outer_sum(dA, dB, dptr, dbatch)
    for trans, X in ((False, dA), (True, dB)):
        O1 = segment_matvec(X, K, dptr, dbatch, trans)
        O2 = segment_matvec(X, K, dptr, dbatch, trans)
        assert torch.equal(O1, O2)


@pytest.mark.parametrize("a,b", [(3, 5), (64, 17)])
def test_unsplit_sum_is_the_ascending_row_sum(a, b):
    """With z = 1 a thread adds its element's products row by row in
    ascending order.  The operands are random fp32 numbers with 8
    significant bits (bf16-representable), so a product is exact in fp32
    and the kernel's fused multiply-add performs the same IEEE addition
    as the separate multiply and add of the CPU loop; the sums
    themselves round at every step."""
    ptr, batch = _segments(_sizes(a, b, torch.float32))
    n = int(ptr[-1])
    A = _normal(n, a, 7, torch.bfloat16).float()
    B = _normal(n, b, 8, torch.bfloat16).float()
    K_ref = torch.zeros(ptr.numel() - 1, H, a, b)
    for g in range(ptr.numel() - 1):
        for i in range(int(ptr[g]), int(ptr[g + 1])):
            K_ref[g] = K_ref[g] + A[i, :, :, None] * B[i, :, None, :]
    K = segment_outer_sum(A.to(DEV), B.to(DEV), ptr.to(DEV), batch.to(DEV),
                          z=1)
    assert torch.equal(K.cpu(), K_ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_matvec_row_does_not_depend_on_row_distribution(dtype):
    """The same rows and the same matrix for every graph, once as one
    graph and once cut into the boundary sizes: the same bits."""
    a, b = 64, 17
    sizes = _sizes(a, b, dtype)
    n = sum(sizes)
    acc = acc_dtype(dtype)
    X = _normal(n, a, 17, dtype).to(DEV, dtype)
    g = torch.Generator().manual_seed(18)
    Km = torch.randn(1, H, a, b, generator=g).to(DEV, acc)
    outs = []
    for sz in ([n], sizes):
        ptr, batch = _segments(sz)
        K = Km.expand(len(sz), H, a, b).contiguous()
        outs.append(segment_matvec(X, K, ptr.to(DEV), batch.to(DEV)))
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------- general values

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("a,b", WIDTHS)
def test_general_values_within_derived_bound(a, b, dtype):
    """Outer sum: n = rows of the segment addends per element, no final
    rounding (the matrix stays in the accumulator type).  Matvec: n =
    input width addends, then one rounding to the row dtype."""
    acc = acc_dtype(dtype)
    u = U[acc]
    sizes = _sizes(a, b, dtype)
    ptr, batch = _segments(sizes)
    n = int(ptr[-1])
    A, B = _normal(n, a, 9, dtype), _normal(n, b, 10, dtype)
    dptr, dbatch = ptr.to(DEV), batch.to(DEV)
    K_ref = torch_segment_outer_sum(A, B, ptr, batch)
    K_abs = torch_segment_outer_sum(A.abs(), B.abs(), ptr, batch)
    rows = torch.tensor(sizes, dtype=torch.float64).view(-1, 1, 1, 1)
    for z in (None, 2):
        K = segment_outer_sum(A.to(DEV, dtype), B.to(DEV, dtype), dptr,
                              dbatch, z=z)
        err = (K.double().cpu() - K_ref).abs()
        assert bool((err <= rows * u * K_abs).all()), \
            f"outer z={z}: worst excess {(err - rows * u * K_abs).max()}"

    g = torch.Generator().manual_seed(11)
    Km = torch.randn(len(sizes), H, a, b, dtype=torch.float64,
                     generator=g).to(acc).double()
    eps = torch.finfo(dtype).eps
    for trans, X in ((False, A), (True, B)):
        O = segment_matvec(X.to(DEV, dtype), Km.to(DEV, acc), dptr, dbatch,
                           trans)
        O_ref = torch_segment_matvec(X, Km, ptr, batch, trans)
        O_abs = torch_segment_matvec(X.abs(), Km.abs(), ptr, batch, trans)
        bound = X.shape[2] * u * O_abs + eps * O_ref.abs()
        err = (O.double().cpu() - O_ref).abs()
        assert bool((err <= bound).all()), \
            f"matvec trans={trans}: worst excess {(err - bound).max()}"


# ------------------------------------------------------------- autograd

def _attention(fq, fk, v1, ptr, batch, outer, matvec):
    return matvec(fq, outer(fk, v1, ptr, batch), ptr, batch)


def _two_orders(fq, fk, v1, W, T, ptr, batch, outer, matvec):
    """First-order gradients of <W, O> and the gradients of
    <T, first order> with respect to everything."""
    O = _attention(fq, fk, v1, ptr, batch, outer, matvec)
    first = torch.autograd.grad((O * W).sum(), (fq, fk, v1),
                                create_graph=True)
    second = torch.autograd.grad(
        sum((f * t).sum() for f, t in zip(first, T)), (fq, fk, v1))
    return (O,) + first + second


def test_first_and_second_order_stay_on_the_kernels():
    """fp64 rows.  O, its gradients and their gradients are multilinear
    in (phi q, phi k, [v 1], W, T) with coefficients 0 or 1, so the same
    derivative evaluated at the operands' absolute values is sum|addend|
    of its fully expanded sum, which has at most n_g * a * b addends per
    element: the bound is n_g * a * b * u * that value."""
    a, b = 64, 17
    sizes = _sizes(a, b, torch.float64)
    ptr, batch = _segments(sizes)
    dptr, dbatch = ptr.to(DEV), batch.to(DEV)
    n = int(ptr[-1])
    g = torch.Generator().manual_seed(12)

    def rnd(*shape):
        return torch.randn(*shape, dtype=torch.float64, generator=g)

    fq, fk = rnd(n, H, a).abs() + 0.1, rnd(n, H, a).abs() + 0.1
    v1 = torch.cat([rnd(n, H, b - 1), torch.ones(n, H, 1,
                                                 dtype=torch.float64)], -1)
    W = rnd(n, H, b)
    T = (rnd(n, H, a), rnd(n, H, a), rnd(n, H, b))

    def leaves(ts, dev, absolute=False):
        return [(t.abs() if absolute else t).to(dev).requires_grad_(True)
                for t in ts]

    before = _counts()
    got = _two_orders(*leaves((fq, fk, v1), DEV), W.to(DEV),
                      [t.to(DEV) for t in T], dptr, dbatch,
                      segment_outer_sum, segment_matvec)
    d = _delta(before)
    # forward 1 + 1; first order: the matvec's backward is one matvec
    # and one outer sum, the outer sum's is two matvecs; the second
    # order differentiates those again.  None may reach the torch form.
    assert d["torch_outer"] == 0 and d["torch_matvec"] == 0
    assert d["outer"] >= 3 and d["matvec"] >= 6

    outer_t = lambda A, B, p, bt: torch_segment_outer_sum(A, B, p, bt)  # noqa: E731,E501
    matvec_t = lambda A, K, p, bt: torch_segment_matvec(A, K, p, bt)  # noqa: E731,E501
    ref = _two_orders(*leaves((fq, fk, v1), "cpu"), W, list(T), ptr, batch,
                      outer_t, matvec_t)
    mag = _two_orders(*leaves((fq, fk, v1), "cpu", True), W.abs(),
                      [t.abs() for t in T], ptr, batch, outer_t, matvec_t)
    n_add = max(sizes) * a * b
    names = ("O", "dq", "dk", "dv", "ddq", "ddk", "ddv")
    for name, x, r, m in zip(names, got, ref, mag):
        err = (x.detach().cpu() - r.detach()).abs()
        bound = n_add * U[torch.float64] * m.detach()
        assert bool((err <= bound).all()), \
            f"{name}: worst excess {(err - bound).max()}"


def test_first_order_backward_calls_are_the_other_primitive():
    a, b = 3, 5
    ptr, batch = _segments(_sizes(a, b, torch.float32))
    dptr, dbatch = ptr.to(DEV), batch.to(DEV)
    n = int(ptr[-1])
    A = _ints(n, a, 13).to(DEV, torch.float32).requires_grad_(True)
    B = _ints(n, b, 14).to(DEV, torch.float32).requires_grad_(True)
    K = segment_outer_sum(A, B, dptr, dbatch)
    before = _counts()
    K.sum().backward()
    assert _delta(before) == {"outer": 0, "matvec": 2, "torch_outer": 0,
                              "torch_matvec": 0}
    Kl = K.detach().requires_grad_(True)
    O = segment_matvec(A.detach().requires_grad_(True), Kl, dptr, dbatch)
    before = _counts()
    O.sum().backward()
    assert _delta(before) == {"outer": 1, "matvec": 1, "torch_outer": 0,
                              "torch_matvec": 0}


# --------------------------------------------------- envelope and edges

@pytest.mark.parametrize("a,b", [(129, 5), (3, 133)])
def test_outside_the_envelope_takes_the_torch_form(a, b):
    ptr, batch = _segments([1, 0, 33, 17])
    n = int(ptr[-1])
    A, B = _ints(n, a, 15), _ints(n, b, 16)
    dA, dB = A.to(DEV, torch.float32), B.to(DEV, torch.float32)
    dptr, dbatch = ptr.to(DEV), batch.to(DEV)
    assert not segment_linear_ok(a, b, dA)
    K_ref = torch_segment_outer_sum(A, B, ptr, batch)
    before = _counts()
    K = segment_outer_sum(dA, dB, dptr, dbatch)
    O = segment_matvec(dA, K, dptr, dbatch)
    assert _delta(before) == {"outer": 0, "matvec": 0, "torch_outer": 1,
                              "torch_matvec": 1}
    assert torch.equal(K.double().cpu(), K_ref)
    assert torch.equal(O.double().cpu(),
                       torch_segment_matvec(A, K_ref, ptr, batch))
    with pytest.raises(RuntimeError, match="envelope"):
        _ext().segment_outer_sum(dA, dB, dptr)
    with pytest.raises(RuntimeError, match="envelope"):
        _ext().segment_matvec(dA, K, dptr)


def test_raw_entry_points_check_their_operands():
    ptr, _ = _segments([2, 3])
    dptr = ptr.to(DEV)
    A = torch.zeros(5, H, 3, device=DEV)
    B = torch.zeros(5, H, 5, device=DEV)
    K = torch.zeros(2, H, 3, 5, device=DEV)
    with pytest.raises(RuntimeError):
        _ext().segment_outer_sum(A, B.double(), dptr)
    with pytest.raises(RuntimeError):      # matrix not in the acc type
        _ext().segment_matvec(A.bfloat16(), K.bfloat16(), dptr)
    with pytest.raises(RuntimeError):      # width of the other side
        _ext().segment_matvec(A, K, dptr, trans=True)
    with pytest.raises(RuntimeError):
        _ext().segment_outer_sum(A, B, dptr, z=33)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sizes", [[], [0, 0, 0]])
def test_no_rows_and_no_graphs(sizes, dtype):
    ptr, batch = _segments(sizes)
    dptr, dbatch = ptr.to(DEV), batch.to(DEV)
    G = len(sizes)
    A = torch.zeros(0, H, 3, device=DEV, dtype=dtype)
    B = torch.zeros(0, H, 5, device=DEV, dtype=dtype)
    before = _counts()
    K = segment_outer_sum(A, B, dptr, dbatch)
    assert K.shape == (G, H, 3, 5) and K.dtype == acc_dtype(dtype)
    assert torch.count_nonzero(K) == 0
    assert segment_matvec(A, K, dptr, dbatch).shape == (0, H, 5)
    assert segment_matvec(B, K, dptr, dbatch, trans=True).shape == (0, H, 3)
    assert _delta(before)["outer"] == 1 and _delta(before)["matvec"] == 2
    torch.cuda.synchronize()


# --------------------------------------------------------------- module

def _layer_run(layer, x, batch, w, autocast):
    layer.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out, _ = layer(x, None, batch=batch)
    (out.double() * w).sum().backward()
    grads = {k: p.grad.detach().double().cpu()
             for k, p in layer.named_parameters() if p.grad is not None}
    return out.detach().double().cpu(), grads


@pytest.mark.parametrize("autocast", [False, True])
def test_gps_performer_layer_against_fp64_dense(autocast, monkeypatch):
    """HydraGPSConv(performer) on graphs of [1, 0, 40, 130] nodes: the
    segment path and the dense-batch path (HYDRAGNN_VARLEN_PERFORMER=0)
    on the GPU, both measured against the same layer in fp64 on the CPU
    dense path.  The segment path's error may be at most twice the
    dense path's plus one ulp of the compute dtype at the reference's
    magnitude (the factor 2 covers the different summation order).

    Observed on an MI355X: see the "Linear attention" section of
    docs/kernels.md.
    """
    torch.manual_seed(21)
    C, heads = 32, 4
    ptr, batch = _segments([1, 0, 40, 130])
    n = int(ptr[-1])
    layer = HydraGPSConv(C, None, heads=heads, attn_type="performer")
    layer.train()
    x = torch.randn(n, C)
    w = torch.randn(n, C, dtype=torch.float64)

    ref_layer = copy.deepcopy(layer).double()
    ref_layer.zero_grad(set_to_none=True)
    ref_out, _ = ref_layer(x.double(), None, batch=batch)
    (ref_out * w).sum().backward()
    ref_grads = {k: p.grad.detach() for k, p in
                 ref_layer.named_parameters() if p.grad is not None}
    ref_out = ref_out.detach()

    dev_layer = copy.deepcopy(layer).to(DEV)
    dx, dbatch, dw = x.to(DEV), batch.to(DEV), w.to(DEV)

    monkeypatch.delenv("HYDRAGNN_VARLEN_PERFORMER", raising=False)
    before = _counts()
    new_out, new_grads = _layer_run(dev_layer, dx, dbatch, dw, autocast)
    d = _delta(before)
    assert d["outer"] >= 1 and d["matvec"] >= 1
    assert d["torch_outer"] == 0 and d["torch_matvec"] == 0

    monkeypatch.setenv("HYDRAGNN_VARLEN_PERFORMER", "0")
    before = _counts()
    old_out, old_grads = _layer_run(dev_layer, dx, dbatch, dw, autocast)
    assert not any(_delta(before).values())

    eps = torch.finfo(torch.bfloat16 if autocast else torch.float32).eps
    assert set(new_grads) == set(old_grads) == set(ref_grads)
    items = [("out", new_out, old_out, ref_out)] + [
        (k, new_grads[k], old_grads[k], ref_grads[k]) for k in ref_grads]
    failures = []
    for name, new, old, ref in items:
        e_new = (new - ref).abs().max().item()
        e_old = (old - ref).abs().max().item()
        allowed = 2 * e_old + eps * ref.abs().max().item()
        print(f"{'bf16 autocast' if autocast else 'fp32'} {name}: "
              f"segment {e_new:.3e} dense {e_old:.3e} "
              f"allowed {allowed:.3e}")
        if not e_new <= allowed:
            failures.append(name)
    assert not failures, failures
