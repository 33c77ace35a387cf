"""Shared pieces of the tests of the fused PNA aggregation
(test_pna_aggr.py on the CPU doubles, test_gpu_pna_aggr.py on the HIP
kernels): cases, fp64 references that do not go through
`hydragnn_amd.ops`, derived error bounds, and checks that take the op
under test and a device as arguments.

Exact-integer method as in _exact_agg.py: sources are integers in
[-8, 8] and rows hold at most a few hundred entries, so sums, extremes
and (on rows built as pairs m +- d) means and variances are integers
far below 2^24: the fp64 reference rounded once fixes every bit.
"""

import math

import torch

from _exact_agg import (BF, F16, F32, F64, N_SEG, gen, ints, layout, put,
                        ref_mean, ref_minmax, ref_minmax_grad, ref_sum,
                        rowptr_of, same)

STD_EPS = 1e-5
AVG_LIN, AVG_LOG = 3.7, 1.3        # the module's two buffers, any values
ALL_SCALERS = ("identity", "amplification", "attenuation", "linear",
               "inverse_linear")
DEFAULT_AGGS = ("mean", "min", "max", "std")
DEFAULT_SCALERS = ("identity", "amplification", "attenuation", "linear")
LAYOUTS = ("gaps", "one_row", "single", "long")
LONG_LEN = 300
TRAILING = ((1,), (3,), (64,), (4, 3))      # F in {1, 3, 64}, one rank 3


def acc_of(dtype):
    return F64 if dtype == F64 else F32


def unit_roundoff(dtype):
    """u = eps / 2 of a format."""
    return torch.finfo(dtype).eps / 2


def ulp_at(value, dtype):
    """One unit in the last place of `dtype` at |value| (normal range)."""
    value = abs(float(value))
    if value == 0:
        return float(torch.finfo(dtype).tiny)
    return 2.0 ** math.floor(math.log2(value)) * torch.finfo(dtype).eps


# ---------------------------------------------------------------------------
# routes: how a case reaches the op
# ---------------------------------------------------------------------------
def route_case(route, src, index):
    """The case as the route sees it: "sorted" reorders the edges (the
    reference then speaks of the reordered edges), "perm" keeps them."""
    if route == "sorted":
        o = torch.argsort(index, stable=True)
        return src[o], index[o]
    assert route == "perm"
    return src, index


def operands(route, index, n, dev):
    """(rowptr, perm) on `dev` for an index already passed through
    `route_case`."""
    rowptr = put(rowptr_of(index, n), dev)
    perm = None
    if route == "perm":
        perm = put(torch.argsort(index, stable=True), dev)
    return rowptr, perm


def run(ops, route, x, index, n, aggs, scalers, dev):
    """pna_aggregate of the device tensor x; returns (out, scale as
    fetched from the device)."""
    rowptr, perm = operands(route, index, n, dev)
    scale = ops.pna_scale(rowptr, scalers, AVG_LIN, AVG_LOG, x.dtype)
    out = ops.pna_aggregate(x, rowptr, scale, aggs, perm=perm)
    return out, scale.detach().cpu()


# ---------------------------------------------------------------------------
# fp64 references (indexing only)
# ---------------------------------------------------------------------------
def counts_of(index, n):
    return torch.bincount(index, minlength=n)


def ref_var(src, index, n):
    """Centered variance sum (x - mu)^2 / max(n, 1) in fp64."""
    src = src.to(F64)
    mu = ref_mean(src, index, n)
    y = src - mu[index]
    ss = torch.zeros_like(mu).index_add_(0, index, y * y)
    d = counts_of(index, n).clamp(min=1).to(F64)
    return ss / d.view(-1, *([1] * (src.dim() - 1)))


def ref_block(name, src, index, n):
    """One aggregator block [n, F] in fp64, trailing dims flattened."""
    if name == "sum":
        out = ref_sum(src, index, n)
    elif name == "mean":
        out = ref_mean(src, index, n)
    elif name in ("min", "max"):
        out = ref_minmax(src, index, n, name == "max")[0]
    elif name == "var":
        out = ref_var(src, index, n)
    else:
        assert name == "std"
        out = torch.sqrt(ref_var(src, index, n) + STD_EPS)
    return out.reshape(n, -1)


def split_blocks(out, n_scalers, n_aggs):
    """out [N, S*A*F] -> [N, S, A, F]."""
    return out.reshape(out.shape[0], n_scalers, n_aggs, -1)


def ref_differentiable(x, index, n, aggs, scale, arg_min=None, arg_max=None):
    """Plain-torch fp64 forward, differentiable in x: out [N, S*A*F]
    with the given scale [N, S].  min/max pick x at the given args."""
    x = x.reshape(x.shape[0], -1)
    d = counts_of(index, n).clamp(min=1).to(x.dtype).unsqueeze(1)
    total = torch.zeros(n, x.shape[1], dtype=x.dtype).index_add(0, index, x)
    mu = total / d
    y = x - mu[index]
    var = torch.zeros_like(mu).index_add(0, index, y * y) / d
    blocks = []
    for a in aggs:
        if a == "sum":
            blocks.append(total)
        elif a == "mean":
            blocks.append(mu)
        elif a in ("min", "max"):
            arg = arg_max if a == "max" else arg_min
            picked = torch.gather(x, 0, arg.clamp(min=0))
            blocks.append(torch.where(arg >= 0, picked,
                                      torch.zeros_like(picked)))
        elif a == "std":
            blocks.append(torch.sqrt(var + STD_EPS))
        else:
            blocks.append(var)
    block = torch.stack(blocks, 1)                        # [N, A, F]
    return (block.unsqueeze(1) * scale.view(n, -1, 1, 1)).reshape(n, -1)


# ---------------------------------------------------------------------------
# derived bounds
# ---------------------------------------------------------------------------
def std_exact_bound(dtype):
    """Relative error allowed on std = sqrt(v + 1e-5) * scale where v is
    an exact integer in the accumulator and scale is taken as given.
    With u the accumulator's unit roundoff:
      the constant 1e-5 is rounded to the accumulator, u relative on
        itself, at most u on v + 1e-5;
      the addition rounds once: u; the argument is good to 2 u;
      sqrt halves that, u, and rounds once: 2 u;
      the multiply by scale rounds once: 3 u;
    4 u = 2 eps covers the second-order terms.  A half-type output is
    rounded once more: + its unit roundoff.  The fp64 reference does the
    same three steps in fp64: + 3 u64."""
    u = unit_roundoff(acc_of(dtype))
    b = 4 * u + 3 * unit_roundoff(F64)
    if dtype in (BF, F16):
        b += unit_roundoff(dtype)
    return b


def var_bound(n_row, v, xmax, dtype, with_reference=True):
    """Absolute error allowed on the centered variance of a row of n
    entries, exact inputs, true variance v, max |x| = xmax; u the
    accumulator's unit roundoff.

    Mean: the n - 1 additions and the division give
      |mu^ - mu| <= n u xmax =: delta.
    Second walk: d = fl(x - mu^) (u, twice in the square), d*d (u),
    n - 1 additions of non-negative terms ((n - 1) u), the division
    (u): the computed value is sum (x - mu^)^2 / n to (n + 3) u
    relative, (n + 4) u with the second-order terms.  And
    sum (x - mu^)^2 / n = v + delta^2 exactly, since sum (x - mu) = 0.
    So

      |v^ - v| <= (n + 4) u (v + delta^2) + delta^2
               <= (n + 4) u v + 2 (n u xmax)^2.

    In units of eps = 2 u the leading term is (n + 4) / 2: 34 eps at
    n = 64.  A half-type output is rounded once more: + its unit
    roundoff times v.  That is the bound on the code under test
    (`with_reference=False`); the fp64 reference runs the same
    algorithm, so a comparison with it is allowed the same expression
    with u64 on top."""
    def one(u):
        return (n_row + 4) * u * v + 2 * (n_row * u * xmax) ** 2
    b = one(unit_roundoff(acc_of(dtype)))
    if with_reference:
        b = b + one(unit_roundoff(F64))
    if dtype in (BF, F16):
        b = b + unit_roundoff(dtype) * v
    return b


def std_bound(n_row, v, xmax, dtype, with_reference=True):
    """Relative error allowed on std = sqrt(v^ + 1e-5) * scale of general
    data: the argument v^ + c carries var_bound, the rounding of the
    constant (u c) and of the addition (u (v + c)); sqrt halves the
    relative error and rounds (u), the multiply by scale rounds (u); one
    more u for the second-order terms.  The reference adds its variance
    error, halved, and its three roundings; a half-type output its unit
    roundoff."""
    u = unit_roundoff(acc_of(dtype))
    acc = F64 if dtype == F64 else F32
    arg = (var_bound(n_row, v, xmax, acc, with_reference)
           + u * STD_EPS) / (v + STD_EPS) + u
    b = 0.5 * arg + 3 * u
    if with_reference:
        b = b + 3 * unit_roundoff(F64)
    if dtype in (BF, F16):
        b = b + unit_roundoff(dtype)
    return b


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
def int_case(name, trailing):
    g = gen("pna", name, trailing)
    index = layout(name, g, long_len=LONG_LEN)
    return ints(g, -8, 8, index.numel(), *trailing), index


def ext_case(name, trailing, is_max):
    """Integers with ties and +-inf entries; "gaps" has a row of nothing
    but the reduction's identity."""
    g = gen("pna_ext", name, trailing)
    index = layout(name, g, long_len=LONG_LEN)
    src = ints(g, -8, 8, index.numel(), *trailing)
    hit = torch.rand(src.shape, generator=g)
    src[hit < 0.03] = float("inf")
    src[hit > 0.97] = float("-inf")
    if name == "gaps":
        src[index == 9] = float("-inf") if is_max else float("inf")
    return src, index


def pair_case(feat=3):
    """Rows of k pairs m +- d (k = 0 .. 6 by row, m and d integers per
    row and feature): mu = m and v = d^2 exactly."""
    g = gen("pna_pairs", feat)
    k = torch.arange(N_SEG) % 7
    m = ints(g, -8, 8, N_SEG, feat)
    d = ints(g, 0, 4, N_SEG, feat)
    index = torch.repeat_interleave(torch.arange(N_SEG), 2 * k)
    sign = torch.ones(index.numel(), 1, dtype=F64)
    sign[1::2] = -1          # row lengths are even: pairs stay in a row
    src = m[index] + sign * d[index]
    shuffle = torch.randperm(index.numel(), generator=g)
    var = torch.where((k > 0).unsqueeze(1), d * d, torch.zeros_like(d))
    return src[shuffle], index[shuffle], var


def general_case(dtype, feat=4):
    """Rows of 0 .. 64 entries (row i holds i), values uniform in
    [-1, 1] rounded to `dtype`, shuffled."""
    g = gen("pna_general", dtype)
    n = 65
    index = torch.repeat_interleave(torch.arange(n), torch.arange(n))
    index = index[torch.randperm(index.numel(), generator=g)]
    x = torch.rand(index.numel(), feat, generator=g, dtype=F64) * 2 - 1
    return x.to(dtype).to(F64), index, n


def shifted_case():
    """bf16-representable values 16 + k/8, k in 0 .. 8; rows of 0 .. 64
    entries, 16 features: E[x^2] - E[x]^2 cancels badly here."""
    g = gen("pna_shifted")
    n = 65
    index = torch.repeat_interleave(torch.arange(n), torch.arange(n))
    index = index[torch.randperm(index.numel(), generator=g)]
    k = torch.randint(0, 9, (index.numel(), 16), generator=g).to(F64)
    return 16 + k / 8, index, n


def grad_case(dtype, name="gaps", feat=3):
    """Distinct finite values (unique args) rounded to `dtype`, a
    cotangent W of the output and a cotangent C of dx."""
    g = gen("pna_grad", dtype, name, feat)
    index = layout(name, g, long_len=LONG_LEN)
    e = index.numel()
    x = torch.randn(e, feat, generator=g, dtype=F64).to(dtype).to(F64)
    c = torch.randn(e, feat, generator=g, dtype=F64).to(dtype).to(F64)
    return x, index, c, g


# ---------------------------------------------------------------------------
# checks shared by the CPU and the device tests
# ---------------------------------------------------------------------------
def check_int_blocks(ops, dev, dtype, route, name, aggs=("sum", "mean",
                                                         "min", "max")):
    """sum/min/max equal the fp64 reference rounded once; mean follows
    check_mean_general's rule.  All five scalers: every scaled block is
    one multiply of the accumulator-type block by the fetched scale,
    rounded once."""
    acc = acc_of(dtype)
    for trailing in TRAILING:
        src, index = route_case(route, *int_case(name, trailing))
        out, scale = run(ops, route, put(src, dev, dtype), put(index, dev),
                         N_SEG, aggs, ALL_SCALERS, dev)
        assert out.dtype == dtype and out.shape[0] == N_SEG
        got = split_blocks(out.cpu(), len(ALL_SCALERS), len(aggs))
        assert scale.dtype == acc and scale.shape == (N_SEG, 5)
        assert torch.equal(scale[:, 0], torch.ones(N_SEG, dtype=acc))
        for a, agg in enumerate(aggs):
            ref = ref_block(agg, src, index, N_SEG)
            # the accumulator-type block: exact integers, or the
            # correctly rounded quotient
            block = ref.to(acc)
            what = f"{agg} {route} {name} {dtype} {trailing}"
            if agg == "mean" and dtype in (BF, F16):
                assert torch.equal(got[:, 0, a], block.to(dtype)), what
            else:
                assert same(got[:, 0, a], ref, dtype), what
            for s in range(1, len(ALL_SCALERS)):
                want = (block * scale[:, s:s + 1]).to(dtype)
                assert torch.equal(got[:, s, a], want), \
                    f"{what} scaler {ALL_SCALERS[s]}"


def check_extremes(ops, dev, dtype, route, name, trailing):
    """min and max with +-inf entries: values, gradient routing to the
    lowest position attaining the extreme, and h_min / h_max of the
    second order; integer cotangents, identity scaler: bit for bit."""
    for is_max in (False, True):
        agg = "max" if is_max else "min"
        src, index = route_case(route, *ext_case(name, trailing, is_max))
        ref, arg = ref_minmax(src, index, N_SEG, is_max)
        x = put(src, dev, dtype).requires_grad_(True)
        out, _ = run(ops, route, x, put(index, dev), N_SEG, (agg,),
                     ("identity",), dev)
        what = f"{agg} {route} {name} {dtype} {trailing}"
        assert same(out, ref.reshape(N_SEG, -1), dtype), what
        g = gen("pna_ext_grad", name, trailing)
        w64 = ints(g, 1, 8, *out.shape)
        w = put(w64, dev, dtype).requires_grad_(True)
        (dx,) = torch.autograd.grad(out, x, w, create_graph=True)
        want = ref_minmax_grad(arg, w64.reshape(ref.shape), src.shape[0])
        assert same(dx, want, dtype), f"routing {what}"
        # second order: R = <c, dx>; dR/dw picks c at the arg
        c64 = ints(g, 1, 8, *src.shape)
        (hw,) = torch.autograd.grad(dx, w, put(c64, dev, dtype))
        flat_c = c64.reshape(src.shape[0], -1)
        flat_arg = arg.reshape(N_SEG, -1)
        picked = torch.gather(flat_c, 0, flat_arg.clamp(min=0))
        want = torch.where(flat_arg >= 0, picked, torch.zeros_like(picked))
        assert same(hw, want, dtype), f"second order {what}"


def check_pairs(ops, dev, dtype, route):
    src, index, var = pair_case()
    src, index = route_case(route, src, index)
    out, _ = run(ops, route, put(src, dev, dtype), put(index, dev), N_SEG,
                 ("var", "std", "mean"), ("identity",), dev)
    got = split_blocks(out.cpu(), 1, 3)[:, 0]
    assert same(got[:, 0], var, dtype), f"var {route} {dtype}"
    ref = torch.sqrt(var + STD_EPS)
    rel = (got[:, 1].to(F64) - ref).abs() / ref
    assert bool((rel <= std_exact_bound(dtype)).all()), \
        f"std {route} {dtype}: worst {rel.max():.3e}"
    assert same(got[:, 2], ref_block("mean", src, index, N_SEG), dtype)


def check_general(ops, dev, dtype, route):
    """var and std of general data against the fp64 centered reference,
    within the derived bounds; returns the worst errors in units of the
    accumulator eps."""
    src, index, n = general_case(dtype)
    src, index = route_case(route, src, index)
    out, _ = run(ops, route, put(src, dev, dtype), put(index, dev), n,
                 ("var", "std"), ("identity",), dev)
    got = split_blocks(out.cpu(), 1, 2)[:, 0].to(F64)
    v = ref_var(src, index, n)
    sd = torch.sqrt(v + STD_EPS)
    lens = counts_of(index, n).to(F64).unsqueeze(1)
    xmax = torch.zeros_like(v).scatter_reduce(
        0, index.unsqueeze(1).expand_as(src), src.abs(), "amax")
    vb = var_bound(lens, v, xmax, dtype)
    sb = std_bound(lens, v, xmax, dtype)
    eps = torch.finfo(acc_of(dtype)).eps
    if dtype in (F32, F64):
        # the condition on the bound itself: at most 64 eps, relative,
        # for these rows of up to 64 entries
        rows = lens.squeeze(1) >= 2
        own_v = var_bound(lens, v, xmax, dtype, with_reference=False)
        own_s = std_bound(lens, v, xmax, dtype, with_reference=False)
        assert bool((own_v[rows] / v[rows] <= 64 * eps).all())
        assert bool((own_s <= 64 * eps).all())
    err_v = (got[:, 0] - v).abs()
    err_s = (got[:, 1] - sd).abs() / sd
    assert bool((err_v <= vb).all()), \
        f"var {route} {dtype}: worst excess {(err_v - vb).max():.3e}"
    assert bool((err_s <= sb).all()), \
        f"std {route} {dtype}: worst {err_s.max():.3e}"
    rows = lens.squeeze(1) >= 2
    return (float((err_v[rows] / v[rows]).max() / eps),
            float(err_s.max() / eps))


def check_empty(ops, dev, dtype):
    """E = 0 and N = 0: the empty-row values times the scale, and
    empty gradients."""
    aggs = ("sum", "mean", "min", "max", "std", "var")
    for n in (N_SEG, 0):
        x = put(torch.zeros(0, 5), dev, dtype).requires_grad_(True)
        index = torch.zeros(0, dtype=torch.long)
        out, scale = run(ops, "sorted", x, put(index, dev), n, aggs,
                         DEFAULT_SCALERS, dev)
        assert out.shape == (n, 4 * 6 * 5) and out.dtype == dtype
        acc = acc_of(dtype)
        block = torch.zeros(n, 6, 5, dtype=acc)
        block[:, 4] = torch.sqrt(torch.tensor(STD_EPS, dtype=acc))
        want = (block.unsqueeze(1) * scale.view(n, 4, 1, 1)).to(dtype)
        assert torch.equal(out.detach().cpu(), want.flatten(1))
        (dx,) = torch.autograd.grad(out, x, torch.ones_like(out))
        assert dx.shape == (0, 5)


def grads_of(ops, dev, dtype, route, aggs, scalers, name="gaps"):
    """(out, dx, gx, hw) of the op in `dtype` on `dev`, the fp64
    autograd reference of the same four, for one grad_case."""
    x64, index, c64, g = grad_case(dtype, name)
    if route == "sorted":          # the cotangent of dx moves with x
        c64 = c64[torch.argsort(index, stable=True)]
    x64, index = route_case(route, x64, index)
    x = put(x64, dev, dtype).requires_grad_(True)
    out, scale = run(ops, route, x, put(index, dev), N_SEG, aggs, scalers,
                     dev)
    w64 = torch.randn(out.shape, generator=g, dtype=F64).to(dtype).to(F64)
    w = put(w64, dev, dtype).requires_grad_(True)
    (dx,) = torch.autograd.grad(out, x, w, create_graph=True)
    gx, hw = torch.autograd.grad(dx, (x, w), put(c64, dev, dtype),
                                 allow_unused=True)
    if gx is None:
        gx = torch.zeros_like(x)
    got = [t.detach().cpu().to(F64) for t in (out, dx, gx, hw)]

    _, amin = ref_minmax(x64, index, N_SEG, False)
    _, amax = ref_minmax(x64, index, N_SEG, True)
    xr = x64.clone().requires_grad_(True)
    wr = w64.clone().requires_grad_(True)
    ro = ref_differentiable(xr, index, N_SEG, aggs, scale.to(F64), amin,
                            amax)
    (rdx,) = torch.autograd.grad(ro, xr, wr, create_graph=True)
    rgx, rhw = torch.autograd.grad(rdx, (xr, wr), c64, allow_unused=True)
    if rgx is None:
        rgx = torch.zeros_like(x64)
    return got, [ro.detach(), rdx.detach(), rgx, rhw]


def max_errors(got, ref):
    return [float((a - b).abs().max()) for a, b in zip(got, ref)]
