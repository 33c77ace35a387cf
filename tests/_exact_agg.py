"""Shared pieces of the exact tests of the aggregation family
(test_agg_exact.py on the CPU paths, test_gpu_agg_exact.py on the HIP
kernels): case builders and references that do not go through
`hydragnn_amd.ops.scatter`.  The checks take the ops under test as
arguments.

Exact-integer method, as in _exact_linear.py: sources are seeded
integers in [-8, 8] and a segment holds at most about 2500 entries, so
every partial sum is an integer below 2^24, exact in fp32 whatever the
order of accumulation, atomics included.  The fp64 reference then fixes
every output bit: the expected output is the reference rounded once to
the output dtype and the comparison is `torch.equal`.

Ordered-float method, for the fixed-order sum routes on arbitrary
floats: the same IEEE additions in the same order (ascending position
within the row, from 0, in fp32 for fp32/bf16/f16 and in fp64 for fp64)
give the same bits.
"""

import torch

BF = torch.bfloat16
F16 = torch.float16
F32 = torch.float32
F64 = torch.float64
DTYPES = [F32, F64, BF, F16]


def dtype_id(dtype):
    """Readable test ids: float32, float64, bfloat16, float16."""
    return str(dtype).split(".")[-1]


N_SEG = 40          # dim_size of the small layouts
# explicit mantissa bits and least normal exponent of the half types
_FMT = {BF: (7, -126), F16: (10, -14)}


def seed_of(*key):
    """A seed that does not depend on the interpreter's hash salt."""
    s = 0
    for ch in "/".join(str(k) for k in key):
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


def gen(*key):
    g = torch.Generator()
    g.manual_seed(seed_of(*key))
    return g


def ints(g, lo, hi, *shape):
    """Seeded integers, uniform in [lo, hi], as fp64 on the CPU."""
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


# ---------------------------------------------------------------------------
# segment layouts: an unsorted int64 index over N_SEG rows
# ---------------------------------------------------------------------------
# rows that stay empty in "gaps": the start, the middle and the end, so
# dim_size also exceeds index.max() + 1
EMPTY_ROWS = (0, 1, 17, 18, 19, 20, 36, 37, 38, 39)
LAYOUTS = ("gaps", "one_row", "single", "long", "run")


def layout(name, g, long_len=2100):
    if name == "gaps":
        rows = torch.tensor([r for r in range(N_SEG)
                             if r not in EMPTY_ROWS])
        return rows[torch.randint(0, len(rows), (301,), generator=g)]
    if name == "one_row":      # worst atomic contention
        return torch.full((500,), 7, dtype=torch.long)
    if name == "single":       # E = 1
        return torch.tensor([5])
    # "run" is the layout of "long"; its sum case holds ones only
    if name in ("long", "run"):     # one long row among short ones
        idx = torch.cat([torch.full((long_len,), 3, dtype=torch.long),
                         torch.randint(4, 30, (200,), generator=g)])
        return idx[torch.randperm(idx.numel(), generator=g)]
    raise KeyError(name)


TRAILING = ((), (1,), (3,), (5,), (64,), (4, 3))


def rowptr_of(index, n):
    """CSR row pointer of a (sorted or stably sorted) index."""
    rp = torch.zeros(n + 1, dtype=torch.long)
    rp[1:] = torch.bincount(index, minlength=n).cumsum(0)
    return rp


def csr_of(index, n):
    """(perm, rowptr) with perm = argsort(index, stable=True)."""
    return torch.argsort(index, stable=True), rowptr_of(index, n)


# ---------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------
def _bc(v, like):
    return v.view(-1, *([1] * (like.dim() - 1)))


def ref_sum(src, index, n):
    out = torch.zeros((n,) + src.shape[1:], dtype=F64)
    return out.index_add_(0, index, src.to(F64))


def ref_mean(src, index, n):
    s = ref_sum(src, index, n)
    count = torch.bincount(index, minlength=n).clamp(min=1).to(F64)
    return s / _bc(count, s)


def ref_minmax(src, index, n, is_max):
    """Direct per-segment reduction.  The lowest edge index attaining
    the extreme wins the arg; an empty segment gives 0 and -1."""
    src = src.to(F64)
    out = torch.zeros((n,) + src.shape[1:], dtype=F64)
    arg = torch.full((n,) + src.shape[1:], -1, dtype=torch.long)
    for r in torch.unique(index).tolist():
        e = (index == r).nonzero().flatten()        # ascending
        v = src[e]
        m = v.max(0).values if is_max else v.min(0).values
        first = (v == m).to(torch.int8).argmax(0)   # first True
        out[r] = m
        arg[r] = e[first]
    return out, arg


def ref_minmax_grad(arg, grad_out, n_edges):
    """grad_src[arg[r, f], f] = grad_out[r, f] where arg >= 0."""
    n = arg.shape[0]
    a = arg.reshape(n, -1)
    g = grad_out.to(F64).reshape(n, -1)
    cols = torch.arange(a.shape[1]).expand_as(a)
    gs = torch.zeros(n_edges, a.shape[1], dtype=F64)
    ok = a >= 0
    gs.index_put_((a[ok], cols[ok]), g[ok], accumulate=True)
    return gs.reshape((n_edges,) + arg.shape[1:])


def ref_ordered_sum(src, index, n):
    """Per row, acc = 0; acc += src[e] for e ascending: in fp64 for
    fp64 sources, else in fp32 with one final rounding to src.dtype.
    A vectorised add over a padded [rows, max_len] layout; the trailing
    zeros of shorter rows add nothing."""
    acc_t = F64 if src.dtype == F64 else F32
    order = torch.argsort(index, stable=True)
    sidx = index[order]
    counts = torch.bincount(index, minlength=n)
    pos = torch.arange(index.numel()) - (counts.cumsum(0) - counts)[sidx]
    width = int(counts.max()) if index.numel() else 0
    pad = torch.zeros((n, width) + src.shape[1:], dtype=acc_t)
    pad[sidx, pos] = src[order].to(acc_t)
    acc = torch.zeros((n,) + src.shape[1:], dtype=acc_t)
    for k in range(width):
        acc = acc + pad[:, k]
    return acc.to(src.dtype)


# ---------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------
def same(got, ref, dtype):
    """Bit equality with the fp64 reference rounded once to `dtype`.
    Integer references pass through fp32 unchanged (< 2^24)."""
    assert got is not None, "result is missing"
    fin = ref[torch.isfinite(ref)]
    assert fin.numel() == 0 or fin.abs().max() < 2 ** 24
    want = ref.to(dtype)
    got = got.detach().cpu()
    return (got.dtype == dtype and got.shape == want.shape
            and torch.equal(got, want))


def ulp(ref, dtype):
    """Unit in the last place of `dtype` at the fp64 values `ref`."""
    bits, emin = _FMT[dtype]
    _, e = torch.frexp(ref.abs())            # |ref| = m 2^e, m in [.5, 1)
    e = torch.where(ref == 0, torch.full_like(e, emin), e - 1)
    e = e.clamp(min=emin)
    return torch.ldexp(torch.ones_like(ref), e - bits)


def within_one_ulp(got, ref, dtype):
    got = got.detach().cpu()
    return (got.dtype == dtype and got.shape == ref.shape
            and bool(((got.to(F64) - ref).abs() <= ulp(ref, dtype)).all()))


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
def sum_case(name, trailing, long_len=2100):
    g = gen("sum", name, trailing, long_len)
    index = layout(name, g, long_len)
    if name == "run":
        # signed values keep a long row's partial sums small; a run of
        # ones walks them up to long_len, past 2048 where an f16
        # accumulator stops counting
        return torch.ones(index.numel(), *trailing, dtype=F64), index
    return ints(g, -8, 8, index.numel(), *trailing), index


# rows of the constant-mean case: (row, count); every entry of row r is
# the integer v[r] (per trailing element), so the mean is exactly v[r]
CONST_COUNTS = ((2, 1), (3, 2), (5, 259), (8, 1000), (9, 3), (21, 7),
                (30, 1), (35, 300))


def const_mean_case(trailing, lo=-8, hi=8):
    g = gen("const_mean", trailing)
    v = ints(g, lo, hi, N_SEG, *trailing)
    index = torch.cat([torch.full((c,), r, dtype=torch.long)
                       for r, c in CONST_COUNTS])
    index = index[torch.randperm(index.numel(), generator=g)]
    want = torch.zeros_like(v)
    rows = torch.tensor([r for r, _ in CONST_COUNTS])
    want[rows] = v[rows]
    return v[index], index, want


def minmax_case(name, trailing, is_max):
    """Integer sources (ties are common) with some +-inf entries, and
    for "gaps" a row that holds nothing but the reduction's identity
    (-inf under max, +inf under min)."""
    g = gen("minmax", name, trailing)
    index = layout(name, g, long_len=400)
    src = ints(g, -8, 8, index.numel(), *trailing)
    hit = torch.rand(src.shape, generator=g)
    src[hit < 0.03] = float("inf")
    src[hit > 0.97] = float("-inf")
    ident_row = None
    if name == "gaps":
        ident_row = 9
        src[index == ident_row] = float("-inf") if is_max else float("inf")
    return src, index, ident_row


def closure_case(n_nodes=50, n_edges=400, feat=5):
    """x [n_nodes, feat], w [n_edges, feat] integers in [-3, 3]; gather
    index i and scatter index j.  Every polynomial of the two gradient
    orders stays far below 2^24 (asserted on the reference)."""
    g = gen("closure")
    x = ints(g, -3, 3, n_nodes, feat)
    w = ints(g, -3, 3, n_edges, feat)
    i = torch.randint(0, n_nodes, (n_edges,), generator=g)
    j = torch.randint(0, N_SEG, (n_edges,), generator=g)
    return x, w, i, j


def closure_reference(x, w, i, j):
    """First and second gradients of scatter(gather(x, i)^2 w, j).sum()
    in fp64 torch indexing."""
    x = x.clone().requires_grad_(True)
    y = torch.zeros(N_SEG, x.shape[1], dtype=F64).index_add(
        0, j, x[i] ** 2 * w).sum()
    g1 = torch.autograd.grad(y, x, create_graph=True)[0]
    g2 = torch.autograd.grad(g1.square().sum(), x)[0]
    return g1.detach(), g2


def softmax_case(dtype):
    """Finite inputs in [-8, 8] already rounded to `dtype`; 128
    segments of 0 to 3 entries (the lengths for which the bound of
    `softmax_bound` is a worst-case one), several of exactly one."""
    g = gen("softmax", dtype)
    lens = torch.randint(0, 4, (SOFTMAX_SEG,), generator=g)
    lens[[4, 11, 40]] = 1
    index = torch.repeat_interleave(torch.arange(SOFTMAX_SEG), lens)
    index = index[torch.randperm(index.numel(), generator=g)]
    x = (torch.rand(index.numel(), generator=g, dtype=F64) * 16 - 8)
    return x.to(dtype), index, lens


def softmax_bound(shift, dtype):
    """Relative error allowed on segment_softmax: (|x - max| + 4) eps
    with eps = 2^-23 (fp32) or 2^-52 (fp64); u = eps / 2 is the unit
    roundoff.  Derived, for segments of n <= 3 entries:
      numerator   exp(fl(x - max)): the subtraction is rounded once,
                  |x - max| u relative on the result, and exp is good
                  to 1 ulp = 2 u;
      denominator its terms carry the same errors weighted by their
                  share p_k of the sum; the largest term is exp(0) = 1
                  exactly, so the weighted 2 u part is at most
                  (1 - 1/n) 2 u and sum_k p_k |x_k - max| u <= log(n) u;
                  the n - 1 additions round once each;
      quotient    one rounding, u.
    Sum at n = 3: (2 + 4/3 + 1.1 + 2 + 1) u + |x - max| u < 8 u + 2
    |x - max| u = (|x - max| + 4) eps."""
    eps = 2.0 ** -23 if dtype == F32 else 2.0 ** -52
    return (shift + 4) * eps


SOFTMAX_SEG = 128


def ref_softmax(x, index, n):
    """fp64 per-segment softmax and |x - max| per entry."""
    x = x.to(F64)
    out = torch.zeros_like(x)
    shift = torch.zeros_like(x)
    for r in torch.unique(index).tolist():
        e = index == r
        shift[e] = x[e].max() - x[e]
        out[e] = torch.softmax(x[e], 0)
    return out, shift


# ---------------------------------------------------------------------------
# checks, shared by the CPU and the device tests.  `ops` provides
# scatter, gather and segment_softmax; `dev` is where the inputs go.
# ---------------------------------------------------------------------------
SUM_ROUTES = ("atomic", "sorted", "indexed", "deterministic")


def put(t, dev, dtype=None):
    return t.to(device=dev, dtype=dtype)


def run_sum(ops, route, src, index, n):
    """scatter-sum of device tensors by one of the four routes.  On the
    CPU all four are `index_add_`."""
    import os
    if route == "atomic":
        return ops.scatter(src, index, n, "sum")
    if route == "sorted":
        o = torch.argsort(index, stable=True)
        return ops.scatter(src[o], index[o], n, "sum", sorted_index=True)
    if route == "indexed":
        perm, rowptr = csr_of(index.cpu(), n)
        return ops.scatter(src, index, n, "sum",
                           csr=(put(perm, src.device),
                                put(rowptr, src.device)))
    assert route == "deterministic"
    os.environ["HYDRAGNN_DETERMINISTIC"] = "1"
    try:
        return ops.scatter(src, index, n, "sum")
    finally:
        os.environ.pop("HYDRAGNN_DETERMINISTIC")


def check_gather(ops, dev, dtype, trailing):
    g = gen("gather", trailing)
    src = ints(g, -8, 8, 37, *trailing).to(dtype)
    index = torch.randint(0, 37, (301,), generator=g)
    out = ops.gather(put(src, dev), put(index, dev))
    assert out.dtype == dtype and torch.equal(out.cpu(), src[index]), \
        f"gather {dtype} {trailing}"
    one = ops.gather(put(src, dev), put(index[:1], dev))       # E = 1
    assert torch.equal(one.cpu(), src[index[:1]])


def check_sum(ops, dev, dtype, route, name):
    for trailing in TRAILING:
        src, index = sum_case(name, trailing)
        out = run_sum(ops, route, put(src, dev, dtype), put(index, dev),
                      N_SEG)
        assert same(out, ref_sum(src, index, N_SEG), dtype), \
            f"sum {route} {name} {dtype} trailing {trailing}"


def run_mean(ops, sorted_route, src, index, n):
    if sorted_route:
        o = torch.argsort(index, stable=True)
        return ops.scatter(src[o], index[o], n, "mean", sorted_index=True)
    return ops.scatter(src, index, n, "mean")


def check_mean_const(ops, dev, dtype, sorted_route):
    """Every entry of row r is the integer v_r: the sum count * v_r is
    exact in the accumulator and its quotient by count is v_r."""
    for trailing in ((), (3,), (4, 3)):
        src, index, want = const_mean_case(trailing)
        out = run_mean(ops, sorted_route, put(src, dev, dtype),
                       put(index, dev), N_SEG)
        assert same(out, want, dtype), \
            f"constant mean {dtype} sorted={sorted_route} {trailing}"


def check_mean_general(ops, dev, dtype, sorted_route):
    """fp32/fp64: the fp64 quotient rounded to the output type.  With
    numerator and count below 2^24 a quotient that is not itself an
    fp32 number is at least 2^-49 (relative) away from any fp32
    rounding boundary, further than the fp64 quotient's own error, so
    rounding it is the correctly rounded fp32 division.  bf16/f16: one
    ulp of the output type around the fp64 mean; the exact sum divided
    in fp32 and rounded once is within 1/2 ulp plus the fp32 division's
    2^-24, which can cross one rounding boundary and no more.  The
    half-type result is also pinned bit for bit as the fp32 quotient
    rounded once, which is what the kernels are documented to do."""
    for name in ("gaps", "long", "one_row", "run"):
        for trailing in ((), (5,), (4, 3)):
            src, index = sum_case(name, trailing)
            ref = ref_mean(src, index, N_SEG)
            out = run_mean(ops, sorted_route, put(src, dev, dtype),
                           put(index, dev), N_SEG)
            ok = (same(out, ref, dtype) if dtype in (F32, F64)
                  else within_one_ulp(out, ref, dtype))
            assert ok, (f"mean {dtype} sorted={sorted_route} {name} "
                        f"{trailing}")
            if dtype in (BF, F16):
                # the kernels' route, bit for bit: the fp32 quotient
                # (the fp64 one rounded to fp32, as above) rounded once
                assert same(out, ref.to(F32).to(F64), dtype), \
                    f"mean {dtype} sorted={sorted_route} {name} fp32 route"


def check_minmax(ops, dev, dtype, is_max, name, trailing):
    """Value, and through a nonzero integer cotangent the arg: the
    gradient lands on the lowest edge attaining the extreme, rows
    without edges route nothing."""
    red = "max" if is_max else "min"
    src, index, ident_row = minmax_case(name, trailing, is_max)
    ref, arg = ref_minmax(src, index, N_SEG, is_max)
    if ident_row is not None:     # all -inf under max, all +inf under min
        first = int((index == ident_row).nonzero()[0])
        assert torch.isinf(ref[ident_row]).all()
        assert (arg[ident_row] == first).all()
    x = put(src, dev, dtype).requires_grad_(True)
    out = ops.scatter(x, put(index, dev), N_SEG, red)
    assert same(out, ref, dtype), f"{red} {name} {dtype} {trailing}"
    grad_out = ints(gen("minmax_grad", name, trailing), 1, 8, *ref.shape)
    (gs,) = torch.autograd.grad(out, x, put(grad_out, dev, dtype))
    assert same(gs, ref_minmax_grad(arg, grad_out, src.shape[0]), dtype), \
        f"{red} gradient routing {name} {dtype} {trailing}"
    return x.detach(), arg


def check_empty_edges(ops, dev, dtype):
    """E = 0 with trailing dims: zeros of [dim_size, 5] from every
    reduce and every sum route; min/max backward gives an empty
    gradient.  dim_size = 0 gives an empty result."""
    index = put(torch.zeros(0, dtype=torch.long), dev)
    for n in (N_SEG, 0):
        want = torch.zeros(n, 5, dtype=dtype)
        for route in SUM_ROUTES:
            src = put(torch.zeros(0, 5), dev, dtype)
            out = run_sum(ops, route, src, index, n)
            assert out.dtype == dtype and torch.equal(out.cpu(), want), \
                f"sum {route} E=0 n={n}"
        for sorted_route in (False, True):
            src = put(torch.zeros(0, 5), dev, dtype)
            out = run_mean(ops, sorted_route, src, index, n)
            assert torch.equal(out.cpu(), want), f"mean E=0 n={n}"
        for red in ("max", "min"):
            x = put(torch.zeros(0, 5), dev, dtype).requires_grad_(True)
            out = ops.scatter(x, index, n, red)
            assert out.dtype == dtype and torch.equal(out.cpu(), want), \
                f"{red} E=0 n={n}"
            (gs,) = torch.autograd.grad(out, x, torch.ones_like(out))
            assert gs.shape == (0, 5)
    out = ops.gather(put(torch.ones(7, 5), dev, dtype), index)
    assert out.shape == (0, 5)


def check_closure(ops, dev, dtype, variant):
    """First and second gradients of scatter(gather(x, i)^2 w, j).sum()
    against fp64 torch indexing, bit for bit."""
    x64, w, i, j = closure_case()
    if variant == "sorted":
        j = j.sort().values
    r1, r2 = closure_reference(x64, w, i, j)
    x = put(x64, dev, dtype).requires_grad_(True)
    csr = None
    if variant == "backward_csr":
        perm, rowptr = csr_of(i, x64.shape[0])
        csr = (put(perm, dev), put(rowptr, dev))
    y = ops.scatter(ops.gather(x, put(i, dev), backward_csr=csr) ** 2
                    * put(w, dev, dtype), put(j, dev), N_SEG, "sum",
                    sorted_index=(variant == "sorted")).sum()
    g1 = torch.autograd.grad(y, x, create_graph=True)[0]
    assert same(g1, r1, dtype), f"first gradient {variant} {dtype}"
    g2 = torch.autograd.grad(g1.square().sum(), x)[0]
    assert same(g2, r2, dtype), f"second gradient {variant} {dtype}"


def check_softmax(ops, dev, dtype):
    x, index, lens = softmax_case(dtype)
    ref, shift = ref_softmax(x, index, SOFTMAX_SEG)
    out = ops.segment_softmax(put(x, dev), put(index, dev), SOFTMAX_SEG)
    out = out.cpu()
    assert out.dtype == dtype
    # bound derived in softmax_bound, not measured
    rel = (out.to(F64) - ref).abs() / ref
    assert bool((rel <= softmax_bound(shift, dtype)).all()), \
        f"segment_softmax {dtype}: worst rel err {rel.max():.3e}"
    alone = lens[index] == 1
    assert bool(alone.any()) and bool((out[alone] == 1).all())
