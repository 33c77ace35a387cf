"""Exact tests of the aggregation kernels of `csrc/hip_ops.hip`
(`gather_kernel(_vec)`, `scatter_add_*`, `segment_sum_csr(_idx)_kernel`,
`count_kernel` / `divide_rows_kernel`, the `scatter_max_*` passes) and
of the dispatch in `ops/scatter.py`, against the references of
_exact_agg.py, which do not go through the project's CPU path.

Sources are seeded integers in [-8, 8] and no segment holds more than
about 2500 of them: every partial sum is an integer below 2^24, exact
in fp32 in any order, atomics included.  The fp64 reference rounded
once to the output dtype is then the only right answer and the
comparison is `torch.equal`.  The three fixed-order sum routes are also
compared bit for bit, on random normal sources, with a reference that
performs the same IEEE additions in the same order.  Only two checks
carry a tolerance, each derived where it is defined: the bf16/f16 mean
of general sources (one ulp of the output type,
`_exact_agg.check_mean_general`) and `segment_softmax`
(`_exact_agg.softmax_bound`).

Shapes are the smallest at which these kernels can go wrong: trailing
dims 1, 3, 5, 64, ranks 1 to 3, rows on both sides of the float4
condition, empty rows at the start, middle and end, one row taking
every edge, E = 1, E = 0, dim_size = 0, one long row, strided inputs,
and one case per kernel family just above the grid cap (2048 blocks of
256 threads; 8192 blocks for the CSR kernels) so that the grid-stride
loop runs a second iteration.

NaN sources and out-of-range indices are unspecified and never passed.
"""

import types

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

import _exact_agg as A  # noqa: E402
from _exact_agg import BF, F16, F32, F64, N_SEG, put  # noqa: E402
from hydragnn_amd.ops import (  # noqa: E402
    gather, get_extension, scatter, segment_softmax,
)

DEV = "cuda"
OPS = types.SimpleNamespace(scatter=scatter, gather=gather,
                            segment_softmax=segment_softmax)
WIDE = [F32, F64]
CAP = 2048 * 256          # threads of a full grid
CAP_CSR = 8192 * 256

# row lengths on the float4 path (row bytes % 16 == 0) and off it
F4_ROWS = {F32: (4, 3, 6), BF: (8, 4, 12), F16: (8, 4, 12), F64: (2, 1, 3)}


def _ext():
    return get_extension(required=True)


# ---------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.dtype_id)
def test_gather(dtype):
    for trailing in A.TRAILING + tuple((f,) for f in F4_ROWS[dtype]):
        A.check_gather(OPS, DEV, dtype, trailing)


@pytest.mark.parametrize("dtype,feat", [(F32, 4), (BF, 8)],
                         ids=["float32-4", "bfloat16-8"])
def test_gather_misaligned_base(dtype, feat):
    """A contiguous view one element into a larger buffer: the row is a
    multiple of 16 bytes, the base is not."""
    g = A.gen("gather_misaligned", feat)
    flat = A.ints(g, -8, 8, 1 + 37 * feat).to(dtype)
    index = torch.randint(0, 37, (301,), generator=g)
    src = put(flat, DEV)[1:].view(37, feat)
    assert src.is_contiguous() and src.data_ptr() % 16 != 0
    out = gather(src, put(index, DEV))
    assert torch.equal(out.cpu(), flat[1:].view(37, feat)[index])


@pytest.mark.parametrize("path", ["scalar", "float4"])
def test_gather_second_grid_stride_iteration(path):
    g = A.gen("gather_stride", path)
    feat = 64 if path == "scalar" else 256
    flat = A.ints(g, -8, 8, 1 + 100 * feat).to(F32)
    index = torch.randint(0, 100, (8200,), generator=g)
    # the scalar kernel takes 16-byte rows only from a misaligned base
    off = 1 if path == "scalar" else 0
    src = put(flat, DEV)[off:off + 100 * feat].view(100, feat)
    assert (src.data_ptr() % 16 != 0) == (path == "scalar")
    per_thread = 1 if path == "scalar" else 4
    assert 8200 * feat // per_thread > CAP
    out = gather(src, put(index, DEV))
    assert torch.equal(out.cpu(),
                       flat[off:off + 100 * feat].view(100, feat)[index])


# ---------------------------------------------------------------------------
# sum
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.LAYOUTS)
@pytest.mark.parametrize("route", A.SUM_ROUTES)
@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.dtype_id)
def test_sum(dtype, route, name):
    A.check_sum(OPS, DEV, dtype, route, name)


@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.dtype_id)
def test_sum_fixed_order_routes_bitwise(dtype):
    """Sorted CSR, indexed CSR with a stable perm and
    HYDRAGNN_DETERMINISTIC=1 add each row's entries in ascending
    position from 0, in fp32 (fp64 for fp64): on random normal sources
    they equal the ordered reference, and so one another, bit for
    bit."""
    for name, long_len in (("gaps", 0), ("long", 300)):
        g = A.gen("ordered", name, dtype)
        index = A.layout(name, g, long_len)
        src = torch.randn(index.numel(), 5, generator=g, dtype=F64).to(dtype)
        want = A.ref_ordered_sum(src, index, N_SEG)
        for route in ("sorted", "indexed", "deterministic"):
            out = A.run_sum(OPS, route, put(src, DEV), put(index, DEV),
                            N_SEG)
            assert out.dtype == dtype and torch.equal(out.cpu(), want), \
                f"{route} {name} {dtype}"


def test_sum_atomic_second_grid_stride_iteration():
    g = A.gen("sum_stride")
    index = torch.randint(0, N_SEG, (8200,), generator=g)
    src = A.ints(g, -8, 8, 8200, 64)
    assert src.numel() > CAP
    out = scatter(put(src, DEV, F32), put(index, DEV), N_SEG, "sum")
    assert A.same(out, A.ref_sum(src, index, N_SEG), F32)


@pytest.mark.parametrize("route", ["sorted", "indexed"])
def test_sum_csr_second_grid_stride_iteration(route):
    """N * F = 8200 * 257 output elements, above the CSR kernels' cap
    of 8192 blocks; rows hold 0 or 1 entries."""
    g = A.gen("csr_stride")
    n, feat = 8200, 257
    assert n * feat > CAP_CSR
    index = torch.randperm(n, generator=g)[:n // 2]
    src = A.ints(g, -8, 8, index.numel(), feat)
    out = A.run_sum(OPS, route, put(src, DEV, F32), put(index, DEV), n)
    assert A.same(out, A.ref_sum(src, index, n), F32)


def test_csr_sum_of_a_zero_row_source():
    """The entry point itself: a [0, F] source gives zeros of [N, F],
    with and without a perm; N = 0 gives an empty result."""
    ext = _ext()
    none = put(torch.zeros(0, dtype=torch.long), DEV)
    for dtype in A.DTYPES:
        src = put(torch.zeros(0, 5), DEV, dtype)
        for rows in (N_SEG, 0):
            rowptr = put(torch.zeros(rows + 1, dtype=torch.long), DEV)
            for perm in (None, none):
                out = ext.segment_sum_csr(src, rowptr, perm)
                assert torch.equal(out.cpu(),
                                   torch.zeros(rows, 5, dtype=dtype))
            out = ext.segment_sum_csr(src, rowptr, None, True)
            assert torch.equal(out.cpu(), torch.zeros(rows, 5, dtype=dtype))


# ---------------------------------------------------------------------------
# mean
# ---------------------------------------------------------------------------
MEAN_ROUTES = pytest.mark.parametrize(
    "sorted_route", [False, True], ids=["atomic", "sorted"])


@MEAN_ROUTES
@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.dtype_id)
def test_mean_of_constant_segments(dtype, sorted_route):
    A.check_mean_const(OPS, DEV, dtype, sorted_route)


@MEAN_ROUTES
@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.dtype_id)
def test_mean_is_rounded_once(dtype, sorted_route):
    A.check_mean_general(OPS, DEV, dtype, sorted_route)


@MEAN_ROUTES
def test_mean_f16_sum_beyond_the_f16_range(sorted_route):
    """300 values of 400 sum to 120000, past f16's 65504; the fp32
    accumulator is divided before the one cast, so the mean is 400."""
    index = torch.cat([torch.full((300,), 6), torch.arange(10, 20)])
    src = torch.cat([torch.full((300, 3), 400.0), torch.ones(10, 3)])
    out = A.run_mean(OPS, sorted_route, put(src, DEV, F16),
                     put(index, DEV), N_SEG)
    assert A.same(out, A.ref_mean(src, index, N_SEG), F16)
    assert bool((out[6] == 400).all())


def test_mean_count_second_grid_stride_iteration():
    """E = 524 800 with F = 1: `count_kernel` runs past its grid."""
    g = A.gen("count_stride")
    n, n_edges = 300, 524_800
    assert n_edges > CAP
    index = torch.randint(0, n, (n_edges,), generator=g)
    assert int(torch.bincount(index).max()) < 2500
    src = A.ints(g, -8, 8, n_edges, 1)
    out = scatter(put(src, DEV, F32), put(index, DEV), n, "mean")
    assert A.same(out, A.ref_mean(src, index, n), F32)


# ---------------------------------------------------------------------------
# min / max
# ---------------------------------------------------------------------------
IS_MAX = pytest.mark.parametrize("is_max", [True, False],
                                 ids=["max", "min"])


@pytest.mark.parametrize("name", A.LAYOUTS)
@IS_MAX
@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.dtype_id)
def test_minmax_value_arg_and_gradient(dtype, is_max, name):
    """Value and gradient routing through `scatter`, and the arg the
    entry point returns: ties go to the lowest edge, +-inf entries
    count, a row of nothing but the identity gives it back with its
    first edge, empty rows give 0 and -1."""
    for trailing in ((), (3,), (5,), (64,), (4, 3)):
        x, arg = A.check_minmax(OPS, DEV, dtype, is_max, name, trailing)
        index = A.minmax_case(name, trailing, is_max)[1]
        _, got = _ext().scatter_minmax_fwd(x, put(index, DEV), N_SEG,
                                           is_max)
        assert torch.equal(got.cpu(), arg), f"arg {name} {trailing}"


@IS_MAX
@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.dtype_id)
def test_minmax_row_of_identity_values(dtype, is_max):
    """A non-empty row that is all -inf under max (all +inf under min)
    is not an empty row: the value is -+inf and the arg its first
    edge."""
    ident = float("-inf") if is_max else float("inf")
    index = torch.tensor([4, 2, 4, 2, 4, 7])
    src = torch.tensor([1.0, ident, 3.0, ident, -2.0, ident])
    src = src.view(-1, 1).expand(-1, 3).contiguous()
    out, arg = _ext().scatter_minmax_fwd(put(src, DEV, dtype),
                                         put(index, DEV), 9, is_max)
    want, want_arg = A.ref_minmax(src, index, 9, is_max)
    assert want[2, 0] == ident and want_arg[2, 0] == 1
    assert want[7, 0] == ident and want_arg[7, 0] == 5
    assert A.same(out, want, dtype)
    assert torch.equal(arg.cpu(), want_arg)


@IS_MAX
def test_minmax_second_grid_stride_iteration(is_max):
    g = A.gen("minmax_stride")
    index = torch.randint(0, N_SEG, (8200,), generator=g)
    src = A.ints(g, -8, 8, 8200, 64)
    assert src.numel() > CAP
    out, arg = _ext().scatter_minmax_fwd(put(src, DEV, F32),
                                         put(index, DEV), N_SEG, is_max)
    want, want_arg = A.ref_minmax(src, index, N_SEG, is_max)
    assert A.same(out, want, F32) and torch.equal(arg.cpu(), want_arg)


# ---------------------------------------------------------------------------
# empty and strided inputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.dtype_id)
def test_no_edges(dtype):
    A.check_empty_edges(OPS, DEV, dtype)


@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.dtype_id)
def test_strided_index_and_source(dtype):
    """`index` a column of an [E, 2] edge list, `src` a transposed
    view: both are read through their strides."""
    g = A.gen("strided")
    n_edges = 301
    pairs = torch.randint(2, 30, (n_edges, 2), generator=g)
    base = A.ints(g, -8, 8, 5, n_edges)
    index = put(pairs, DEV)[:, 1]
    src = put(base, DEV, dtype).t()
    assert not index.is_contiguous() and not src.is_contiguous()
    idx_c, src_c = pairs[:, 1].contiguous(), base.t().contiguous()
    assert A.same(scatter(src, index, N_SEG, "sum"),
                  A.ref_sum(src_c, idx_c, N_SEG), dtype)
    assert A.same(scatter(src, index, N_SEG, "max"),
                  A.ref_minmax(src_c, idx_c, N_SEG, True)[0], dtype)
    if dtype in WIDE:
        assert A.same(scatter(src, index, N_SEG, "mean"),
                      A.ref_mean(src_c, idx_c, N_SEG), dtype)
    table = put(base, DEV, dtype).t()[:30]
    assert torch.equal(gather(table, index).cpu(),
                       src_c.to(dtype)[:30][idx_c])


# ---------------------------------------------------------------------------
# autograd closure, segment_softmax
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["atomic", "backward_csr", "sorted"])
@pytest.mark.parametrize("dtype", WIDE, ids=A.dtype_id)
def test_autograd_closure(dtype, variant):
    A.check_closure(OPS, DEV, dtype, variant)


@pytest.mark.parametrize("dtype", WIDE, ids=A.dtype_id)
def test_segment_softmax(dtype):
    A.check_softmax(OPS, DEV, dtype)
