"""The CPU paths of `scatter`, `gather` and `segment_softmax` against
the independent references of _exact_agg.py, no GPU.

The rest of the suite treats the CPU path as ground truth for the HIP
aggregation kernels, so it has to agree with a reference that does not
go through it: on empty rows, on E = 0 with trailing dims, on rows that
hold only the reduction's identity (-inf under max, +inf under min), on
ties and where their gradient goes, and on means.  Integer-valued
sources make every fp32/fp64 sum exact, so those comparisons are
`torch.equal`; the same cases and checks run on the device in
test_gpu_agg_exact.py.

bf16/f16 CPU sums go through `index_add_` in that precision and are not
exact by construction: half types are checked on min/max and gather
only.  NaN sources and out-of-range indices are unspecified and not
exercised.
"""

import types

import pytest
import torch

import _exact_agg as A
from hydragnn_amd.ops import gather, scatter, segment_softmax

OPS = types.SimpleNamespace(scatter=scatter, gather=gather,
                            segment_softmax=segment_softmax)
WIDE = [A.F32, A.F64]


# ---- the references themselves -------------------------------------------
def test_ordered_sum_reference_is_a_plain_loop():
    g = A.gen("ordered_ref")
    index = A.layout("gaps", g)
    for dtype in A.DTYPES:
        src = torch.randn(index.numel(), 3, generator=g).to(dtype)
        acc_t = A.F64 if dtype == A.F64 else A.F32
        want = torch.zeros(A.N_SEG, 3, dtype=acc_t)
        for e in range(index.numel()):
            want[index[e]] = want[index[e]] + src[e].to(acc_t)
        got = A.ref_ordered_sum(src, index, A.N_SEG)
        assert got.dtype == dtype and torch.equal(got, want.to(dtype))


def test_minmax_reference_tie_break_and_empty_rows():
    src = torch.tensor([1., 5., 5., -2., 5., -2.], dtype=A.F64)
    index = torch.tensor([2, 0, 2, 0, 0, 2])
    out, arg = A.ref_minmax(src, index, 4, True)
    assert out.tolist() == [5., 0., 5., 0.] and arg.tolist() == [1, -1, 2, -1]
    out, arg = A.ref_minmax(src, index, 4, False)
    assert out.tolist() == [-2., 0., -2., 0.]
    assert arg.tolist() == [3, -1, 5, -1]
    grad = A.ref_minmax_grad(arg, torch.tensor([3., 9., 4., 9.]), 6)
    assert grad.tolist() == [0., 0., 0., 3., 0., 4.]


def test_ulp_helper():
    ref = torch.tensor([1.0, 1.5, 3.0, 400.0, 0.0, 2.0 ** -20], dtype=A.F64)
    assert A.ulp(ref, A.BF).tolist() == [
        2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0, 2.0 ** -133, 2.0 ** -27]
    assert A.ulp(ref, A.F16).tolist() == [
        2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 0.25, 2.0 ** -24, 2.0 ** -24]


# ---- the CPU paths ---------------------------------------------------------
@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.dtype_id)
def test_gather(dtype):
    for trailing in A.TRAILING:
        A.check_gather(OPS, "cpu", dtype, trailing)


@pytest.mark.parametrize("name", A.LAYOUTS)
@pytest.mark.parametrize("dtype", WIDE, ids=A.dtype_id)
def test_sum(dtype, name):
    A.check_sum(OPS, "cpu", dtype, "atomic", name)


@pytest.mark.parametrize("dtype", WIDE, ids=A.dtype_id)
def test_mean_of_constant_segments(dtype):
    A.check_mean_const(OPS, "cpu", dtype, False)


@pytest.mark.parametrize("dtype", WIDE, ids=A.dtype_id)
def test_mean_is_correctly_rounded(dtype):
    A.check_mean_general(OPS, "cpu", dtype, False)


@pytest.mark.parametrize("name", A.LAYOUTS)
@pytest.mark.parametrize("is_max", [True, False], ids=["max", "min"])
@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.dtype_id)
def test_minmax_value_ties_inf_and_gradient(dtype, is_max, name):
    for trailing in ((), (3,), (4, 3)):
        A.check_minmax(OPS, "cpu", dtype, is_max, name, trailing)


@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.dtype_id)
def test_no_edges(dtype):
    A.check_empty_edges(OPS, "cpu", dtype)


@pytest.mark.parametrize("variant", ["atomic", "backward_csr", "sorted"])
@pytest.mark.parametrize("dtype", WIDE, ids=A.dtype_id)
def test_autograd_closure(dtype, variant):
    A.check_closure(OPS, "cpu", dtype, variant)


@pytest.mark.parametrize("dtype", WIDE, ids=A.dtype_id)
def test_segment_softmax(dtype):
    A.check_softmax(OPS, "cpu", dtype)
