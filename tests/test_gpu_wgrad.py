"""The tall-skinny weight-gradient kernels (csrc/wgrad.hip) on the GPU:
gW = g^T x and gb = g.sum(0) against the fp64 CPU product.

Exact cases: integers in [-4, 4], so every partial sum is an integer below
2^24 that every accumulator holds exactly: the result is known bit for bit
whatever the order.  General values: any order of E terms stays within
gamma_E sum|g||x|, gamma_E = E u / (1 - E u), u the accumulator's unit
roundoff (Higham, Accuracy and Stability, eq. 3.5).  Models: fp64 against
the CPU, 1e-12 as in test_gpu_gather_mul.
"""

import copy
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact_gather_mul as X  # noqa: E402
from _exact_linear import ints  # noqa: E402
from hydragnn_amd.ops import get_extension, splitk_linear  # noqa: E402
from hydragnn_amd.ops.splitk_linear import (SplitKLinear,  # noqa: E402
                                            wgrad_paths)

DEV = torch.device("cuda:0")
F64 = torch.float64
DTYPES = [torch.float64, torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(1, 1), (8, 42), (64, 8), (17, 33), (64, 64), (64, 192), (256, 256)]
ext = get_extension(required=True)


def acc_of(dtype):
    return dtype if dtype in (torch.float64, torch.float32) else torch.float32


def rows_of(case, N, K):
    """E of a named case, from the split the extension reports."""
    chunk = ext.linear_wgrad_chunk_rows(1, N, K)
    E = {"chunk": chunk, "chunk-1": chunk - 1, "chunk+1": chunk + 1,
         "ragged": 3 * chunk + 37}.get(case, case)
    want = {"chunk": 1, "chunk-1": 1, "chunk+1": 2, "ragged": 4}.get(case)
    if want is not None:
        assert ext.linear_wgrad_chunks(E, N, K) == want
    return E


def check_exact(g, x, g_dev, x_dev, dtype):
    gW, gb = ext.linear_wgrad(g_dev, x_dev, True)
    assert gW.dtype == gb.dtype == acc_of(dtype)
    assert torch.equal(gW.cpu().double(), g.t() @ x)
    assert torch.equal(gb.cpu().double(), g.sum(0))
    assert ext.linear_wgrad(g_dev, x_dev, False)[1].numel() == 0


@pytest.mark.parametrize("case", [0, 1, 3, 5, "chunk", "chunk-1", "chunk+1",
                                  "ragged"])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact(dtype, N, K, case):
    E = rows_of(case, N, K)
    gen = torch.Generator().manual_seed(1000 * N + K)
    g, x = ints(gen, -4, 4, E, N), ints(gen, -4, 4, E, K)
    check_exact(g, x, g.to(DEV, dtype), x.to(DEV, dtype), dtype)


@pytest.mark.parametrize("N,K", [(17, 33), (6, 43)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_views(dtype, N, K):
    """Row 1 onward of larger buffers starts off a 16-byte boundary (an
    odd width is no multiple of 16 bytes in any dtype); column slices of
    wider buffers are not contiguous."""
    E = rows_of("ragged", N, K)
    gen = torch.Generator().manual_seed(7)
    g, x = ints(gen, -4, 4, E + 1, N + 3), ints(gen, -4, 4, E + 1, K + 3)
    gd = g[:, :N].contiguous().to(DEV, dtype)
    xd = x[:, :K].contiguous().to(DEV, dtype)
    assert gd[1:].data_ptr() % 16 or xd[1:].data_ptr() % 16
    assert gd[1:].is_contiguous()
    check_exact(g[1:, :N], x[1:, :K], gd[1:], xd[1:], dtype)
    gd, xd = g.to(DEV, dtype)[:, 3:], x.to(DEV, dtype)[:, 3:]
    assert not gd.is_contiguous()
    check_exact(g[:, 3:], x[:, 3:], gd, xd, dtype)


@pytest.mark.parametrize("N,K", [(64, 64), (8, 42)])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_general_values(dtype, N, K):
    E = 3000
    gen = torch.Generator().manual_seed(3)
    g = torch.randn(E, N, generator=gen, dtype=dtype)
    x = torch.randn(E, K, generator=gen, dtype=dtype)
    gW, gb = ext.linear_wgrad(g.to(DEV), x.to(DEV), True)
    g64, x64 = g.double(), x.double()
    u = torch.finfo(dtype).eps / 2
    gamma = E * u / (1 - E * u)
    err_w = (gW.cpu().double() - g64.t() @ x64).abs()
    err_b = (gb.cpu().double() - g64.sum(0)).abs()
    bound_w = gamma * (g64.abs().t() @ x64.abs())
    bound_b = gamma * g64.abs().sum(0)
    print(f"worst error over bound: gW {float((err_w / bound_w).max()):.3e} "
          f"gb {float((err_b / bound_b).max()):.3e}")
    assert bool((err_w <= bound_w).all()) and bool((err_b <= bound_b).all())
    gW2, gb2 = ext.linear_wgrad(g.to(DEV), x.to(DEV), True)
    assert torch.equal(gW, gW2) and torch.equal(gb, gb2)


def force_chain(lin, x, v):
    """d/d(weight, bias, x) of |d e / d x|^2, e = sum(v tanh(lin(x)))."""
    e = (torch.tanh(lin(x)) * v).sum()
    (dx,) = torch.autograd.grad(e, x, create_graph=True)
    return torch.autograd.grad((dx ** 2).sum(), [lin.weight, lin.bias, x])


@pytest.mark.parametrize("flag", ["1", "0"])
def test_splitk_linear_force_chain(monkeypatch, flag):
    monkeypatch.setenv(splitk_linear.WGRAD_FLAG, flag)
    monkeypatch.setattr(splitk_linear, "MIN_ROWS", 1)
    E, K, N = 3 * 256 + 37, 42, 8
    gen = torch.Generator().manual_seed(5)
    lin = SplitKLinear(K, N).double()
    x = torch.randn(E, K, generator=gen, dtype=F64).requires_grad_(True)
    v = torch.randn(E, N, generator=gen, dtype=F64)
    ref = force_chain(lin, x, v)
    wgrad_paths.reset()
    got = force_chain(copy.deepcopy(lin).to(DEV),
                      x.detach().to(DEV).requires_grad_(True), v.to(DEV))
    counts = wgrad_paths.snapshot()
    if flag == "1":
        assert counts["kernel"] > 0 and counts["composition"] == 0, counts
    else:
        assert counts["kernel"] == 0, counts
    for a, b in zip(got, ref):
        err = float((a.cpu() - b).abs().max() / b.abs().max())
        print(f"relative error {err:.3e}")
        assert err <= 1e-12


def test_dimenet_fp64_matches_the_cpu_model_and_reruns(monkeypatch):
    """The fixture of test_gpu_gather_mul: three periodic cells of 27
    atoms.  Two blocks of 16 edge-row or triplet-row layers and the
    embedding's two make 34; the first block's output layer feeds node
    features that the second block does not read, so 33 have a weight
    gradient.  MIN_ROWS sits between the 81 atoms and the edges: the five
    linears of the graph head (3 rows) keep the composition."""
    from hydragnn_amd.models.dimenet import RowLinear
    from hydragnn_amd.utils.datasets.synthetic import lj_dataset
    from hydragnn_amd.data import Batch
    dataset = lj_dataset(num_samples=3, num_atoms=27, cell_size=6.1,
                         radius=3.0, pbc=True, seed=31, dtype=F64)
    model = X.build_model("DimeNet", dataset, mlip=False,
                          radius=3.0).double().train()
    assert sum(isinstance(m, RowLinear) for m in model.modules()) == 34

    def batch():
        return Batch.from_data_list([d.clone() for d in dataset])

    ref_out, ref_grads = X.graph_step(copy.deepcopy(model), batch())
    monkeypatch.setenv(splitk_linear.WGRAD_FLAG, "1")
    monkeypatch.setattr(splitk_linear, "MIN_ROWS", 256)
    assert sum(d.edge_index.shape[1] for d in dataset) > 1000
    dev_model = copy.deepcopy(model).to(DEV)
    wgrad_paths.reset()
    out, grads = X.graph_step(dev_model, batch().to(DEV))
    assert wgrad_paths.snapshot() == {"kernel": 33, "composition": 5}
    e_out, e_grad = X.rel_err(out, ref_out), X.rel_err(grads, ref_grads)
    print(f"DimeNet fp64 vs the CPU model: outputs {e_out:.3e} "
          f"gradients {e_grad:.3e}")
    assert set(grads) == set(ref_grads)
    assert e_out <= 1e-12 and e_grad <= 1e-12
    out2, grads2 = X.graph_step(dev_model, batch().to(DEV))
    for a, c in zip(out, out2):
        assert torch.equal(a, c)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k
