"""The weight-gradient kernel's route, flag and split, without a GPU."""

import pytest
import torch

from hydragnn_amd.ops import get_extension, splitk_linear
from hydragnn_amd.ops.splitk_linear import (SplitKLinear, wgrad_kernel_enabled,
                                            wgrad_paths, wgrad_route)


def test_flag_is_tri_state(monkeypatch):
    monkeypatch.delenv(splitk_linear.WGRAD_FLAG, raising=False)
    assert wgrad_kernel_enabled() is False
    assert wgrad_kernel_enabled(True) is True
    monkeypatch.setenv(splitk_linear.WGRAD_FLAG, "0")
    assert wgrad_kernel_enabled(True) is False
    monkeypatch.setenv(splitk_linear.WGRAD_FLAG, "1")
    assert wgrad_kernel_enabled(False) is True


def test_cpu_tensors_never_take_the_route(monkeypatch):
    monkeypatch.setenv(splitk_linear.WGRAD_FLAG, "1")
    monkeypatch.setattr(splitk_linear, "MIN_ROWS", 1)
    torch.manual_seed(0)
    lin = SplitKLinear(42, 8).double()
    x = torch.randn(300, 42, dtype=torch.float64, requires_grad=True)
    assert not wgrad_route(x, 8)
    wgrad_paths.reset()
    out = lin(x)
    assert out.grad_fn.name() == "AddmmBackward0"     # F.linear itself
    out.square().sum().backward()
    assert wgrad_paths.snapshot() == {"kernel": 0, "composition": 0}
    ref = torch.nn.functional.linear(x, lin.weight, lin.bias)
    assert torch.equal(out, ref)


@pytest.mark.parametrize("N,K", [(8, 42), (64, 64), (64, 192), (256, 256)])
def test_split_depends_on_shapes_alone(N, K):
    ext = get_extension(required=True)
    assert ext.linear_wgrad_chunks(0, N, K) == 0
    assert ext.linear_wgrad_chunks(0, K, N) == 0
    last = 0
    for E in [1, 255, 256, 257, 1000, 71372, 131072, 131073, 1197894,
              2 ** 31 - 1]:
        chunks = ext.linear_wgrad_chunks(E, N, K)
        rows = ext.linear_wgrad_chunk_rows(E, N, K)
        assert chunks == ext.linear_wgrad_chunks(E, N, K)
        assert chunks >= last and chunks >= 1
        assert rows >= 256 and chunks * rows >= E
        last = chunks
