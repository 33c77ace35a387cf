"""Shared pieces of the exact-arithmetic tests of the bf16 linear family
(test_linear_autograd_closure.py, test_gpu_linear_exact.py).

With small integer-valued bf16 operands every product and every fp32
partial sum is an exactly representable integer, whatever the order of
accumulation; the only rounding is the final round-to-nearest-even
store to bf16.  The right answer is then known bit for bit from an fp64
reference: the tolerance is zero, and it is derived, not measured.
"""

import torch

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64

# LDS a workgroup may use: 160 KiB less the irreps kernels' static
# 64 B lmap table
LDS_MAX = 160 * 1024 - 64


# host envelopes, restated from the C++ checks (independent of ops/)
def fwd_envelope(c_in, c_out, d, n_l):
    """`irreps_linear`, either trans_w: [*, c_in, d] -> c_out."""
    lds = (d * 32 * (c_in + 8) + n_l * c_in * (c_out + 8)) * 2
    return (c_in % 32 == 0 and c_out % 64 == 0 and d <= 16
            and lds <= LDS_MAX)


def gw_envelope(c_in, c_out, d, n_l):
    """`irreps_linear_gw`: x [*, c_in, d], g [*, c_out, d]."""
    tiles = (c_in // 16) * (c_out // 16)
    lds = (d * 32 * (c_in + 8) + d * 32 * (c_out + 8)) * 2
    return (c_in % 16 == 0 and c_out % 16 == 0 and tiles % 4 == 0
            and tiles <= 16 and n_l <= 4 and d <= 16
            and lds <= LDS_MAX)


def ints(gen, lo, hi, *shape):
    """Seeded integers, uniform in [lo, hi], as fp64 on the CPU."""
    return torch.randint(lo, hi + 1, shape, generator=gen).to(F64)


def leaf(t, dtype, device="cpu"):
    return t.to(device=device, dtype=dtype).requires_grad_(True)


def lmap_for(lmax):
    return torch.cat([torch.full((2 * l + 1,), l, dtype=torch.long)
                      for l in range(lmax + 1)])


def same(got, ref, store=BF):
    """Bit equality with the fp64 reference after the route's final
    store (bf16 unless stated)."""
    assert got is not None, "gradient is missing"
    assert ref.abs().max() < 2 ** 24
    want = ref.detach().to(F32).to(store)
    got = got.detach().cpu()
    return got.shape == want.shape and torch.equal(got.to(store), want)


def sparse_rows(t, rows):
    out = torch.zeros_like(t)
    out[rows] = t[rows]
    return out


def irreps_formula(x, W, lmap, bias=None, add=None):
    """out[n,o,m] = sum_i x[n,i,m] W[lmap[m],i,o] (+ bias on m = 0,
    + residual)."""
    out = torch.einsum("nim,mio->nom", x, W[lmap])
    if bias is not None:
        out = torch.cat([out[:, :, :1] + bias.view(1, -1, 1),
                         out[:, :, 1:]], dim=-1)
    return out if add is None else out + add


def splitk_partials_exact(a, b):
    """Every per-chunk a^T b of `_splitk_weight_grad`'s split is an
    integer bf16 holds exactly, and so is their sum in any order."""
    E = a.shape[0]
    S = min(64, max(1, E // 256))
    pad = (S - E % S) % S
    a = torch.nn.functional.pad(a, (0, 0, 0, pad)).view(S, -1, a.shape[1])
    b = torch.nn.functional.pad(b, (0, 0, 0, pad)).view(S, -1, b.shape[1])
    parts = torch.bmm(a.transpose(1, 2), b)
    return bool(parts.abs().sum(0).max() <= 256)


def fold_exact(a, b, lmap):
    """The per-m a^T b over rows are integers bf16 holds exactly, and
    so is their fold m -> l in any order of accumulation."""
    gw_m = torch.einsum("nim,nom->mio", a, b).abs()
    fold = torch.zeros(int(lmap.max()) + 1, *gw_m.shape[1:],
                       dtype=gw_m.dtype).index_add_(0, lmap, gw_m)
    return bool(fold.max() <= 256)
