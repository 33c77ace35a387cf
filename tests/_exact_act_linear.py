"""Shared pieces of the act_linear tests (test_act_linear.py,
test_gpu_act_linear.py): the flagship differentiation pattern, the fp64
formulas of the activation and its derivatives, the exhaustive bf16 input
set and the bounds the tests hold the kernels to."""

import torch

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64


def ints(gen, lo, hi, *shape):
    """Seeded integers, uniform in [lo, hi], as fp64 on the CPU."""
    return torch.randint(lo, hi + 1, shape, generator=gen).to(F64)


# phi = silu and its derivatives, evaluated in the dtype of x
def phi(x):
    return x * torch.sigmoid(x)


def dphi(x):
    s = torch.sigmoid(x)
    # 1 - s as s(-x): exact where s rounds to 1
    return s * (1 + x * torch.sigmoid(-x))


def d2phi(x):
    s, t = torch.sigmoid(x), torch.sigmoid(-x)
    return s * t * (2 + x * (t - s))


def composition(h, W, b):
    return torch.nn.functional.linear(torch.nn.functional.silu(h), W, b)


def flagship(fn, h, W, b, r):
    """Forward, create_graph gradient with respect to h, backward of a
    scalar function of that gradient: -> (y, first-order grads of
    e = <y, r> w.r.t. (h, W, b), grads of e + |gh|^2 w.r.t. (h, W, b))."""
    y = fn(h, W, b)
    e = (y * r).sum()
    leaves = (h, W) if b is None else (h, W, b)
    first = torch.autograd.grad(e, leaves, retain_graph=True)
    (gh,) = torch.autograd.grad(e, h, create_graph=True)
    loss = e + (gh.to(F64 if gh.dtype == F64 else F32) ** 2).sum()
    second = torch.autograd.grad(loss, leaves, allow_unused=True)
    return y, first, second


def all_finite_bf16():
    """The 65,280 finite bf16 values."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    v = bits.view(BF)
    return v[torch.isfinite(v)]


def bf16_neighbours(p):
    """(next larger magnitude, next smaller magnitude) of bf16 p; zero
    and the largest finite value keep themselves."""
    bits = p.view(torch.int16).to(torch.int32)
    mag = bits & 0x7FFF
    up = torch.where(mag < 0x7F7F, bits + 1, bits)
    dn = torch.where(mag > 0, bits - 1, bits)
    return (up.to(torch.int16).view(BF), dn.to(torch.int16).view(BF))


def exhaustive_ok(got, ref, h, scale):
    """|got - ref| <= 2^-8 |ref| + 2^-20 max(1, |h|) |scale|: one bf16
    rounding, and 8x the error torch's own fp32 evaluation of 1 - sigma
    shows against fp64 over this input set."""
    got, ref = got.to(F64), ref.to(F64)
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * h.abs().clamp(min=1) \
        * abs(scale)
    return (got - ref).abs() <= bound


def random_bound(want, k_len, sum_abs):
    """2^-7 |want| + 2^-24 K' sum|a_i b_i|: two bf16 roundings that may
    disagree, and the fp32 accumulation-order term."""
    return 2.0 ** -7 * want.to(F64).abs() + 2.0 ** -24 * k_len * sum_abs
