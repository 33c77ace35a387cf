"""Fused SiLU -> Linear, activation first, closed under the two
differentiations of force training.

    act_linear(h[E, K], W[N, K], b[N] | None) -> y[E, N]
        y = silu(h) W^T + b

Five primitives (csrc/act_linear.hip) carry every order the flagship
produces; the activated tensor and the derivative of the activation are
never written to memory.  With phi(x) = x s(x), s the logistic function,
phi' = s (1 + x (1 - s)) and phi'' = s (1 - s)(2 + x (1 - 2 s)):

    act_linear      y[e,n]  = sum_k r(phi(h[e,k])) W[n,k] + b[n]
    dgrad           gh[e,k] = (sum_n g[e,n] W[n,k]) phi'(h[e,k])
    wgrad           gW[n,k] = sum_e g[e,n] p[e,k],  gb[n] = sum_e g[e,n]
                    p = r(phi(h)), or r(u phi'(h)) when u is given
    dgrad_dg        dg[e,n] = sum_k r(u[e,k] phi'(h[e,k])) W[n,k]
    dgrad_dh        dh[e,k] = u[e,k] (sum_n g[e,n] W[n,k]) phi''(h[e,k])

Sums and the activation run in the accumulator type (fp32 for bf16/f16,
the dtype itself otherwise); ``r`` rounds to the tensor dtype, and every
result is rounded once.  The same holds for the HIP kernels and for the
pure-torch doubles below, which serve CPU tensors,
``HYDRAGNN_AMD_FORCE_EAGER=1``, dtypes other than bf16 and shapes outside
the envelope.

Autograd: ``act_linear``'s backward is ``dgrad`` + ``wgrad``; ``dgrad`` is
a Function too, with backward ``dgrad_dg`` + ``dgrad_dh`` + ``wgrad(g, h,
u)``.  What the flagship never produces runs the doubles as differentiable
torch ops: a backward that is itself recorded (a cotangent that will
arrive on a weight or bias gradient; third order).

``HYDRAGNN_ACT_LINEAR=0`` restores the composition ``linear(silu(h))``.
No host sync anywhere; workspaces come from the torch allocator.
"""

from __future__ import annotations

import os

import torch

from ._extension import get_extension, use_eager

__all__ = ["act_linear", "fused_route", "in_envelope", "path_counts",
           "reset_path_counts"]

_counts = {"act_linear": 0, "dgrad": 0, "wgrad": 0, "dgrad_dg": 0,
           "dgrad_dh": 0, "composition": 0}


def path_counts() -> dict:
    """Kernel launches per primitive, and calls that ran a torch double
    or the unfused composition instead."""
    return dict(_counts)


def reset_path_counts() -> None:
    for k in _counts:
        _counts[k] = 0


def fused_route(default: bool = True) -> bool:
    """HYDRAGNN_ACT_LINEAR=0 restores the composition, any other value
    selects the fused route, unset leaves the default.  Read at call
    time."""
    value = os.environ.get("HYDRAGNN_ACT_LINEAR")
    return default if value is None else value != "0"


def in_envelope(E: int, N: int, K: int) -> bool:
    """Shapes the kernels serve (csrc/act_linear.hip checks the same)."""
    return (N % 64 == 0 and K % 64 == 0 and 64 <= N <= 320
            and 64 <= K <= 256 and E >= 256)


def _acc(dtype: torch.dtype) -> torch.dtype:
    return torch.float32 if dtype in (torch.bfloat16, torch.float16) \
        else dtype


# ---------------------------------------------------------------------------
# pure-torch doubles (differentiable)
# ---------------------------------------------------------------------------
def _phi(x):
    return x * torch.sigmoid(x)


def _dphi(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def _d2phi(x):
    s = torch.sigmoid(x)
    return s * (1 - s) * (2 + x * (1 - 2 * s))


def torch_act_linear(h, W, b=None):
    acc = _acc(h.dtype)
    p = _phi(h.to(acc)).to(h.dtype)
    y = p.to(acc) @ W.to(acc).t()
    if b is not None:
        y = y + b.to(acc)
    return y.to(h.dtype)


def torch_dgrad(g, W, h):
    acc = _acc(h.dtype)
    return ((g.to(acc) @ W.to(acc)) * _dphi(h.to(acc))).to(h.dtype)


def torch_wgrad(g, h, u=None, want_bias=False, act=True):
    acc = _acc(h.dtype)
    p = h.to(acc)
    if u is not None:
        p = u.to(acc) * _dphi(p)
    elif act:
        p = _phi(p)
    gW = (g.to(acc).t() @ p.to(h.dtype).to(acc)).to(h.dtype)
    gb = g.to(acc).sum(0).to(h.dtype) if want_bias else None
    return gW, gb


def torch_dgrad_dg(u, W, h):
    acc = _acc(h.dtype)
    p = (u.to(acc) * _dphi(h.to(acc))).to(h.dtype)
    return (p.to(acc) @ W.to(acc).t()).to(h.dtype)


def torch_dgrad_dh(u, g, W, h):
    acc = _acc(h.dtype)
    return (u.to(acc) * (g.to(acc) @ W.to(acc))
            * _d2phi(h.to(acc))).to(h.dtype)


# ---------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------
def _kernel_route(W, *tensors) -> bool:
    E = tensors[0].shape[0]
    return (not use_eager()
            and all(t.is_cuda and t.dtype == torch.bfloat16
                    for t in (W,) + tensors)
            and in_envelope(E, W.shape[0], W.shape[1]))


def _fwd(h, W, b):
    if _kernel_route(W, h) and (b is None or (
            b.is_cuda and b.dtype == torch.bfloat16)):
        _counts["act_linear"] += 1
        return get_extension(required=True).act_linear_fwd(
            h.contiguous(), W.contiguous(),
            None if b is None else b.contiguous())
    _counts["composition"] += 1
    return torch_act_linear(h, W, b)


def _dgrad(g, W, h):
    if _kernel_route(W, g, h):
        _counts["dgrad"] += 1
        return get_extension(required=True).act_linear_dgrad(
            g.contiguous(), W.contiguous(), h.contiguous())
    _counts["composition"] += 1
    return torch_dgrad(g, W, h)


def _wgrad(g, W, h, u, want_bias, recorded):
    """(gW, gb | None).  ``recorded``: the caller's backward is itself
    being recorded, so the result has to be differentiable."""
    tensors = (g, h) if u is None else (g, h, u)
    if not recorded and _kernel_route(W, *tensors):
        _counts["wgrad"] += 1
        gW, gb = get_extension(required=True).act_linear_wgrad(
            g.contiguous(), h.contiguous(),
            None if u is None else u.contiguous(), True, want_bias)
        return gW, (gb if want_bias else None)
    _counts["composition"] += 1
    return torch_wgrad(g, h, u, want_bias)


def _dgrad_dg(u, W, h, recorded):
    if not recorded and _kernel_route(W, u, h):
        _counts["dgrad_dg"] += 1
        return get_extension(required=True).act_linear_dgrad_dg(
            u.contiguous(), W.contiguous(), h.contiguous())
    _counts["composition"] += 1
    return torch_dgrad_dg(u, W, h)


def _dgrad_dh(u, g, W, h, recorded):
    if not recorded and _kernel_route(W, u, g, h):
        _counts["dgrad_dh"] += 1
        return get_extension(required=True).act_linear_dgrad_dh(
            u.contiguous(), g.contiguous(), W.contiguous(), h.contiguous())
    _counts["composition"] += 1
    return torch_dgrad_dh(u, g, W, h)


def _wanted(ctx, i: int) -> bool:
    """Whether this backward call has to produce the gradient of input i:
    ``needs_input_grad`` says only that the input requires grad, so a
    force pass (autograd.grad with respect to positions) would compute
    every weight gradient and throw it away."""
    if not ctx.needs_input_grad[i]:
        return False
    try:
        node = ctx.next_functions[i][0]
        return node is not None and \
            torch._C._will_engine_execute_node(node)
    except (RuntimeError, AttributeError):
        # the engine cannot say (a captured leaf under autograd.grad)
        return True


class _ActLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, W, b):
        ctx.save_for_backward(h, W)
        ctx.has_bias = b is not None
        return _fwd(h, W, b)

    @staticmethod
    def backward(ctx, g):
        h, W = ctx.saved_tensors
        g = g.to(h.dtype)
        gh = gW = gb = None
        if _wanted(ctx, 0):
            gh = _ActLinearDgrad.apply(g, W, h)
        need_b = ctx.has_bias and _wanted(ctx, 2)
        if _wanted(ctx, 1) or need_b:
            gW, gb = _wgrad(g, W, h, None, need_b,
                            torch.is_grad_enabled())
        return gh, gW, gb


class _ActLinearDgrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, W, h):
        ctx.save_for_backward(g, W, h)
        return _dgrad(g, W, h)

    @staticmethod
    def backward(ctx, u):
        g, W, h = ctx.saved_tensors
        u = u.to(h.dtype)
        recorded = torch.is_grad_enabled()
        dg = dW = dh = None
        if _wanted(ctx, 0):
            dg = _dgrad_dg(u, W, h, recorded)
        if _wanted(ctx, 1):
            dW, _ = _wgrad(g, W, h, u, False, recorded)
        if _wanted(ctx, 2):
            dh = _dgrad_dh(u, g, W, h, recorded)
        return dg, dW, dh


def act_linear(h: torch.Tensor, W: torch.Tensor, b=None) -> torch.Tensor:
    """silu(h) W^T + b for h [E, K], W [N, K], b [N] or None.  See the
    module docstring."""
    if h.dim() != 2 or W.dim() != 2 or h.shape[1] != W.shape[1]:
        raise ValueError(
            f"act_linear wants h [E, K] and W [N, K], got "
            f"{tuple(h.shape)} and {tuple(W.shape)}")
    if b is not None and b.shape != (W.shape[0],):
        raise ValueError(f"bias must be [{W.shape[0]}]")
    if not fused_route():
        _counts["composition"] += 1
        return torch.nn.functional.linear(
            torch.nn.functional.silu(h), W, b)
    return _ActLinear.apply(h, W, b)


act_linear.path_counts = path_counts
act_linear.reset_path_counts = reset_path_counts
