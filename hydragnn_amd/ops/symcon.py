"""Fused MACE symmetric contraction.

The product block is a polynomial in the node features with per-element
weights.  With x~ = (x_0 .. x_{D-1}, 1) and W[e, p, c] the block's
weights concatenated over (lout, nu),

    out[n,c,o] = sum_k coef_k W[elem[n], p_k, c] x~[i_k] x~[j_k] x~[l_k]

with one entry per non-zero of each U^(nu); index D, the constant 1,
fills the slots a lower order leaves unused.  On the GPU the forward, the
first-order pass (Q = <g, out>: dQ/dx, dQ/dW) and the second-order pass
(R = <t_x, dQ/dx>: dR/dg, dR/dx, dR/dW) are one launch each
(csrc/symcon.hip); weight gradients are summed per element in a fixed
order over nodes sorted by element (`element_sort`).  `_dense_symcon` is
the pure-torch form: the CPU path, the fallback outside the kernels'
envelope, and the reference the tests differentiate.
"""

from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import torch

from ._extension import get_extension, use_eager
from .scatter import _rowptr_from_sorted

_KERNEL_DTYPES = (torch.float32, torch.bfloat16, torch.float64)
_LDS_BUDGET = 150 * 1024
MAX_D, MAX_P, MAX_ENTRIES = 9, 32, 1024

# how often each path ran (tests read this to see which one served)
symcon_stats = {"fwd": 0, "first": 0, "second": 0, "ref_first": 0,
                "ref_second": 0, "dense": 0}


def enabled() -> bool:
    """HYDRAGNN_SYMCON=0 keeps the modules on their composition."""
    return os.environ.get("HYDRAGNN_SYMCON", "1") != "0"


class SymconTable:
    """Entries (o, p, i, j, l, coef), sorted by o.  D input slots (slot
    D is the constant 1), Do outputs, P weights per (element, channel)."""

    def __init__(self, o, p, i, j, l, coef, D: int, Do: int, P: int):
        o, p, i, j, l = (torch.as_tensor(v, dtype=torch.long).reshape(-1)
                         for v in (o, p, i, j, l))
        coef = torch.as_tensor(coef, dtype=torch.float32).reshape(-1)
        order = torch.argsort(o, stable=True)
        self.o, self.p, self.i, self.j, self.l = (
            v[order].contiguous() for v in (o, p, i, j, l))
        self.coef = coef[order].contiguous()
        self.D, self.Do, self.P = int(D), int(Do), int(P)
        self.K = int(self.o.numel())
        if self.K:
            assert 0 <= int(self.o.min()) and int(self.o.max()) < self.Do
            assert 0 <= int(self.p.min()) and int(self.p.max()) < self.P
            for v in (self.i, self.j, self.l):
                assert 0 <= int(v.min()) and int(v.max()) <= self.D
        self._dev: Dict[Tuple, Tuple] = {}
        self._idx: Dict[Tuple, Tuple] = {}

    @property
    def in_envelope(self) -> bool:
        return (1 <= self.D <= MAX_D and 1 <= self.Do <= MAX_D
                and 1 <= self.P <= MAX_P and 1 <= self.K <= MAX_ENTRIES)

    def device_tensors(self, device):
        """Packed entry words (o | p<<4 | i<<10 | j<<14 | l<<18) and
        fp32 coefficients on `device`."""
        key = (device,)
        if key not in self._dev:
            assert self.in_envelope
            words = (self.o | self.p << 4 | self.i << 10 | self.j << 14
                     | self.l << 18).to(torch.int32)
            self._dev[key] = (words.to(device).contiguous(),
                              self.coef.to(device).contiguous())
        return self._dev[key]

    def index_tensors(self, device, dtype):
        key = (device, dtype)
        if key not in self._idx:
            self._idx[key] = tuple(
                v.to(device) for v in (self.o, self.p, self.i, self.j,
                                       self.l)) + (
                self.coef.to(device=device, dtype=dtype),)
        return self._idx[key]


def table_from_contractions(contractions) -> SymconTable:
    """Expand the U buffers of a SymmetricContraction's per-lout
    `Contraction` modules.  Weight index p runs over (lout, nu) in the
    order `concat_weights` concatenates the parameters."""
    D = None
    cols = [[] for _ in range(5)]
    coefs = []
    p_off = 0
    for con in contractions:
        o_off = con.lout * con.lout
        for nu in range(con.correlation, 0, -1):
            U = getattr(con, f"U{nu}").detach().cpu()
            D = U.shape[1] if D is None else D
            k = U.shape[-1]
            if k == 0:
                continue
            nz = U.nonzero()
            slots = [nz[:, 1 + s] if s < nu else
                     torch.full_like(nz[:, 0], D) for s in range(3)]
            cols[0].append(nz[:, 0] + o_off)
            cols[1].append(nz[:, -1] + p_off)
            for s in range(3):
                cols[2 + s].append(slots[s])
            coefs.append(U[tuple(nz.t())])
            p_off += k
    last = contractions[len(contractions) - 1]
    Do = (last.lout + 1) ** 2
    cat = [torch.cat(c) if c else torch.zeros(0, dtype=torch.long)
           for c in cols]
    coef = torch.cat(coefs) if coefs else torch.zeros(0)
    return SymconTable(*cat, coef, D, Do, max(p_off, 0))


def concat_weights(contractions, dtype) -> torch.Tensor:
    """W [nel, P, C]: the existing per-(lout, nu) parameters side by
    side; autograd splits its gradient back onto them."""
    ws = [con.weights[str(nu)] for con in contractions
          for nu in range(con.correlation, 0, -1)
          if con.weights[str(nu)].shape[1] > 0]
    return torch.cat(ws, dim=1).to(dtype)


def element_sort(elem: torch.Tensor, nel: int):
    """(perm, rowptr): nodes in element order and the row pointer of
    length nel+1.  No host sync, so a captured step can hold it."""
    perm = torch.argsort(elem, stable=True)
    return perm, _rowptr_from_sorted(elem[perm], nel)


def _dense_symcon(x, W, elem, table: SymconTable):
    """Pure-torch form; autograd differentiates it as often as asked."""
    N, C, _ = x.shape
    o, p, i, j, l, coef = table.index_tensors(x.device, x.dtype)
    xt = torch.cat([x, x.new_ones(N, C, 1)], dim=-1)
    Wn = W.index_select(0, elem)  # [N, P, C]
    terms = coef * Wn[:, p, :].transpose(1, 2) * xt[..., i] * \
        xt[..., j] * xt[..., l]  # [N, C, K]
    return x.new_zeros(N, C, table.Do).index_add(2, o, terms)


def kernel_ok(table: SymconTable, x: torch.Tensor,
              W: Optional[torch.Tensor] = None) -> bool:
    if not (x.is_cuda and x.dtype in _KERNEL_DTYPES and x.dim() == 3
            and table.in_envelope and x.shape[2] == table.D
            and not use_eager()):
        return False
    if W is not None and (W.dtype != x.dtype or not W.is_cuda):
        return False
    ext = get_extension(required=True)
    acc = 8 if x.dtype == torch.float64 else 4
    return max(ext.symcon_lds_bytes(table.D, table.Do, table.P, table.K,
                                    order, acc)
               for order in (0, 1, 2)) <= _LDS_BUDGET


def _up(*ts):
    """Half-precision operands go through the torch forms in fp32, so
    that they round once at the end, as the kernels do."""
    return tuple(t.float() if t is not None and t.dtype in (
        torch.bfloat16, torch.float16) else t for t in ts)


def _down(res, dtype):
    return tuple(None if r is None else r.to(dtype) for r in res)


def _ref_first(x, W, g, elem, table, mask):
    symcon_stats["ref_first"] += 1
    dtype = x.dtype
    x, W, g = _up(x, W, g)
    with torch.enable_grad():
        xd, Wd = x.detach().requires_grad_(True), \
            W.detach().requires_grad_(True)
        out = _dense_symcon(xd, Wd, elem, table)
        wanted = [v for v, m in zip((xd, Wd), mask) if m]
        res = list(torch.autograd.grad(out, wanted, g.detach()))
    return _down([res.pop(0) if m else None for m in mask], dtype)


def _ref_second(x, W, g, t_x, t_W, elem, table, mask):
    symcon_stats["ref_second"] += 1
    dtype = x.dtype
    x, W, g, t_x, t_W = _up(x, W, g, t_x, t_W)
    with torch.enable_grad():
        xd, Wd, gd = (v.detach().requires_grad_(True) for v in (x, W, g))
        out = _dense_symcon(xd, Wd, elem, table)
        gx, gW = torch.autograd.grad(out, (xd, Wd), gd, create_graph=True)
        R = 0
        if t_x is not None:
            R = R + (t_x.detach() * gx).sum()
        if t_W is not None:
            R = R + (t_W.detach() * gW).sum()
        wanted = [v for v, m in zip((xd, Wd, gd), mask) if m]
        res = list(torch.autograd.grad(R, wanted, allow_unused=True))
    return _down([res.pop(0) if m else None for m in mask], dtype)


def _bits(mask) -> int:
    return sum(1 << s for s, m in enumerate(mask) if m)


def _first(x, W, g, elem, perm, rowptr, table, mask):
    """(dQ/dx, dQ/dW) on the mask, Q = <g, out>."""
    if not any(mask):
        return (None, None)
    if not kernel_ok(table, x, W):
        return _ref_first(x, W, g, elem, table, mask)
    symcon_stats["first"] += 1
    ext = get_extension(required=True)
    ent, coef = table.device_tensors(x.device)
    outs = ext.symcon_grad(x.contiguous(), g.contiguous(), None,
                           W.contiguous(), perm, rowptr, ent, coef,
                           _bits(mask))
    return tuple(outs)


def _second(x, W, g, t_x, t_W, elem, perm, rowptr, table, mask):
    """(dR/dx, dR/dW, dR/dg) on the mask, R = <t_x, dQ/dx> +
    <t_W, dQ/dW>.  The kernel serves training's case, t_W absent."""
    if not any(mask) or (t_x is None and t_W is None):
        return (None, None, None)
    if t_W is not None or not kernel_ok(table, x, W):
        return _ref_second(x, W, g, t_x, t_W, elem, table, mask)
    symcon_stats["second"] += 1
    ext = get_extension(required=True)
    ent, coef = table.device_tensors(x.device)
    outs = ext.symcon_grad(x.contiguous(), g.contiguous(),
                           t_x.contiguous(), W.contiguous(), perm, rowptr,
                           ent, coef, _bits(mask))
    return tuple(outs)


class _SymconGrad(torch.autograd.Function):
    """(x, W, g) -> (dQ/dx, dQ/dW) on the mask.  Its backward is the
    second-order pass with the incoming cotangents as tangents."""

    @staticmethod
    def forward(ctx, x, W, g, elem, perm, rowptr, table, mask):
        ctx.save_for_backward(x, W, g, elem, perm, rowptr)
        ctx.table = table
        ctx.set_materialize_grads(False)
        return _first(x, W, g, elem, perm, rowptr, table, mask)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, t_x, t_W):
        x, W, g, elem, perm, rowptr = ctx.saved_tensors
        mask = tuple(ctx.needs_input_grad[:3])
        return _second(x, W, g, t_x, t_W, elem, perm, rowptr, ctx.table,
                       mask) + (None,) * 5


class _SymconFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, elem, perm, rowptr, table):
        ctx.save_for_backward(x, W, elem, perm, rowptr)
        ctx.table = table
        ctx.set_materialize_grads(False)
        if kernel_ok(table, x, W):
            symcon_stats["fwd"] += 1
            ext = get_extension(required=True)
            ent, coef = table.device_tensors(x.device)
            return ext.symcon_forward(x.contiguous(), elem,
                                      W.contiguous(), ent, coef, table.Do)
        return _dense_symcon(x, W, elem, table)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 6
        x, W, elem, perm, rowptr = ctx.saved_tensors
        mask = tuple(ctx.needs_input_grad[:2])
        if not any(mask):
            return (None,) * 6
        gx, gW = _SymconGrad.apply(x, W, g, elem, perm, rowptr, ctx.table,
                                   mask)
        return gx, gW, None, None, None, None


def symcon(x: torch.Tensor, W: torch.Tensor, elem: torch.Tensor,
           table: SymconTable, elem_csr=None) -> torch.Tensor:
    """x [N, C, D], W [nel, P, C], elem [N] -> out [N, C, Do].
    `elem_csr` is `element_sort(elem, nel)`, built here when absent."""
    if not kernel_ok(table, x, W):
        symcon_stats["dense"] += 1
        return _dense_symcon(x, W, elem, table)
    if elem_csr is None:
        elem_csr = element_sort(elem, W.shape[0])
    perm, rowptr = elem_csr
    return _SymconFn.apply(x, W, elem.contiguous(), perm.contiguous(),
                           rowptr.contiguous(), table)
