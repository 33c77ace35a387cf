"""Generalized equivariant tensor-product contraction (ETP).

The primitive:  out[i, c, o] = sum_k coef_k A[i,c,a_k] B[i,b_k] C[i,c,g_k]
with a small constant entry table — covers the MACE edge tensor product
(A = gathered node feats, B = spherical harmonics, C = radial-MLP path
weights), its gradients, and the symmetric-contraction fold steps.

Key property: gradients of a trilinear form are trilinear forms with
role-permuted tables, and the channel-reduced B-gradient closes the
family.  So both autograd passes of force training (create_graph=True)
run on the fused HIP kernels (csrc/etp.hip); CPU uses a dense-einsum
path that autograd differentiates directly.  The backward passes run
as sweeps: one launch yields every wanted first derivative, and one
more the whole second-order contribution (see "Sweep family" below).
A table that is exactly one of the compiled-in ones (etp_static.py)
runs its forward and sweeps on the static-table kernels
(csrc/etp_static.hip, HYDRAGNN_ETP_STATIC) at 64 channels.
"""

from __future__ import annotations

import os
from typing import Dict, Tuple

import torch

from ._extension import get_extension, use_eager
from .scatter import _rowptr_from_sorted

_KERNEL_DTYPES = (torch.float32, torch.bfloat16, torch.float16,
                  torch.float64)


class ETPTable:
    """Entry table (a, b, g, o, coef) with dims (da, db, dg, do).
    Role permutations and device copies are cached."""

    def __init__(self, entries: torch.Tensor, coefs: torch.Tensor,
                 dims: Tuple[int, int, int, int]):
        assert entries.dim() == 2 and entries.shape[1] == 4
        self.entries = entries.to(torch.int64).cpu()
        self.coefs = coefs.to(torch.float32).cpu()
        self.dims = tuple(int(d) for d in dims)
        self._perm_cache: Dict[str, "ETPTable"] = {}
        self._dev_cache: Dict[Tuple, Tuple] = {}
        self._dense_cache: Dict[Tuple, torch.Tensor] = {}
        self._static_id = None

    @property
    def static_id(self) -> int:
        """Id of the compile-time table (csrc/etp_static_tables.inc)
        this table equals exactly, -1 if none.  Resolved once, on the
        CPU copies; a permuted table from perm() resolves its own."""
        if self._static_id is None:
            from .etp_static import lookup
            self._static_id = lookup(self.entries, self.coefs, self.dims)
        return self._static_id

    def perm(self, order: str) -> "ETPTable":
        """order: 4-char permutation of 'abgo' giving the new roles,
        e.g. 'obga' swaps A <-> out (the A-gradient table)."""
        if order in self._perm_cache:
            return self._perm_cache[order]
        col = {"a": 0, "b": 1, "g": 2, "o": 3}
        idx = [col[ch] for ch in order]
        ent = self.entries[:, idx].contiguous()
        dims = tuple(self.dims[i] for i in idx)
        t = ETPTable(ent, self.coefs, dims)
        self._perm_cache[order] = t
        return t

    def device_tensors(self, device):
        """(entries int32 [n, 4], coefs fp32 [n]) on `device`, stably
        sorted by output slot: this is the kernels' summation order."""
        key = (device,)
        if key in self._dev_cache:
            return self._dev_cache[key]
        order = torch.argsort(self.entries[:, 3], stable=True)
        ent = self.entries[order].to(torch.int32)
        coefs = self.coefs[order]
        out = (ent.to(device).contiguous(),
               coefs.to(device).contiguous())
        self._dev_cache[key] = out
        return out

    def dense(self, device, dtype) -> torch.Tensor:
        key = (device, dtype)
        if key in self._dense_cache:
            return self._dense_cache[key]
        da, db, dg, do = self.dims
        W = torch.zeros(da, db, dg, do, dtype=dtype, device=device)
        e = self.entries
        W[e[:, 0], e[:, 1], e[:, 2], e[:, 3]] = \
            self.coefs.to(dtype).to(device)
        self._dense_cache[key] = W
        return W


def _dense_general(A, B, C, table: ETPTable):
    W = table.dense(A.device, torch.float32).to(A.dtype)
    return torch.einsum("eca,eb,ecg,abgo->eco", A, B, C, W)


_LDS_BUDGET = 150 * 1024


def _on_kernels(t: torch.Tensor) -> bool:
    """Device, dtype and mode conditions of the whole family; CPU
    tensors never reach the extension."""
    return t.is_cuda and t.dtype in _KERNEL_DTYPES and not use_eager()


def _form_fits(table: ETPTable, t, b_out: bool, staged: bool) -> bool:
    """The single-output form's LDS footprint (csrc/etp.hip,
    etp_form_lds_bytes: the launcher's own block size; fp64 slices are
    8 bytes) against the family's budget."""
    ext = get_extension(required=True)
    return ext.etp_form_lds_bytes(
        *table.dims, table.entries.shape[0],
        8 if t.dtype == torch.float64 else 4, b_out, staged) <= _LDS_BUDGET


def _kernel_ok(table: ETPTable, *tensors) -> bool:
    """Whether the o-type form takes this launch; the dense path takes
    it otherwise.  This predicate gates the whole family (folds,
    sweeps): over the staged footprint nothing of it runs."""
    t = tensors[0]
    return (_on_kernels(t)
            and all(x.dtype == t.dtype for x in tensors
                    if torch.is_tensor(x))
            and max(table.dims) <= 192
            and _form_fits(table, t, b_out=False, staged=True))


def _reduce_ok(table: ETPTable, t) -> bool:
    """Whether the b-type form takes this launch: staged within the
    budget, else (chosen in the extension) on the instance that reads
    its operands through L1 and keeps only the accumulator in LDS."""
    return (_on_kernels(t) and table.dims[1] <= 12
            and _form_fits(table, t, b_out=True, staged=False))


# ---------------------------------------------------------------------------
# Sweep family.  The contraction is one quadrilinear form
#   Q(a, b, g, o) = sum_k coef_k a[a_k] b[b_k] g[g_k] o[o_k]
# (a, g, o: [rows, nch, d]; b: [rows, db]) and every kernel above is
# dQ/dslot.  A sweep produces several of these derivatives in one walk
# of the entry table with every row staged once (csrc/etp.hip,
# etp_sweep_kernel), instead of one single-output launch per derivative
# plus the adds that sum second-order contributions.
# ---------------------------------------------------------------------------
_SLOTS = "abgo"
_SLOT_SUB = {"a": "eca", "b": "eb", "g": "ecg", "o": "eco"}

# how often each path ran (tests read this to see a fallback happen)
sweep_stats = {"sweep1": 0, "sweep2": 0, "compose1": 0, "compose2": 0}


_STATIC_DTYPES = (torch.float32, torch.bfloat16)


def _static_id(table: ETPTable) -> int:
    """HYDRAGNN_ETP_STATIC (default 1): 0 keeps every launch on the
    run-time-table kernels."""
    if os.environ.get("HYDRAGNN_ETP_STATIC", "1") == "0":
        return -1
    return table.static_id


def _static_applies(table: ETPTable, a, order: int, omask: int,
                    tmask: int) -> bool:
    """Whether csrc/etp_static.hip takes this launch: a compile-time
    table, 64 channels, bf16/fp32, and an instantiated (order, omask,
    tmask).  The same conditions decide in the extension."""
    sid = _static_id(table)
    if sid < 0 or a.shape[1] != 64 or a.dtype not in _STATIC_DTYPES:
        return False
    return get_extension(required=True).etp_static_supported(
        sid, order, omask, tmask)


def path_counts() -> Dict[str, int]:
    """Launches of etp_general / etp_sweep so far on the static-table
    kernels and on the run-time-table kernels (tests read the deltas
    to see which path ran)."""
    s, g = get_extension(required=True).etp_path_counts()
    return {"static": s, "generic": g}


def _sweep_mode() -> int:
    """HYDRAGNN_ETP_SWEEP: 0 = single-output kernels only, 1 = fused
    first-order backward, 2 = fused first- and second-order (default)."""
    v = os.environ.get("HYDRAGNN_ETP_SWEEP", "2")
    return int(v) if v in ("0", "1", "2") else 2


def _dense_dq(slots, s: int, W):
    """dQ/dslot_s as a dense einsum over the other three slots."""
    others = [r for r in range(4) if r != s]
    expr = ",".join(_SLOT_SUB[_SLOTS[r]] for r in others) + \
        ",abgo->" + _SLOT_SUB[_SLOTS[s]]
    return torch.einsum(expr, *[slots[r] for r in others], W)


def _dense_sweep(primals, tangents, mask, table: ETPTable):
    """Pure-torch reference of the sweep kernels.

    primals: (a, b, g, o) slot tensors.  mask: four bools, the wanted
    output slots.  tangents None -> first order: out_s = dQ/ds.
    Otherwise a 4-tuple with None for absent tangents -> second order:
    out_s = sum over r != s with t_r present of dQ/ds with slot r
    replaced by t_r.  Returns a 4-tuple, None outside the mask (and for
    a second-order slot that no present tangent reaches)."""
    W = table.dense(primals[0].device, torch.float32).to(primals[0].dtype)
    outs = []
    for s in range(4):
        if not mask[s]:
            outs.append(None)
        elif tangents is None:
            outs.append(_dense_dq(primals, s, W))
        else:
            acc = None
            for r in range(4):
                if r == s or tangents[r] is None:
                    continue
                slots = list(primals)
                slots[r] = tangents[r]
                term = _dense_dq(slots, s, W)
                acc = term if acc is None else acc + term
            outs.append(acc)
    return tuple(outs)


def _single_dq(slots, s: int, table: ETPTable):
    """dQ/dslot_s through the single-output kernels."""
    a, b, g, o = slots
    if s == 0:
        return etp_general(o, b, g, table.perm("obga"))
    if s == 1:
        return etp_reduce(a, g, o, table)
    if s == 2:
        return etp_general(a, b, o, table.perm("abog"))
    return etp_general(a, b, g, table)


def _compose_second(primals, tangents, mask, table: ETPTable):
    """Second-order sweep as single-output launches plus adds."""
    outs = []
    for s in range(4):
        acc = None
        if mask[s]:
            for r in range(4):
                if r == s or tangents[r] is None:
                    continue
                slots = list(primals)
                slots[r] = tangents[r]
                term = _single_dq(slots, s, table)
                acc = term if acc is None else acc + term
        outs.append(acc)
    return tuple(outs)


def _bits(flags) -> int:
    return sum(1 << s for s in range(4) if flags[s])


def _sweep_fits(table: ETPTable, primals, tangents, mask) -> bool:
    """Kernel dtype/device conditions plus the sweep's own LDS
    footprint: block x (input + tangent + output rows) x accumulator
    size + table, against the family's 150 KiB budget.  A launch the
    static-table kernel takes uses no LDS and always fits."""
    if not _kernel_ok(table, *primals):
        return False
    tmask = 0 if tangents is None else _bits(
        [t is not None for t in tangents])
    if _static_applies(table, primals[0], 1 if tangents is None else 2,
                       _bits(mask), tmask):
        return True
    acc = 8 if primals[0].dtype == torch.float64 else 4
    da, db, dg, do = table.dims
    ext = get_extension(required=True)
    return ext.etp_sweep_lds_bytes(
        da, db, dg, do, table.entries.shape[0], tmask, _bits(mask),
        acc) <= _LDS_BUDGET


def etp_sweep(primals, tangents, mask, table: ETPTable):
    """Sweep on the HIP kernel where it applies, `_dense_sweep`
    elsewhere (CPU, forced eager, unsupported dtypes, over budget).
    Not differentiable by itself: `_ETPSweep1` carries the autograd."""
    primals = tuple(primals)
    assert tuple(primals[0].shape[2:]) == (table.dims[0],) and \
        primals[1].shape[1] == table.dims[1] and \
        primals[2].shape[2] == table.dims[2] and \
        primals[3].shape[2] == table.dims[3], "slot dims vs table"
    if tangents is not None:
        tangents = tuple(tangents)
        # a slot reached by no present tangent is identically zero
        mask = tuple(bool(mask[s]) and any(
            tangents[r] is not None for r in range(4) if r != s)
            for s in range(4))
    if not any(mask):
        return (None, None, None, None)
    if not _sweep_fits(table, primals, tangents, mask):
        return _dense_sweep(primals, tangents, mask, table)
    ext = get_extension(required=True)
    ent, coefs = table.device_tensors(primals[0].device)
    tang = [None] * 4 if tangents is None else [
        None if t is None else t.contiguous() for t in tangents]
    outs = ext.etp_sweep(*[p.contiguous() for p in primals], *tang,
                         ent, coefs, _bits(mask),
                         1 if tangents is None else 2, _static_id(table))
    return tuple(outs)


class _ETPSweep1(torch.autograd.Function):
    """(a, b, g, o) -> (dQ/da, dQ/db, dQ/dg, dQ/do) on the masked
    slots (None elsewhere), one launch.  Its backward is the
    second-order sweep with the incoming cotangents as tangents."""

    @staticmethod
    def forward(ctx, a, b, g, o, table, mask):
        ctx.save_for_backward(a, b, g, o)
        ctx.table = table
        ctx.set_materialize_grads(False)
        sweep_stats["sweep1"] += 1
        return etp_sweep((a, b, g, o), None, mask, table)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *tangents):
        primals = ctx.saved_tensors
        table = ctx.table
        mask = tuple(ctx.needs_input_grad[:4])
        if _kernel_ok(table, *primals) and not (
                _sweep_mode() >= 2
                and _sweep_fits(table, primals, tangents, mask)):
            # first-order-only mode, or over the LDS budget
            sweep_stats["compose2"] += 1
            outs = _compose_second(primals, tangents, mask, table)
        else:
            sweep_stats["sweep2"] += 1
            outs = etp_sweep(primals, tangents, mask, table)
        return outs + (None, None)


def _first_order(primals, mask, table: ETPTable):
    """Masked first derivatives of Q: one sweep launch when enabled and
    within the LDS budget, else None (caller composes single-output
    kernels, as before the sweep family)."""
    if _sweep_mode() >= 1 and any(mask) and \
            _sweep_fits(table, primals, None, mask):
        return _ETPSweep1.apply(*primals, table, tuple(mask))
    sweep_stats["compose1"] += 1
    return None


class _ETPGeneral(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, C, table):
        ctx.save_for_backward(A, B, C)
        ctx.table = table
        ext = get_extension(required=True)
        ent, coefs = table.device_tensors(A.device)
        return ext.etp_general(A.contiguous(), B.contiguous(),
                               C.contiguous(), ent, coefs,
                               table.dims[3], static_id=_static_id(table))

    @staticmethod
    def backward(ctx, gout):
        A, B, C = ctx.saved_tensors
        table = ctx.table
        gout = gout.contiguous()
        mask = tuple(ctx.needs_input_grad[:3]) + (False,)
        swept = _first_order((A, B, C, gout), mask, table)
        if swept is not None:
            return swept[0], swept[1], swept[2], None
        gA = gB = gC = None
        if ctx.needs_input_grad[0]:
            gA = etp_general(gout, B, C, table.perm("obga"))
        if ctx.needs_input_grad[1]:
            gB = etp_reduce(A, C, gout, table)
        if ctx.needs_input_grad[2]:
            gC = etp_general(A, B, gout, table.perm("abog"))
        return gA, gB, gC, None


class _ETPReduce(torch.autograd.Function):
    """out[e, b] = sum_c sum_k coef A[.,a] C[.,g] D[.,o]."""

    @staticmethod
    def forward(ctx, A, C, D, table):
        ctx.save_for_backward(A, C, D)
        ctx.table = table
        ext = get_extension(required=True)
        ent, coefs = table.device_tensors(A.device)
        return ext.etp_reduce(A.contiguous(), C.contiguous(),
                              D.contiguous(), ent, coefs, table.dims[1])

    @staticmethod
    def backward(ctx, gout):
        A, C, D = ctx.saved_tensors
        table = ctx.table
        gout = gout.contiguous()
        need = ctx.needs_input_grad
        # gout sits in the b slot: the three outputs share their inputs
        swept = _first_order((A, gout, C, D),
                             (need[0], False, need[1], need[2]), table)
        if swept is not None:
            return swept[0], swept[2], swept[3], None
        gA = gC = gD = None
        if ctx.needs_input_grad[0]:
            # gA[e,c,a] = sum coef gout[b] C[g] D[o]
            gA = etp_general(C, gout, D, table.perm("gboa"))
        if ctx.needs_input_grad[1]:
            # gC[e,c,g] = sum coef A[a] gout[b] D[o]:
            # roles A=a, B=b, C=o, out=g
            gC = etp_general(A, gout, D, table.perm("abog"))
        if ctx.needs_input_grad[2]:
            # gD[e,c,o] = sum coef A[a] gout[b] C[g]: base role order
            gD = etp_general(A, gout, C, table.perm("abgo"))
        return gA, gC, gD, None


def etp_general(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor,
                table: ETPTable) -> torch.Tensor:
    """out[i,c,o] = sum_k coef_k A[i,c,a] B[i,b] C[i,c,g]."""
    if _kernel_ok(table, A, B, C):
        return _ETPGeneral.apply(A, B, C, table)
    return _dense_general(A, B, C, table)


_FOLD_TABLES: Dict[Tuple[int, int], ETPTable] = {}


def fold_last(t: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """out[n,c,P] = sum_i t[n,c,P,i] x[n,c,i] — the symmetric
    contraction fold step, via the fused ETP kernel when dims fit."""
    n, c = t.shape[0], t.shape[1]
    D = t.shape[-1]
    P = t.numel() // (n * c * D)
    key = (P, D)
    if key not in _FOLD_TABLES:
        ents = [(p * D + i, 0, i, p) for p in range(P) for i in range(D)]
        _FOLD_TABLES[key] = ETPTable(
            torch.tensor(ents, dtype=torch.long),
            torch.ones(len(ents)), (P * D, 1, D, P))
    table = _FOLD_TABLES[key]
    A = t.reshape(n, c, P * D)
    if _kernel_ok(table, A, x, x):
        ones = torch.ones(n, 1, dtype=t.dtype, device=t.device)
        out = etp_general(A, ones, x, table)
    else:
        out = torch.einsum("ncpi,nci->ncp", t.reshape(n, c, P, D), x)
    return out.reshape(t.shape[:-1])


def etp_reduce(A: torch.Tensor, C: torch.Tensor, D: torch.Tensor,
               table: ETPTable) -> torch.Tensor:
    """out[e,b] = sum_c sum_k coef_k A[e,c,a] C[e,c,g] D[e,c,o]."""
    if _reduce_ok(table, A):
        return _ETPReduce.apply(A, C, D, table)
    W = table.dense(A.device, torch.float32).to(A.dtype)
    return torch.einsum("eca,ecg,eco,abgo->eb", A, C, D, W)


# ---------------------------------------------------------------------------
# Indexed / CSR-fused family: gather + TP + segment-sum in one kernel.
#
# Primitive (positions e walk a chosen edge ordering):
#   OUT[r, c, o] = sum_{e in rowptr[r]..rowptr[r+1]} sum_k coef_k
#                  A[ai[e], c, a] B[bi[e], b] C[ci[e], c, g]
# Gradients are instances of the SAME primitive with re-sorted positions
# (see ETPMeta.grad_meta_a), so force training stays fused end to end.
# ---------------------------------------------------------------------------
class ETPMeta:
    """Edge-ordering metadata: per-slot row indices + optional output
    CSR.  bi/ci must be bijections (or None = identity); ai may be a
    many-to-one node map."""

    def __init__(self, n_positions, ai=None, bi=None, ci=None,
                 rowptr=None, n_a_rows=None):
        self.n_positions = int(n_positions)
        self.ai = ai
        self.bi = bi
        self.ci = ci
        self.rowptr = rowptr
        self.n_a_rows = n_a_rows  # rows of A (for the gA output)
        self._r_of_pos = None
        self._grad_meta_a = None

    def r_of_pos(self):
        """Output row of each position (identity without CSR)."""
        if self.rowptr is None:
            return None
        if self._r_of_pos is None:
            counts = self.rowptr[1:] - self.rowptr[:-1]
            self._r_of_pos = torch.repeat_interleave(
                torch.arange(counts.numel(),
                             device=self.rowptr.device), counts)
        return self._r_of_pos

    def grad_meta_a(self):
        """Meta for the A-slot gradient: positions re-sorted by ai so
        the output CSR accumulates over A's rows."""
        if self._grad_meta_a is None:
            assert self.ai is not None and self.n_a_rows is not None, \
                "A-slot gradient needs ai + n_a_rows"
            rho = torch.argsort(self.ai, stable=True)
            rowptr_a = _rowptr_from_sorted(self.ai[rho], self.n_a_rows)
            r = self.r_of_pos()
            ai_new = r[rho] if r is not None else rho
            bi_new = self.bi[rho] if self.bi is not None else rho
            ci_new = self.ci[rho] if self.ci is not None else rho
            # the gradient instance's A is the original OUT tensor:
            # its row count (for second-order CSR) is R (CSR mode) or
            # the position count (per-edge mode)
            n_rows_gA = (self.rowptr.numel() - 1
                         if self.rowptr is not None
                         else self.n_positions)
            m = ETPMeta(self.n_positions, ai=ai_new, bi=bi_new,
                        ci=ci_new, rowptr=rowptr_a,
                        n_a_rows=n_rows_gA)
            self._grad_meta_a = (rho, m)
        return self._grad_meta_a


def _pos_index(t, idx, E):
    if idx is None:
        return t[:E]
    return t.index_select(0, idx)


def _etp_indexed_dense(A, B, C, table, meta):
    """Differentiable fallback (CPU / fp64): gather positions, dense
    einsum, CSR accumulate."""
    E = meta.n_positions
    Apos = _pos_index(A, meta.ai, E)
    Bpos = _pos_index(B, meta.bi, E)
    Cpos = _pos_index(C, meta.ci, E)
    out_pos = _dense_general(Apos, Bpos, Cpos, table)
    if meta.rowptr is None:
        return out_pos
    r = meta.r_of_pos()
    R = meta.rowptr.numel() - 1
    out = out_pos.new_zeros(R, out_pos.shape[1], out_pos.shape[2])
    out.index_add_(0, r, out_pos)
    return out


class _ETPIndexed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, C, table, meta):
        ctx.save_for_backward(A, B, C)
        ctx.table = table
        ctx.meta = meta
        ext = get_extension(required=True)
        ent, coefs = table.device_tensors(A.device)
        if meta.rowptr is not None:
            return ext.etp_nodesum(A.contiguous(), B.contiguous(),
                                   C.contiguous(), ent, coefs,
                                   table.dims[3], meta.rowptr,
                                   meta.ai, meta.bi, meta.ci)
        return ext.etp_general(A.contiguous(), B.contiguous(),
                               C.contiguous(), ent, coefs,
                               table.dims[3], meta.ai, meta.bi,
                               meta.ci, meta.n_positions)

    @staticmethod
    def backward(ctx, gout):
        A, B, C = ctx.saved_tensors
        table = ctx.table
        meta = ctx.meta
        gout = gout.contiguous()
        E = meta.n_positions
        gA = gB = gC = None
        if ctx.needs_input_grad[0]:
            _, meta_a = meta.grad_meta_a()
            gA = etp_indexed(gout, B, C, table.perm("obga"), meta_a)
        if ctx.needs_input_grad[1]:
            # per-position reduce then un-permute via bi (bijection)
            gB_pos = _etp_reduce_idx(A, C, gout, table, meta)
            if meta.bi is not None:
                # index_add_: derived metas can carry many-to-one maps
                gB = gB_pos.new_zeros(B.shape[0], gB_pos.shape[1])
                gB = gB.index_add(0, meta.bi, gB_pos)
            else:
                gB = gB_pos
        if ctx.needs_input_grad[2]:
            r = meta.r_of_pos()
            meta_c = ETPMeta(E, ai=meta.ai, bi=meta.bi,
                             ci=r if r is not None else None,
                             rowptr=None, n_a_rows=A.shape[0])
            gC_pos = etp_indexed(A, B, gout, table.perm("abog"), meta_c)
            if meta.ci is not None:
                gC = gC_pos.new_zeros(C.shape)
                gC = gC.index_add(0, meta.ci, gC_pos)
            else:
                gC = gC_pos
        return gA, gB, gC, None, None


class _ETPReduceIdx(torch.autograd.Function):
    """Per-position channel-reduced contraction with row indices:
    out[e, b] = sum_c sum_k coef A[ai,c,a] C[ci,c,g] D[di,c,o]."""

    @staticmethod
    def forward(ctx, A, C, D, table, ai, ci, di, E):
        ctx.save_for_backward(A, C, D)
        ctx.table = table
        ctx.idx = (ai, ci, di)
        ctx.E = E
        ext = get_extension(required=True)
        ent, coefs = table.device_tensors(A.device)
        return ext.etp_reduce(A.contiguous(), C.contiguous(),
                              D.contiguous(), ent, coefs,
                              table.dims[1], ai, ci, di, E)

    @staticmethod
    def backward(ctx, gout):
        A, C, D = ctx.saved_tensors
        ai, ci, di = ctx.idx
        E = ctx.E
        table = ctx.table
        gout = gout.contiguous()

        def scatter_rows(per_pos, idx, rows):
            if idx is None:
                return per_pos
            out = per_pos.new_zeros((rows,) + per_pos.shape[1:])
            # idx may be many-to-one (node map): accumulate
            return out.index_add_(
                0, idx, per_pos) if idx.numel() == per_pos.shape[0] \
                else out
        gA = gC = gD = None
        if ctx.needs_input_grad[0]:
            # gA[ai,c,a] += coef gout[b] C[g] D[o]
            m = ETPMeta(E, ai=ci, bi=None, ci=di, rowptr=None,
                        n_a_rows=C.shape[0])
            per = etp_indexed(C, gout, D, table.perm("gboa"), m)
            gA = scatter_rows(per, ai, A.shape[0]) if ai is not None \
                else per
        if ctx.needs_input_grad[1]:
            m = ETPMeta(E, ai=ai, bi=None, ci=di, rowptr=None,
                        n_a_rows=A.shape[0])
            per = etp_indexed(A, gout, D, table.perm("abog"), m)
            gC = scatter_rows(per, ci, C.shape[0]) if ci is not None \
                else per
        if ctx.needs_input_grad[2]:
            m = ETPMeta(E, ai=ai, bi=None, ci=ci, rowptr=None,
                        n_a_rows=A.shape[0])
            per = etp_indexed(A, gout, C, table.perm("abgo"), m)
            gD = scatter_rows(per, di, D.shape[0]) if di is not None \
                else per
        return gA, gC, gD, None, None, None, None, None


def _etp_reduce_idx(A, C, D, table, meta):
    r = meta.r_of_pos()
    di = r if r is not None else None
    if _reduce_ok(table, A):
        return _ETPReduceIdx.apply(A, C, D, table, meta.ai, meta.ci,
                                   di, meta.n_positions)
    E = meta.n_positions
    Apos = _pos_index(A, meta.ai, E)
    Cpos = _pos_index(C, meta.ci, E)
    Dpos = D if di is None else D.index_select(0, di)
    W = table.dense(A.device, torch.float32).to(A.dtype)
    return torch.einsum("eca,ecg,eco,abgo->eb", Apos, Cpos, Dpos, W)


def etp_indexed(A, B, C, table, meta: ETPMeta) -> torch.Tensor:
    """Indexed / CSR-fused contraction (see ETPMeta)."""
    if _kernel_ok(table, A, B, C):
        return _ETPIndexed.apply(A, B, C, table, meta)
    return _etp_indexed_dense(A, B, C, table, meta)
