"""Algebra of the ETP sweep family on CPU, in fp64.

`_dense_sweep` is the reference the HIP sweep kernels are tested
against; here it is itself checked against autograd of the dense
forward contraction: first-order mode against `torch.autograd.grad`,
second-order mode against the double backward with random cotangents,
for every output mask and every pattern of absent tangents.  The
autograd wiring (`_ETPSweep1`) runs on its dense path here."""

import itertools

import pytest
import torch

from hydragnn_amd.models.mace.blocks import EdgeTensorProduct
from hydragnn_amd.ops.etp import (
    ETPTable, _dense_general, _dense_sweep, _ETPSweep1, etp_sweep,
)

REL = 1e-10  # the project's fp64 parity level
ROWS, NCH = 5, 3


def _random_table(seed=0, da=4, db=9, dg=6, do=16, n_ent=40):
    # same table as tests/test_gpu_etp.py
    g = torch.Generator().manual_seed(seed)
    ents = torch.stack([
        torch.randint(0, da, (n_ent,), generator=g),
        torch.randint(0, db, (n_ent,), generator=g),
        torch.randint(0, dg, (n_ent,), generator=g),
        torch.randint(0, do, (n_ent,), generator=g),
    ], dim=1)
    coefs = torch.randn(n_ent, generator=g)
    return ETPTable(ents, coefs, (da, db, dg, do))


TABLES = {
    "random": _random_table(),
    "tp021": EdgeTensorProduct(0, 2, 1).etp_table,
    "tp121": EdgeTensorProduct(1, 2, 1).etp_table,
}
MASKS = [m for m in itertools.product([False, True], repeat=4)]


def _slots(table, seed, requires_grad=False):
    g = torch.Generator().manual_seed(seed)
    da, db, dg, do = table.dims
    shapes = [(ROWS, NCH, da), (ROWS, db), (ROWS, NCH, dg),
              (ROWS, NCH, do)]
    return [torch.randn(s, generator=g, dtype=torch.float64)
            .requires_grad_(requires_grad) for s in shapes]


def _rel(x, ref):
    return ((x - ref).abs().max() /
            ref.abs().max().clamp_min(1e-300)).item()


def _form(p, table):
    """Q(a, b, g, o) through the dense forward contraction."""
    return (_dense_general(p[0], p[1], p[2], table) * p[3]).sum()


@pytest.mark.parametrize("name", list(TABLES))
def test_first_order_matches_autograd(name):
    table = TABLES[name]
    p = _slots(table, 1, requires_grad=True)
    ref = torch.autograd.grad(_form(p, table), p)
    for mask in MASKS:
        outs = _dense_sweep(p, None, mask, table)
        for s in range(4):
            if not mask[s]:
                assert outs[s] is None
            else:
                assert _rel(outs[s], ref[s]) <= REL, (mask, s)


@pytest.mark.parametrize("name", list(TABLES))
def test_second_order_matches_double_backward(name):
    table = TABLES[name]
    p = _slots(table, 2, requires_grad=True)
    first = torch.autograd.grad(_form(p, table), p, create_graph=True)
    cot = _slots(table, 3)  # random cotangents, one per slot
    for present in MASKS:
        if not any(present):
            continue
        tangents = [cot[s] if present[s] else None for s in range(4)]
        # d/dp_r of sum_s <t_s, dQ/dp_s>: the double backward
        inner = sum((first[s] * cot[s]).sum()
                    for s in range(4) if present[s])
        ref = torch.autograd.grad(inner, p, retain_graph=True,
                                  allow_unused=True)
        for mask in MASKS:
            outs = _dense_sweep(p, tangents, mask, table)
            for s in range(4):
                reached = any(present[r] for r in range(4) if r != s)
                if not (mask[s] and reached):
                    assert outs[s] is None
                    # Q is linear in slot s: t_s alone gives nothing
                    if mask[s]:
                        assert ref[s] is None or ref[s].abs().max() == 0
                else:
                    assert _rel(outs[s], ref[s]) <= REL, (present, mask, s)


def test_dispatcher_uses_dense_on_cpu():
    table = TABLES["tp121"]
    p = _slots(table, 4)
    t = _slots(table, 5)
    t[1] = None
    mask = (True, True, False, True)
    for tangents in (None, t):
        got = etp_sweep(p, tangents, mask, table)
        ref = _dense_sweep(p, tangents, mask, table)
        for x, r in zip(got, ref):
            assert (x is None) == (r is None)
            if x is not None:
                assert torch.equal(x, r)


@pytest.mark.parametrize("mask", [(True, True, True, False),
                                  (True, False, True, True),
                                  (False, True, False, False)])
def test_sweep_function_autograd(mask):
    """_ETPSweep1 forward = first derivatives, backward = second-order
    sweep: both against plain autograd of the dense contraction."""
    table = TABLES["random"]
    p = _slots(table, 6, requires_grad=True)
    q = [x.detach().clone().requires_grad_(True) for x in p]
    outs = _ETPSweep1.apply(*p, table, mask)
    ref = torch.autograd.grad(_form(q, table), q, create_graph=True)
    cot = _slots(table, 7)
    used = [s for s in range(4) if mask[s] and s != 1]  # drop one
    if not used:
        used = [s for s in range(4) if mask[s]]
    for s in range(4):
        assert (outs[s] is None) == (not mask[s])
        if mask[s]:
            assert _rel(outs[s], ref[s]) <= REL
    loss = sum((outs[s] * cot[s]).sum() for s in used)
    loss_ref = sum((ref[s] * cot[s]).sum() for s in used)
    g = torch.autograd.grad(loss, p, allow_unused=True)
    g_ref = torch.autograd.grad(loss_ref, q, allow_unused=True)
    for s in range(4):
        if g_ref[s] is None or g_ref[s].abs().max() == 0:
            assert g[s] is None or g[s].abs().max() == 0
        else:
            assert _rel(g[s], g_ref[s]) <= REL, s
