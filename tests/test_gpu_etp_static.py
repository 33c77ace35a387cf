"""Static-table ETP kernels (csrc/etp_static.hip) on the GPU.

Kernel tests compare against `_dense_sweep` / `_dense_general` in fp64
on the same inputs (already rounded to the test dtype) with the derived
bound of tests/test_gpu_etp_sweep.py

    |out - ref| <= eps_out * |ref| + K * u_acc * S

eps_out = 2^-8 (bf16), 2^-23 (fp32), 2^-52 (fp64): rounding of the
stored result.  K = entry count, u_acc = 2^-23 (2^-52 for fp64): each
of the <= K terms carries a few fp32 roundings and the running sum up
to K more.  S = the same contraction on absolute values of inputs and
coefficients, i.e. the magnitude the rounding errors scale with.

Every launch is also checked for the path it took (`path_counts`): the
combinations listed in docs/kernels.md run on the static kernel, every
other one on the run-time-table kernels, and both meet the bound."""

import itertools
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

from hydragnn_amd.models.mace.blocks import EdgeTensorProduct  # noqa: E402
from hydragnn_amd.ops.etp import (  # noqa: E402
    ETPTable, _dense_general, _dense_sweep, etp_general, etp_sweep,
    path_counts,
)

DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _one_ulp_table():
    tp121 = EdgeTensorProduct(1, 2, 1).etp_table
    coefs = tp121.coefs.clone()
    coefs[10] = torch.nextafter(coefs[10], torch.tensor(2.0))
    return ETPTable(tp121.entries, coefs, tp121.dims)


TABLES = {
    "tp021": EdgeTensorProduct(0, 2, 1).etp_table,
    "tp121": EdgeTensorProduct(1, 2, 1).etp_table,
}
# one wave; exactly one 256-thread block; one wave into the next block;
# ragged last block
ROWS = [1, 4, 5, 37]
DTYPES = {"fp32": (torch.float32, 2.0 ** -23, 2.0 ** -23),
          "bf16": (torch.bfloat16, 2.0 ** -8, 2.0 ** -23),
          "fp64": (torch.float64, 2.0 ** -52, 2.0 ** -52)}
SUBSETS = list(itertools.product([False, True], repeat=4))
MASKS = [m for m in SUBSETS if any(m)]
FULL = (True, True, True, True)


def _listed_instances():
    """(table id, order, omask, tmask) rows of the instance table in
    docs/kernels.md that are on by default."""
    with open(os.path.join(REPO, "docs", "kernels.md")) as f:
        text = f.read()
    rows = re.findall(
        r"^\s*\| `ETPStatic_(\d)_(\d)_(\d)` \| (\d) \| (\d+) \| (\d+) \| "
        r"(on|off) \|", text, re.M)
    ids = {"021": 0, "121": 1}
    return {(ids[a + b + c], int(o), int(om), int(tm))
            for a, b, c, o, om, tm, state in rows if state == "on"}


LISTED = _listed_instances()


@pytest.fixture(autouse=True)
def _default_switch(monkeypatch):
    monkeypatch.delenv("HYDRAGNN_ETP_STATIC", raising=False)


def _bits(flags):
    return sum(1 << s for s in range(4) if flags[s])


def _slots(table, rows, nch, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    da, db, dg, do = table.dims
    shapes = [(rows, nch, da), (rows, db), (rows, nch, dg),
              (rows, nch, do)]
    return [torch.randn(s, generator=g).to(dtype).to(DEV)
            for s in shapes]


def _abs_table(table):
    return ETPTable(table.entries, table.coefs.abs(), table.dims)


def _counted(fn):
    before = path_counts()
    out = fn()
    after = path_counts()
    return out, {k: after[k] - before[k] for k in before}


def _check(outs, ref, mag, mask, eps_out, u_acc, K, what):
    for s in range(4):
        if ref[s] is None or not mask[s]:
            assert outs[s] is None, (what, s)
            continue
        out = outs[s].double()
        bound = eps_out * ref[s].abs() + K * u_acc * mag[s]
        excess = ((out - ref[s]).abs() - bound).max().item()
        assert excess <= 0, (what, s, excess)


def _run_sweeps(table, dtype, eps_out, u_acc, rows, nch, expect_static,
                presents=None, masks=MASKS):
    """Orders 1 and 2 over masks x tangent subsets against the fp64
    reference; `expect_static(order, omask, tmask)` says which path
    each launch must take."""
    atab = _abs_table(table)
    K = table.entries.shape[0]
    p = _slots(table, rows, nch, dtype, 11)
    t = _slots(table, rows, nch, dtype, 12)
    p64 = [x.double() for x in p]
    t64 = [x.double() for x in t]
    pabs = [x.abs() for x in p64]
    tabs = [x.abs() for x in t64]
    n_static = n_generic = 0
    for present in ([None] + SUBSETS if presents is None else presents):
        if present is None:
            tang = tang64 = tangabs = None
        else:
            tang = [t[s] if present[s] else None for s in range(4)]
            tang64 = [t64[s] if present[s] else None for s in range(4)]
            tangabs = [tabs[s] if present[s] else None for s in range(4)]
        ref = _dense_sweep(p64, tang64, FULL, table)
        mag = _dense_sweep(pabs, tangabs, FULL, atab)
        for mask in masks:
            outs, ran = _counted(
                lambda: etp_sweep(p, tang, mask, table))
            what = (rows, nch, present, mask)
            _check(outs, ref, mag, mask, eps_out, u_acc, K, what)
            # a slot no present tangent reaches is dropped from the mask
            eff = mask if present is None else tuple(
                mask[s] and any(present[r] for r in range(4) if r != s)
                for s in range(4))
            if not any(eff):
                assert ran == {"static": 0, "generic": 0}, what
                continue
            order = 1 if present is None else 2
            tm = 0 if present is None else _bits(present)
            if expect_static(order, _bits(eff), tm):
                assert ran == {"static": 1, "generic": 0}, (what, ran)
                n_static += 1
            else:
                assert ran == {"static": 0, "generic": 1}, (what, ran)
                n_generic += 1
            for s in range(4):
                if outs[s] is not None:
                    assert outs[s].dtype == dtype
                    assert outs[s].shape == p[s].shape
    return n_static, n_generic


def _run_forward(table, dtype, eps_out, u_acc, rows, nch, static):
    atab = _abs_table(table)
    K = table.entries.shape[0]
    a, b, g, _ = _slots(table, rows, nch, dtype, 13)
    ref = _dense_general(a.double(), b.double(), g.double(), table)
    mag = _dense_general(a.double().abs(), b.double().abs(),
                         g.double().abs(), atab)
    with torch.no_grad():
        out, ran = _counted(lambda: etp_general(a, b, g, table))
    assert ran == ({"static": 1, "generic": 0} if static
                   else {"static": 0, "generic": 1}), (rows, nch, ran)
    assert out.dtype == dtype and out.shape == ref.shape
    bound = eps_out * ref.abs() + K * u_acc * mag
    excess = ((out.double() - ref).abs() - bound).max().item()
    assert excess <= 0, (rows, nch, excess)


def test_listed_instances_cover_the_flagship_step():
    # forward, first-order (a, b, g) and the layer's second-order sweep
    assert LISTED <= {(0, 0, 8, 0), (0, 1, 7, 0), (0, 2, 15, 6),
                      (1, 0, 8, 0), (1, 1, 7, 0), (1, 2, 15, 7)}
    assert LISTED, "docs/kernels.md lists no static instance"


@pytest.mark.parametrize("dname", ["bf16", "fp32"])
@pytest.mark.parametrize("tname", list(TABLES))
def test_static_kernels_match_dense(tname, dname):
    table = TABLES[tname]
    tid = table.static_id
    assert tid == list(TABLES).index(tname)
    dtype, eps_out, u_acc = DTYPES[dname]
    n_static = 0
    for rows in ROWS:
        s, g = _run_sweeps(
            table, dtype, eps_out, u_acc, rows, 64,
            lambda order, om, tm: (tid, order, om, tm) in LISTED)
        n_static += s
        assert g > 0
        _run_forward(table, dtype, eps_out, u_acc, rows, 64,
                     (tid, 0, 8, 0) in LISTED)
    # each listed sweep instance of this table ran once per row count
    assert n_static == len(ROWS) * sum(
        1 for (t, order, _, _) in LISTED if t == tid and order > 0)


# forward, first order (a, b, g), second order (all | a, b, g): what the
# static kernels would take if the case qualified
_FALLBACK_PRESENTS = [None, (True, True, True, False)]
_FALLBACK_MASKS = [(True, True, True, False), FULL]


def _assert_generic(table, dname, rows, nch):
    dtype, eps_out, u_acc = DTYPES[dname]
    s, g = _run_sweeps(table, dtype, eps_out, u_acc, rows, nch,
                       lambda order, om, tm: False,
                       presents=_FALLBACK_PRESENTS,
                       masks=_FALLBACK_MASKS)
    assert s == 0 and g == 4
    _run_forward(table, dtype, eps_out, u_acc, rows, nch, False)


@pytest.mark.parametrize("dname", ["bf16", "fp32"])
@pytest.mark.parametrize("rows,nch", [(37, 8), (5, 96)])
def test_other_channel_counts_fall_back(rows, nch, dname):
    _assert_generic(TABLES["tp121"], dname, rows, nch)


def test_fp64_falls_back():
    _assert_generic(TABLES["tp121"], "fp64", 37, 64)


@pytest.mark.parametrize("dname", ["bf16", "fp32"])
def test_random_table_falls_back(dname):
    table = _random_table()
    assert table.static_id == -1
    _assert_generic(table, dname, 37, 64)


@pytest.mark.parametrize("dname", ["bf16", "fp32"])
def test_one_ulp_table_falls_back(dname):
    """A near match must not use the compiled-in table: reference and
    magnitude below are computed with the perturbed coefficient."""
    table = _one_ulp_table()
    assert table.static_id == -1
    _assert_generic(table, dname, 37, 64)


def test_switch_off_runs_generic(monkeypatch):
    monkeypatch.setenv("HYDRAGNN_ETP_STATIC", "0")
    _assert_generic(TABLES["tp121"], "bf16", 37, 64)


def _double_backward(table, dtype, scale, m1, m2):
    torch.manual_seed(2)
    da, db, dg, _ = table.dims
    E, C = 37, 64
    A = (torch.randn(E, C, da, device=DEV) * scale).to(dtype)
    B = (torch.randn(E, db, device=DEV) * scale).to(dtype)
    Cw = (torch.randn(E, C, dg, device=DEV) * scale).to(dtype)
    for x in (A, B, Cw):
        x.requires_grad_(True)
    out = etp_general(A, B, Cw, table)
    g1 = torch.autograd.grad((out ** 2).sum() * m1, (A, B, Cw),
                             create_graph=True)
    g2 = torch.autograd.grad(sum((g ** 2).sum() for g in g1) * m2,
                             (A, B, Cw))
    return tuple(g1) + tuple(g2)


# fp32: the inputs and losses of tests/test_gpu_etp.py.  bf16: the two
# paths differ in fp32 summation order, which can move a stored bf16
# result by one ulp, and an ulp in a first derivative reaches the second
# through the cotangents; the tolerances of tests/test_gpu_etp.py (atol
# 2e-3, rtol 1e-3 < 2^-8) admit two bf16 ulps only below 0.25, so
# inputs and losses are scaled to keep every derivative below that
# (largest first and second derivative about 0.08, from an fp32 run of
# the same seed).
_SWITCH = {"fp32": (torch.float32, 1.0, 1.0, 1.0),
           "bf16": (torch.bfloat16, 0.5, 0.005, 4.0)}


@pytest.mark.parametrize("dname", list(_SWITCH))
def test_switch_double_backward(dname, monkeypatch):
    table = TABLES["tp121"]
    dtype, scale, m1, m2 = _SWITCH[dname]
    monkeypatch.setenv("HYDRAGNN_ETP_STATIC", "0")
    off, ran_off = _counted(
        lambda: _double_backward(table, dtype, scale, m1, m2))
    monkeypatch.setenv("HYDRAGNN_ETP_STATIC", "1")
    on, ran_on = _counted(
        lambda: _double_backward(table, dtype, scale, m1, m2))
    # forward, first-order sweep (twice: the second backward passes
    # through the forward's output again) and second-order sweep
    kinds = ((1, 0, 8, 0), (1, 1, 7, 0), (1, 2, 15, 7))
    assert ran_off["static"] == 0 and ran_off["generic"] >= 3, ran_off
    assert sum(ran_on.values()) == ran_off["generic"], (ran_on, ran_off)
    if all(k in LISTED for k in kinds):
        assert ran_on["generic"] == 0, ran_on
    if not any(k in LISTED for k in kinds):
        assert ran_on["static"] == 0, ran_on
    for i, (f, d) in enumerate(zip(on, off)):
        diff = (f.float() - d.float()).abs().max().item()
        print(f"switch {dname} grad {i}: max |on - off| = {diff:.3e}, "
              f"max |off| = {d.float().abs().max().item():.3e}")
        assert torch.allclose(f, d, atol=2e-3, rtol=1e-3), (
            f"grad {i} mismatch {diff:.2e}")


def test_graph_replay_equals_eager():
    """First- plus second-order sweep of tp121 captured in a graph:
    dispatch does no host sync, and replay gives the eager bits."""
    table = TABLES["tp121"]
    p = _slots(table, 37, 64, torch.bfloat16, 21)
    t = _slots(table, 37, 64, torch.bfloat16, 22)
    m1 = (True, True, True, False)
    tang = [t[0], t[1], t[2], None]

    def both():
        return [o for o in etp_sweep(p, None, m1, table)
                + etp_sweep(p, tang, FULL, table) if o is not None]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = [o.clone() for o in both()]
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        (captured, ran) = _counted(both)
    n_on = sum(1 for inst in ((1, 1, 7, 0), (1, 2, 15, 7))
               if inst in LISTED)
    assert ran == {"static": n_on, "generic": 2 - n_on}, ran
    graph.replay()
    torch.cuda.synchronize()
    assert len(captured) == len(eager) == 7
    for a, b in zip(captured, eager):
        assert torch.equal(a, b)
