"""ETP sweep kernels (csrc/etp.hip, etp_sweep_kernel) on the GPU.

Kernel tests compare against `_dense_sweep` evaluated in fp64 on the
same inputs (already rounded to the test dtype) with the derived bound

    |out - ref| <= eps_out * |ref| + K * u_acc * S

eps_out = 2^-8 (bf16), 2^-23 (fp32), 2^-52 (fp64): rounding of the
stored result.  K = entry count, u_acc = 2^-23 (2^-52 for fp64): each
of the <= K terms carries a few fp32 roundings and the running sum up
to K more.  S = the same contraction on absolute values of inputs and
coefficients, i.e. the magnitude the rounding errors scale with.

End-to-end tests run first- and second-order gradients through
etp_general / etp_reduce / fold_last with the sweep on and off, at the
tolerances of tests/test_gpu_etp.py."""

import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

from hydragnn_amd.models.mace.blocks import EdgeTensorProduct  # noqa: E402
from hydragnn_amd.ops import etp as etp_mod  # noqa: E402
from hydragnn_amd.ops.etp import (  # noqa: E402
    ETPTable, _dense_general, _dense_sweep, _sweep_fits, etp_general,
    etp_reduce, etp_sweep, fold_last,
)

DEV = "cuda"


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


def _fold_table(P=12, D=4):
    ents = [(p * D + i, 0, i, p) for p in range(P) for i in range(D)]
    return ETPTable(torch.tensor(ents, dtype=torch.long),
                    torch.ones(len(ents)), (P * D, 1, D, P))


TABLES = {
    "random": _random_table(),
    "tp021": EdgeTensorProduct(0, 2, 1).etp_table,
    "tp121": EdgeTensorProduct(1, 2, 1).etp_table,
    "fold": _fold_table(),
}
# nch == 64: direct-store b path (37 rows: ragged last block);
# nch 8 / 96: atomic b path with waves straddling rows
SHAPES = [(37, 64), (37, 8), (5, 96), (1, 64), (1, 8)]
DTYPES = {"fp32": (torch.float32, 2.0 ** -23, 2.0 ** -23),
          "bf16": (torch.bfloat16, 2.0 ** -8, 2.0 ** -23),
          "fp64": (torch.float64, 2.0 ** -52, 2.0 ** -52)}
SUBSETS = list(itertools.product([False, True], repeat=4))
MASKS = [m for m in SUBSETS if any(m)]
FULL = (True, True, True, True)


def _slots(table, rows, nch, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    da, db, dg, do = table.dims
    shapes = [(rows, nch, da), (rows, db), (rows, nch, dg),
              (rows, nch, do)]
    return [torch.randn(s, generator=g).to(dtype).to(DEV)
            for s in shapes]


def _abs_table(table):
    return ETPTable(table.entries, table.coefs.abs(), table.dims)


def _check(outs, ref, mag, mask, eps_out, u_acc, K, what):
    for s in range(4):
        if ref[s] is None or not mask[s]:
            assert outs[s] is None, (what, s)
            continue
        out = outs[s].double()
        bound = eps_out * ref[s].abs() + K * u_acc * mag[s]
        excess = ((out - ref[s]).abs() - bound).max().item()
        assert excess <= 0, (what, s, excess)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("tname", list(TABLES))
def test_sweep_kernels_match_dense(tname, dname):
    table = TABLES[tname]
    atab = _abs_table(table)
    dtype, eps_out, u_acc = DTYPES[dname]
    K = table.entries.shape[0]
    ran = skipped = 0
    for rows, nch in SHAPES:
        p = _slots(table, rows, nch, dtype, 11)
        t = _slots(table, rows, nch, dtype, 12)
        p64 = [x.double() for x in p]
        t64 = [x.double() for x in t]
        pabs = [x.abs() for x in p64]
        tabs = [x.abs() for x in t64]
        for present in [None] + SUBSETS:
            if present is None:
                tang = tang64 = tangabs = None
            else:
                tang = [t[s] if present[s] else None for s in range(4)]
                tang64 = [t64[s] if present[s] else None
                          for s in range(4)]
                tangabs = [tabs[s] if present[s] else None
                           for s in range(4)]
            # reference and magnitude once, on the full mask
            ref = _dense_sweep(p64, tang64, FULL, table)
            mag = _dense_sweep(pabs, tangabs, FULL, atab)
            for mask in MASKS:
                if not _sweep_fits(table, p, tang, mask):
                    skipped += 1  # over the LDS budget: not a kernel run
                    continue
                outs = etp_sweep(p, tang, mask, table)
                ran += 1
                _check(outs, ref, mag, mask, eps_out, u_acc, K,
                       (rows, nch, present, mask))
                for s in range(4):
                    if outs[s] is not None:
                        assert outs[s].dtype == dtype
                        assert outs[s].shape == p[s].shape
    # only the fp64 fold table may exceed the budget, and never at
    # first order
    assert ran > 0
    if not (tname == "fold" and dname == "fp64"):
        assert skipped == 0


@pytest.mark.parametrize("dname", list(DTYPES))
def test_sweep_empty_rows(dname):
    table = TABLES["tp121"]
    dtype = DTYPES[dname][0]
    p = _slots(table, 0, 64, dtype, 1)
    outs = etp_sweep(p, None, FULL, table)
    for s in range(4):
        assert outs[s].shape == p[s].shape and outs[s].dtype == dtype
    outs = etp_sweep(p, [p[0], None, None, None], FULL, table)
    assert outs[0] is None
    for s in (1, 2, 3):
        assert outs[s].shape == p[s].shape


# ---- end to end through the public ops --------------------------------

def _grads_general(dense, table, E=64, C=8):
    torch.manual_seed(2)
    da, db, dg, _ = table.dims
    A = torch.randn(E, C, da, device=DEV, requires_grad=True)
    B = torch.randn(E, db, device=DEV, requires_grad=True)
    Cw = torch.randn(E, C, dg, device=DEV, requires_grad=True)
    out = (_dense_general if dense else etp_general)(A, B, Cw, table)
    g1 = torch.autograd.grad((out ** 2).sum(), (A, B, Cw),
                             create_graph=True)
    g2 = torch.autograd.grad(sum((g ** 2).sum() for g in g1),
                             (A, B, Cw))
    return tuple(g1) + tuple(g2)


def _grads_reduce(dense, table, E=48, C=64):
    torch.manual_seed(3)
    da, _, dg, do = table.dims
    A = torch.randn(E, C, da, device=DEV, requires_grad=True)
    G = torch.randn(E, C, dg, device=DEV, requires_grad=True)
    D = torch.randn(E, C, do, device=DEV, requires_grad=True)
    if dense:
        W = table.dense(A.device, torch.float32)
        out = torch.einsum("eca,ecg,eco,abgo->eb", A, G, D, W)
    else:
        out = etp_reduce(A, G, D, table)
    g1 = torch.autograd.grad((out ** 2).sum() / C, (A, G, D),
                             create_graph=True)
    g2 = torch.autograd.grad(sum((g ** 2).sum() for g in g1),
                             (A, G, D))
    return tuple(g1) + tuple(g2)


def _grads_fold(dense, dtype=torch.float32, n=40, c=16, P=3, D=4):
    torch.manual_seed(4)
    t = torch.randn(n, c, P, D, D, device=DEV, dtype=dtype,
                    requires_grad=True)
    x = torch.randn(n, c, D, device=DEV, dtype=dtype,
                    requires_grad=True)
    out = torch.einsum("ncpqi,nci->ncpq", t, x) if dense \
        else fold_last(t, x)
    g1 = torch.autograd.grad((out ** 2).sum(), (t, x),
                             create_graph=True)
    g2 = torch.autograd.grad(sum((g ** 2).sum() for g in g1), (t, x))
    return tuple(g1) + tuple(g2)


@pytest.fixture(scope="module")
def dense_refs():
    tab = TABLES["random"]
    return {"general": _grads_general(True, tab),
            "reduce": _grads_reduce(True, tab),
            "fold": _grads_fold(True)}


@pytest.mark.parametrize("mode", ["0", "1", "2"])
@pytest.mark.parametrize("op", ["general", "reduce", "fold"])
def test_ops_first_and_second_grads(op, mode, dense_refs, monkeypatch):
    monkeypatch.setenv("HYDRAGNN_ETP_SWEEP", mode)
    before = dict(etp_mod.sweep_stats)
    tab = TABLES["random"]
    fused = {"general": lambda: _grads_general(False, tab),
             "reduce": lambda: _grads_reduce(False, tab),
             "fold": lambda: _grads_fold(False)}[op]()
    for i, (f, d) in enumerate(zip(fused, dense_refs[op])):
        assert torch.allclose(f, d, atol=2e-3, rtol=1e-3), (
            f"{op} grad {i} mismatch {(f - d).abs().max().item():.2e}")
    ran = {k: etp_mod.sweep_stats[k] - before[k] for k in before}
    if mode == "0":
        assert ran["sweep1"] == ran["sweep2"] == 0
    elif mode == "1":
        assert ran["sweep1"] > 0 and ran["sweep2"] == 0 \
            and ran["compose2"] > 0
    else:
        assert ran["sweep1"] > 0 and ran["sweep2"] > 0 \
            and ran["compose2"] == 0


def test_over_budget_shape_falls_back(monkeypatch):
    """fp64 fold table with P*D = 48: the second-order sweep (and a
    256-thread first-order one) exceeds the 150 KiB LDS budget, so the
    single-output composition runs — and matches the einsum."""
    monkeypatch.setenv("HYDRAGNN_ETP_SWEEP", "2")
    table = _fold_table(12, 4)
    acc, rows_in, n_ent = 8, 48 + 1 + 4 + 12, 48
    assert 256 * ((rows_in + 48 + 4) | 1) * acc + n_ent * 20 > 150 * 1024
    p = _slots(table, 4, 16, torch.float64, 5)
    assert not _sweep_fits(table, p, [p[0], None, p[2], None],
                           (True, False, True, True))
    before = dict(etp_mod.sweep_stats)
    fused = _grads_fold(False, dtype=torch.float64, P=3)  # P*D*D -> 12x4
    ran = {k: etp_mod.sweep_stats[k] - before[k] for k in before}
    assert ran["compose2"] > 0 and ran["sweep2"] == 0, ran
    dense = _grads_fold(True, dtype=torch.float64, P=3)
    for f, d in zip(fused, dense):
        assert (f - d).abs().max() <= 1e-9 * d.abs().max()


def test_mace_step_graph_replay_equals_eager(monkeypatch):
    """Forward + force pass + backward of a 2-molecule MACE batch,
    captured in a graph with the sweep kernels: replay == eager."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_mace_model import _build, _mace_config
    from hydragnn_amd.data import Batch
    from hydragnn_amd.utils.datasets.synthetic import md17_shape_dataset

    monkeypatch.setenv("HYDRAGNN_ETP_SWEEP", "2")
    torch.manual_seed(0)
    dataset = md17_shape_dataset(num_samples=2)
    model, _, _ = _build(_mace_config(), dataset)
    model = model.float().to(DEV)
    batch = Batch.from_data_list([d.clone() for d in dataset]).to(DEV)
    params = [q for q in model.parameters() if q.requires_grad]

    def step():
        for q in params:
            q.grad = None
        batch.pos.requires_grad_(True)
        pred = model(batch)
        loss, _ = model.energy_force_loss(pred, batch, create_graph=True)
        grads = torch.autograd.grad(loss, params, allow_unused=True)
        return loss, [g for g in grads if g is not None]

    before = dict(etp_mod.sweep_stats)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            loss_e, grads_e = step()
    torch.cuda.current_stream().wait_stream(s)
    assert etp_mod.sweep_stats["sweep2"] > before["sweep2"]
    loss_e = loss_e.clone()
    grads_e = [g.clone() for g in grads_e]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        loss_g, grads_g = step()
    graph.replay()
    torch.cuda.synchronize()
    # same kernels on the same inputs; only the order of fp32 atomic
    # sums (scatter, sub-64-channel b reductions) may differ
    assert torch.allclose(loss_g, loss_e, rtol=1e-4, atol=1e-6)
    assert len(grads_g) == len(grads_e) > 0
    for a, b in zip(grads_g, grads_e):
        scale = b.abs().max().clamp_min(1e-12)
        assert (a - b).abs().max() <= 1e-4 * scale
