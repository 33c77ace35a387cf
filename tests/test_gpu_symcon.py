"""Fused symmetric-contraction kernels (csrc/symcon.hip) on the GPU.

Every kernel is compared with `_dense_symcon`, differentiated by
autograd in fp64 on the same inputs (already rounded to the test
dtype), under the bound of tests/test_gpu_etp_sweep.py:

    |out - ref| <= eps_out * |ref| + K * u_acc * S

eps_out = 2^-8 (bf16), 2^-23 (fp32), 2^-52 (fp64): rounding of the
stored result.  K = entry count, u_acc = 2^-23 (2^-52 for fp64): each
term carries a few roundings of the accumulator type and the running
sum up to K more.  For weight gradients K also counts the rows summed.
S = the same polynomial (or derivative) on absolute values of operands
and coefficients.
"""

import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

from hydragnn_amd.models.mace.symmetric_contraction import (  # noqa: E402
    SymmetricContraction)
from hydragnn_amd.ops import symcon as sc  # noqa: E402

DEV = "cuda"
NEL = 118
DTYPES = {"fp32": (torch.float32, 2.0 ** -23, 2.0 ** -23),
          "bf16": (torch.bfloat16, 2.0 ** -8, 2.0 ** -23),
          "fp64": (torch.float64, 2.0 ** -52, 2.0 ** -52)}
# (1, 64) one row; (37, 64) ragged last block; (37, 8), (5, 96) waves
# straddling rows and a channel tile that is not full; (257, 64) more
# than one chunk per element and per workgroup
SHAPES = [(1, 64), (37, 64), (37, 8), (5, 96), (257, 64)]
PATTERNS = ["equal", "distinct", "mixed"]
CONFIGS = {"bench1": (1, 1, 2), "bench2": (1, 0, 2), "l2nu3": (2, 1, 3)}
MASKS3 = [m for m in itertools.product([False, True], repeat=3) if any(m)]
MASKS2 = [m for m in itertools.product([False, True], repeat=2) if any(m)]


def _abs_table(t):
    return sc.SymconTable(t.o, t.p, t.i, t.j, t.l, t.coef.abs(), t.D,
                          t.Do, t.P)


_TABLES = {}


def _table(name):
    if name not in _TABLES:
        torch.manual_seed(0)
        mod = SymmetricContraction(*CONFIGS[name], 4, NEL)
        _TABLES[name] = mod.symcon_table()
    return _TABLES[name]


def _elems(pattern, N):
    if pattern == "equal":
        e = torch.full((N,), 5)
    elif pattern == "distinct":
        e = torch.arange(N) % NEL
    else:
        e = torch.tensor([0, 117])[torch.arange(N) % 3 % 2]
    return e.to(DEV)


def _inputs(table, N, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(N, C, table.D), (NEL, table.P, C), (N, C, table.Do),
              (N, C, table.D), (NEL, table.P, C)]
    return [torch.randn(s, generator=g).to(dtype).to(DEV) for s in shapes]


def _all_derivs(table, x, W, g, t_x, t_W, elem):
    """out, (gx, gW), (dR/dx, dR/dW, dR/dg) of the dense form."""
    x, W, g = (v.detach().requires_grad_(True) for v in (x, W, g))
    out = sc._dense_symcon(x, W, elem, table)
    gx, gW = torch.autograd.grad(out, (x, W), g, create_graph=True)
    R = 0
    if t_x is not None:
        R = R + (t_x * gx).sum()
    if t_W is not None:
        R = R + (t_W * gW).sum()
    second = torch.autograd.grad(R, (x, W, g), allow_unused=True)
    second = [torch.zeros_like(v) if s is None else s
              for s, v in zip(second, (x, W, g))]
    return out.detach(), (gx.detach(), gW.detach()), second


def _check(got, ref, mag, eps_out, u_acc, K, what):
    bound = eps_out * ref.abs() + K * u_acc * mag
    err = (got.double() - ref).abs()
    excess = (err - bound).max().item() if err.numel() else -1.0
    assert excess <= 0, (what, err.max().item(), excess)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("tname", list(CONFIGS))
def test_kernels_match_dense(tname, dname):
    table = _table(tname)
    atab = _abs_table(table)
    dtype, eps_out, u_acc = DTYPES[dname]
    K = table.K
    before = dict(sc.symcon_stats)
    for (N, C), pattern in itertools.product(SHAPES, PATTERNS):
        what = (tname, dname, N, C, pattern)
        elem = _elems(pattern, N)
        csr = sc.element_sort(elem, NEL)
        x, W, g, t_x, t_W = _inputs(table, N, C, dtype, 7)
        assert sc.kernel_ok(table, x, W)
        d64 = [v.double() for v in (x, W, g, t_x, t_W)]
        dabs = [v.abs() for v in d64]
        out = sc._SymconFn.apply(x, W, elem, *csr, table)
        assert out.dtype == dtype and out.shape == (N, C, table.Do)
        for tangents in [(True, False), (False, True), (True, True)]:
            pick = lambda vs: [  # noqa: E731
                vs[3] if tangents[0] else None,
                vs[4] if tangents[1] else None]
            ref_o, ref_1, ref_2 = _all_derivs(table, *d64[:3], *pick(d64),
                                              elem)
            mag_o, mag_1, mag_2 = _all_derivs(atab, *dabs[:3],
                                              *pick(dabs), elem)
            _check(out, ref_o, mag_o, eps_out, u_acc, K, what + ("out",))
            for mask in MASKS2:
                outs = sc._first(x, W, g, elem, *csr, table, mask)
                for s in range(2):
                    if not mask[s]:
                        assert outs[s] is None
                        continue
                    _check(outs[s], ref_1[s], mag_1[s], eps_out, u_acc,
                           K + (N if s == 1 else 0), what + ("first", s))
            tx, tW = pick([x, W, g, t_x, t_W])
            # every mask on the kernel; the torch form that serves a
            # present t_W is one autograd call whatever the mask
            for mask in (MASKS3 if tW is None else MASKS3[-1:]):
                outs = sc._second(x, W, g, tx, tW, elem, *csr, table,
                                  mask)
                for s in range(3):
                    if not mask[s]:
                        assert outs[s] is None
                        continue
                    got = outs[s] if outs[s] is not None else \
                        torch.zeros_like(ref_2[s])
                    _check(got, ref_2[s], mag_2[s], eps_out, u_acc,
                           K + (N if s == 1 else 0),
                           what + ("second", tangents, mask, s))
    ran = {k: sc.symcon_stats[k] - before[k] for k in before}
    # t_x alone runs on the kernel, a present t_W on the torch form
    assert ran["fwd"] > 0 and ran["first"] > 0 and ran["second"] > 0
    assert ran["ref_first"] == 0 and ran["ref_second"] > 0


@pytest.mark.parametrize("dname", list(DTYPES))
def test_no_nodes(dname):
    table = _table("bench1")
    dtype = DTYPES[dname][0]
    x, W, g, t_x, _ = _inputs(table, 0, 64, dtype, 3)
    elem = torch.zeros(0, dtype=torch.long, device=DEV)
    csr = sc.element_sort(elem, NEL)
    out = sc._SymconFn.apply(x, W, elem, *csr, table)
    assert out.shape == (0, 64, table.Do)
    gx, gW = sc._first(x, W, g, elem, *csr, table, (True, True))
    assert gx.shape == x.shape and (gW == 0).all()
    rx, rW, rg = sc._second(x, W, g, t_x, None, elem, *csr, table,
                            (True, True, True))
    assert rg.shape == g.shape and (rW == 0).all()


def _integer_table():
    # D = 2 (slot 2 is the constant), Do = 2, P = 2; orders 1, 2 and 3
    o = [0, 1, 0, 1, 0]
    p = [0, 1, 1, 0, 0]
    i = [0, 0, 1, 1, 0]
    j = [2, 1, 1, 2, 0]
    l = [2, 2, 2, 2, 1]  # noqa: E741
    return sc.SymconTable(o, p, i, j, l, [1., 2., -1., 1., 1.], 2, 2, 2)


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
def test_weight_gradient_sum_is_exact_and_repeatable(dname):
    """Small-integer operands and coefficients: every product and every
    fp32 partial sum is an integer below 2^24 (at most 1000 rows x 5
    entries x 3 terms x 2^5 < 2^19), so the fixed-order sums are exact
    and the result is the fp64 value rounded once.  Tolerance zero; two
    runs bitwise equal."""
    table = _integer_table()
    dtype = DTYPES[dname][0]
    N, C = 1000, 64
    g_ = torch.Generator().manual_seed(2)
    ri = lambda *s: torch.randint(-2, 3, s, generator=g_).to(  # noqa: E731
        dtype).to(DEV)
    x, W, g, t_x = ri(N, C, 2), ri(NEL, 2, C), ri(N, C, 2), ri(N, C, 2)
    elem = torch.tensor([0, 7, 117])[
        torch.randint(0, 3, (N,), generator=g_)].to(DEV)
    csr = sc.element_sort(elem, NEL)
    geom = sc.get_extension().symcon_grad_geometry(
        N, C, 2, 2, 2, table.K, 1, NEL, False)
    # several workgroups per element, several chunks per workgroup
    assert geom[3] > 1 and N // 4 > geom[2] * geom[3], geom
    _, ref_1, ref_2 = _all_derivs(table, x.double(), W.double(),
                                  g.double(), t_x.double(), None, elem)
    runs = []
    for _ in range(2):
        gW = sc._first(x, W, g, elem, *csr, table, (True, True))[1]
        rW = sc._second(x, W, g, t_x, None, elem, *csr, table,
                        (True, True, True))[1]
        runs.append((gW, rW))
    assert torch.equal(runs[0][0], ref_1[1].to(dtype))
    assert torch.equal(runs[0][1], ref_2[1].to(dtype))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])


def _module_derivs(mod, x, elem, g, t_x):
    ps = [con.weights[str(nu)] for con in mod.contractions
          for nu in range(con.correlation, 0, -1)]
    x = x.detach().requires_grad_(True)
    g = g.detach().requires_grad_(True)
    out = mod(x, elem)
    first = torch.autograd.grad(out, [x] + ps, g, create_graph=True)
    R = (t_x * first[0]).sum()
    second = torch.autograd.grad(R, [x, g] + ps)
    return ([out, first[0], torch.cat(first[1:], 1), second[0],
             torch.cat(second[2:], 1), second[1]])


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
@pytest.mark.parametrize("tname", ["bench1", "bench2"])
def test_module_fused_vs_composition(tname, dname, monkeypatch):
    """SymmetricContraction with the fused op and with HYDRAGNN_SYMCON=0:
    output, first and second gradients, each against the fp64 module.

    The fused side meets the kernel bound above.  The composition rounds
    to the test dtype after every kernel of its chain: per term of a
    correlation-nu block the coupling GEMM, nu folds and nu - 1 adds,
    2 nu roundings, and one more for the stored result.  A first
    gradient walks that chain backwards over the rounded forward values
    (two chains), a second gradient adds a third, and the weight
    gradients sum rows in fp32 atomics before one more rounding.  With
    unit roundoff u = eps_out / 2 that is at most (2 nu + 1) * chains
    roundings of relative size u on every term, so the composition is
    within (2 nu + 1) * chains * u * S of the fp64 value, on top of the
    accumulation term; the two paths differ by at most the sum."""
    dtype, eps_out, u_acc = DTYPES[dname]
    li, lo, nu = CONFIGS[tname]
    torch.manual_seed(3)
    mod = SymmetricContraction(li, lo, nu, 64, NEL).to(DEV)
    with torch.no_grad():
        for q in mod.parameters():
            q.copy_(q.to(dtype))  # representable in the test dtype
    table = mod.symcon_table()
    atab = _abs_table(table)
    N = 37
    elem = _elems("mixed", N)
    x, _, g, t_x, _ = _inputs(table, N, 64, dtype, 9)
    W64 = sc.concat_weights(mod.contractions, torch.float64).detach()
    _, r1, r2 = _all_derivs(table, x.double(), W64, g.double(),
                            t_x.double(), None, elem)
    ro = sc._dense_symcon(x.double(), W64, elem, table)
    _, m1, m2 = _all_derivs(atab, x.double().abs(), W64.abs(),
                            g.double().abs(), t_x.double().abs(), None,
                            elem)
    mo = sc._dense_symcon(x.double().abs(), W64.abs(), elem, atab)
    refs = [ro, r1[0], r1[1], r2[0], r2[1], r2[2]]
    mags = [mo, m1[0], m1[1], m2[0], m2[1], m2[2]]
    chains = [1, 2, 2, 3, 3, 3]
    names = ["out", "gx", "gW", "dR/dx", "dR/dW", "dR/dg"]
    modt = mod.to(dtype)
    before = dict(sc.symcon_stats)
    monkeypatch.setenv("HYDRAGNN_SYMCON", "1")
    fused = _module_derivs(modt, x, elem, g, t_x)
    ran = {k: sc.symcon_stats[k] - before[k] for k in before}
    assert ran["fwd"] == 1 and ran["first"] == 1 and ran["second"] == 1
    monkeypatch.setenv("HYDRAGNN_SYMCON", "0")
    before = dict(sc.symcon_stats)
    comp = _module_derivs(modt, x, elem, g, t_x)
    assert sc.symcon_stats == before
    for k, name in enumerate(names):
        Kk = table.K + (N if "W" in name else 0)
        _check(fused[k], refs[k], mags[k], eps_out, u_acc, Kk,
               (tname, dname, "fused", name))
        extra = (2 * nu + 1) * chains[k] * (eps_out / 2) * mags[k]
        bound = eps_out * refs[k].abs() + Kk * u_acc * mags[k] + extra
        err = (comp[k].double() - refs[k]).abs()
        print(f"{tname} {dname} {name}: fused max err "
              f"{(fused[k].double() - refs[k]).abs().max().item():.3e} "
              f"composition max err {err.max().item():.3e}")
        assert ((err - bound).max().item()) <= 0, (
            tname, dname, "composition", name, err.max().item())


def test_outside_envelope_runs_composition(monkeypatch):
    """fp16 is not a kernel dtype: the module stays on its composition
    and the op on its dense form."""
    torch.manual_seed(0)
    mod = SymmetricContraction(1, 1, 2, 8, NEL).to(DEV).half()
    x = torch.randn(5, 8, 4, device=DEV).half()
    elem = _elems("mixed", 5)
    before = dict(sc.symcon_stats)
    out = mod(x, elem)
    assert out.shape == (5, 8, 4) and sc.symcon_stats == before
    W = sc.concat_weights(mod.contractions, torch.float16)
    out2 = sc.symcon(x, W, elem, mod.symcon_table())
    assert sc.symcon_stats["dense"] == before["dense"] + 1
    assert torch.allclose(out.float(), out2.float(), rtol=2e-2, atol=2e-2)


def test_mace_step_graph_replay_equals_eager(monkeypatch):
    """Forward + force pass + backward of a 2-molecule MACE batch,
    captured in a graph with the fused contraction: replay == eager."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_mace_model import _build, _mace_config
    from hydragnn_amd.data import Batch
    from hydragnn_amd.utils.datasets.synthetic import md17_shape_dataset

    monkeypatch.setenv("HYDRAGNN_SYMCON", "1")
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

    before = dict(sc.symcon_stats)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            loss_e, grads_e = step()
    torch.cuda.current_stream().wait_stream(s)
    assert sc.symcon_stats["second"] > before["second"]
    assert sc.symcon_stats["ref_second"] == before["ref_second"]
    loss_e = loss_e.clone()
    grads_e = [g.clone() for g in grads_e]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        loss_g, grads_g = step()
    graph.replay()
    torch.cuda.synchronize()
    # same kernels on the same inputs; only the order of fp32 atomic
    # sums elsewhere in the model (scatter, sub-64-channel b
    # reductions) may differ
    assert torch.allclose(loss_g, loss_e, rtol=1e-4, atol=1e-6)
    assert len(grads_g) == len(grads_e) > 0
    for a, b in zip(grads_g, grads_e):
        scale = b.abs().max().clamp_min(1e-12)
        assert (a - b).abs().max() <= 1e-4 * scale
