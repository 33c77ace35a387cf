"""The symmetric contraction as one polynomial table (ops/symcon.py),
checked on the CPU in fp64 against the module's composition.

Bound throughout: K * 2^-52 * S, K the table's entry count and S the
same polynomial (or derivative of it) evaluated on the absolute values
of operands and coefficients -- the convention of
tests/test_gpu_etp_sweep.py.  Both sides sum the same K products per
output in different orders, each product a handful of roundings, so
their difference is a small multiple of 2^-52 * S; K is generous.
"""

import pytest
import torch

from hydragnn_amd.models.mace.symmetric_contraction import \
    SymmetricContraction
from hydragnn_amd.ops import symcon as sc

U = 2.0 ** -52
CONFIGS = [(1, 1, 2), (1, 0, 2), (1, 1, 3), (2, 1, 3), (2, 2, 2)]
# (weights per (element, channel), entries) where the sizes are known
SIZES = {(1, 1, 2): (5, 14), (1, 0, 2): (3, 5), (1, 1, 3): (9, 54),
         (2, 1, 3): (17, 514)}
NEL = 118


def abs_table(t):
    return sc.SymconTable(t.o, t.p, t.i, t.j, t.l, t.coef.abs(), t.D,
                          t.Do, t.P)


def make(cfg, C=3, seed=0):
    torch.manual_seed(seed)
    li, lo, nu = cfg
    mod = SymmetricContraction(li, lo, nu, C, NEL).double()
    return mod, mod.symcon_table()


def params_of(mod):
    """Parameters in the order concat_weights lays them side by side."""
    return [con.weights[str(nu)] for con in mod.contractions
            for nu in range(con.correlation, 0, -1)
            if con.weights[str(nu)].shape[1] > 0]


def inputs(table, N, C, elems, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, table.D, generator=g, dtype=torch.float64)
    elem = torch.tensor([elems[k % len(elems)] for k in range(N)],
                        dtype=torch.long)
    return x, elem


def close(a, b, bound, what):
    err = (a - b).abs()
    bad = err > bound
    assert not bad.any(), (
        f"{what}: max err {err.max().item():.3e}, worst excess "
        f"{(err - bound).max().item():.3e}")


@pytest.mark.parametrize("cfg", CONFIGS)
def test_table_expansion_equals_composition(cfg):
    mod, table = make(cfg)
    if cfg in SIZES:
        assert (table.P, table.K) == SIZES[cfg]
    assert table.D == (cfg[0] + 1) ** 2 and table.Do == (cfg[1] + 1) ** 2
    x, elem = inputs(table, 5, 3, [0, 117, 3])
    W = sc.concat_weights(mod.contractions, torch.float64)
    assert W.shape == (NEL, table.P, 3)
    with torch.no_grad():
        ref = mod(x, elem)
        out = sc._dense_symcon(x, W, elem, table)
        S = sc._dense_symcon(x.abs(), W.abs(), elem, abs_table(table))
    assert out.shape == ref.shape
    close(out, ref, table.K * U * S, f"table vs composition {cfg}")


def test_dense_symcon_gradcheck():
    mod, table = make((1, 1, 2))
    x, elem = inputs(table, 5, 3, [0, 117, 3])
    W = sc.concat_weights(mod.contractions, torch.float64).detach()
    x.requires_grad_(True)
    W.requires_grad_(True)
    fn = lambda x_, W_: sc._dense_symcon(x_, W_, elem, table)  # noqa: E731
    assert torch.autograd.gradcheck(fn, (x, W))
    assert torch.autograd.gradgradcheck(fn, (x, W))


def _derivs_composition(mod, x, elem, g, t_x, t_W):
    ps = params_of(mod)
    x = x.detach().requires_grad_(True)
    g = g.detach().requires_grad_(True)
    out = mod(x, elem)
    first = torch.autograd.grad(out, [x] + ps, g, create_graph=True)
    gx, gW = first[0], torch.cat(first[1:], dim=1)
    R = (t_x * gx).sum()
    if t_W is not None:
        R = R + (t_W * gW).sum()
    second = torch.autograd.grad(R, [x, g] + ps)
    return out, gx, gW, second[0], torch.cat(second[2:], dim=1), second[1]


def _derivs_fn(fn, x, W, g, t_x, t_W):
    x = x.detach().requires_grad_(True)
    W = W.detach().requires_grad_(True)
    g = g.detach().requires_grad_(True)
    out = fn(x, W)
    gx, gW = torch.autograd.grad(out, (x, W), g, create_graph=True)
    R = (t_x * gx).sum()
    if t_W is not None:
        R = R + (t_W * gW).sum()
    rx, rW, rg = torch.autograd.grad(R, (x, W, g))
    return out, gx, gW, rx, rW, rg


@pytest.mark.parametrize("cfg", [(1, 1, 2), (1, 0, 2), (1, 1, 3)])
@pytest.mark.parametrize("with_tw", [False, True])
def test_function_pair_matches_composition(cfg, with_tw):
    """First and second derivatives through _SymconFn / _SymconGrad on
    CPU doubles; elements 0 and 117 occur, element 3 and the rest have
    no node."""
    mod, table = make(cfg)
    N, C = 6, 3
    x, elem = inputs(table, N, C, [0, 117])
    W = sc.concat_weights(mod.contractions, torch.float64).detach()
    gen = torch.Generator().manual_seed(5)
    g = torch.randn(N, C, table.Do, generator=gen, dtype=torch.float64)
    t_x = torch.randn(N, C, table.D, generator=gen, dtype=torch.float64)
    t_W = torch.randn(W.shape, generator=gen, dtype=torch.float64) \
        if with_tw else None
    perm, rowptr = sc.element_sort(elem, NEL)
    assert rowptr.tolist()[:2] == [0, 3] and rowptr[-1].item() == N

    def pair(x_, W_):
        return sc._SymconFn.apply(x_, W_, elem, perm, rowptr, table)

    ref = _derivs_composition(mod, x, elem, g, t_x, t_W)
    got = _derivs_fn(pair, x, W, g, t_x, t_W)
    at = abs_table(table)
    S = _derivs_fn(lambda x_, W_: sc._dense_symcon(x_, W_, elem, at),
                   x.abs(), W.abs(), g.abs(), t_x.abs(),
                   None if t_W is None else t_W.abs())
    names = ["out", "gx", "gW", "dR/dx", "dR/dW", "dR/dg"]
    for name, a, b, s in zip(names, got, ref, S):
        rows = N if "W" in name else 0
        close(a, b, (table.K + rows) * U * s, f"{name} {cfg}")
    # rows of elements without a node get exactly zero
    absent = torch.ones(NEL, dtype=torch.bool)
    absent[[0, 117]] = False
    assert (got[2][absent] == 0).all() and (got[4][absent] == 0).all()


def test_function_pair_no_nodes():
    mod, table = make((1, 1, 2))
    x, elem = inputs(table, 0, 3, [0])
    W = sc.concat_weights(mod.contractions, torch.float64).detach()
    perm, rowptr = sc.element_sort(elem, NEL)
    x.requires_grad_(True)
    W.requires_grad_(True)
    out = sc._SymconFn.apply(x, W, elem, perm, rowptr, table)
    assert out.shape == (0, 3, table.Do)
    gx, gW = torch.autograd.grad(out.sum(), (x, W), create_graph=True)
    assert gx.shape == x.shape and (gW == 0).all()


def test_module_parameters_unchanged():
    """The fused path adds no parameter or buffer: checkpoints load."""
    mod, _ = make((1, 1, 2))
    keys = set(mod.state_dict().keys())
    mod.symcon_table()
    assert set(mod.state_dict().keys()) == keys
    assert all(k.startswith("contractions.") for k in keys)
