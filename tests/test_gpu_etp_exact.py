"""Zero-tolerance tests of the single-output ETP kernels.

Operands are integers in [-3, 3] and coefficients multiples of 0.5 up
to 2, so every partial sum the kernels form is a multiple of 0.5 below
2^23: exact in fp32 whatever the order, atomics included.  The kernels
must therefore equal an fp64 loop over the table's entries, cast once
to the output dtype, bit for bit.  (`table.dense` is no reference here:
it assigns, so duplicate entries vanish.)

Shapes are the smallest that reach every branch: 64 channels (a wave
is one row), 128 (two waves per row), 24 (rows straddle waves, the
b-type output takes per-thread atomics); positions below one block, an
exact multiple of both block sizes (256 and 512), a multiple plus one
wave, and none.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

from hydragnn_amd.ops.etp import (  # noqa: E402
    ETPMeta, ETPTable, _etp_reduce_idx, etp_general, etp_indexed,
    etp_reduce,
)

DIMS = (4, 9, 6, 16)
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
NCH = [64, 128, 24]
# rows per channel count: rows*nch below a block, a multiple of 512,
# a multiple of 256 plus one wave (impossible at 128), and no rows
ROWS = {64: (3, 8, 9, 0), 128: (1, 4, 5, 0), 24: (5, 64, 24, 0)}
# CSR row lengths: empty first, middle and last rows, one row of 32
CSR_COUNTS = (0, 32, 3, 0, 1, 5, 2, 4, 1, 3, 2, 0)
_COEFS = torch.tensor([0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0])


def _random_table(dims=DIMS, n_ent=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    ents = torch.stack(
        [torch.randint(0, d, (n_ent,), generator=g) for d in dims], dim=1)
    coefs = _COEFS[torch.randint(0, 8, (n_ent,), generator=g)]
    return ETPTable(ents, coefs, dims)


def _crafted_table():
    """o = 2 and b = 3 are written by no entry; o = 0, o = 7 and b = 4
    by consecutive entries; entry (2, 2, 3, 1) appears twice."""
    rows = [(0, 0, 0, 0, 1.0), (1, 1, 2, 0, -0.5), (2, 2, 3, 1, 1.5),
            (2, 2, 3, 1, 1.5), (3, 8, 5, 15, 2.0), (0, 4, 1, 7, -2.0),
            (1, 4, 1, 7, 0.5), (3, 6, 4, 3, -1.5)]
    ents = torch.tensor([r[:4] for r in rows])
    coefs = torch.tensor([r[4] for r in rows])
    assert not (ents[:, 3] == 2).any() and not (ents[:, 1] == 3).any()
    return ETPTable(ents, coefs, DIMS)


def _single_table():
    return ETPTable(torch.tensor([[1, 2, 3, 4]]), torch.tensor([1.5]), DIMS)


TABLES = {"random": _random_table, "crafted": _crafted_table,
          "single": _single_table}


def _ints(gen, shape, dtype, lim=3):
    """Integers in [-lim, lim] in `dtype` on the GPU, and in fp64 on
    the CPU for the reference."""
    x = torch.randint(-lim, lim + 1, shape, generator=gen)
    return x.to(dtype).cuda(), x.double()


def _ref_general(A, B, C, tab):
    out = torch.zeros(A.shape[0], A.shape[1], tab.dims[3],
                      dtype=torch.float64)
    for (a, b, g, o), coef in zip(tab.entries.tolist(),
                                  tab.coefs.tolist()):
        out[:, :, o] += coef * A[:, :, a] * B[:, None, b] * C[:, :, g]
    return out


def _ref_reduce(A, C, D, tab):
    out = torch.zeros(A.shape[0], tab.dims[1], dtype=torch.float64)
    for (a, b, g, o), coef in zip(tab.entries.tolist(),
                                  tab.coefs.tolist()):
        out[:, b] += (coef * A[:, :, a] * C[:, :, g] * D[:, :, o]).sum(1)
    return out


def _csr_sum(per_pos, counts):
    out = torch.zeros((len(counts),) + per_pos.shape[1:],
                      dtype=torch.float64)
    lo = 0
    for r, n in enumerate(counts):
        out[r] = per_pos[lo:lo + n].sum(0)
        lo += n
    return out


def _check(out, ref, tab, dtype, terms):
    """`terms`: how many entry walks one output sums (longest CSR row,
    or the channel count for the b-type output)."""
    bound = float(tab.coefs.abs().sum()) * 27 * max(terms, 1)
    assert bound < 2 ** 23, f"partial sums may be inexact: {bound}"
    want = ref.to(dtype)
    assert torch.isfinite(want).all(), "reference overflows the dtype"
    got = out.cpu()
    assert got.dtype == dtype and got.shape == want.shape
    assert torch.equal(got, want), (
        f"{(got.double() - want.double()).abs().max().item()} off, "
        f"{(got != want).sum().item()} of {want.numel()} differ")


def _index_maps(gen, E, N):
    """Many-to-one ai into N rows, permutations bi and ci."""
    ai = torch.randint(0, N, (E,), generator=gen)
    bi = torch.randperm(E, generator=gen)
    ci = torch.randperm(E, generator=gen)
    return ai, bi, ci


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("nch", NCH)
def test_general_exact(dtype, nch):
    gen = torch.Generator().manual_seed(nch)
    da, db, dg, _ = DIMS
    for name, make in TABLES.items():
        tab = make()
        for E in ROWS[nch] if name == "random" else ROWS[nch][2:3]:
            A, Ar = _ints(gen, (E, nch, da), dtype)
            B, Br = _ints(gen, (E, db), dtype)
            C, Cr = _ints(gen, (E, nch, dg), dtype)
            out = etp_general(A, B, C, tab)
            _check(out, _ref_general(Ar, Br, Cr, tab), tab, dtype, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("nch", NCH)
def test_reduce_exact(dtype, nch):
    gen = torch.Generator().manual_seed(100 + nch)
    da, _, dg, do = DIMS
    lim = 2 if dtype == torch.float16 else 3
    for name, make in TABLES.items():
        tab = make()
        for E in ROWS[nch] if name == "random" else ROWS[nch][2:3]:
            A, Ar = _ints(gen, (E, nch, da), dtype, lim)
            C, Cr = _ints(gen, (E, nch, dg), dtype, lim)
            D, Dr = _ints(gen, (E, nch, do), dtype, lim)
            out = etp_reduce(A, C, D, tab)
            _check(out, _ref_reduce(Ar, Cr, Dr, tab), tab, dtype, nch)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("nch", NCH)
def test_indexed_exact(dtype, nch):
    """etp_indexed without a CSR: one output row per position, rows of
    A, B, C picked through ai (many-to-one), bi and ci (permuted)."""
    gen = torch.Generator().manual_seed(200 + nch)
    da, db, dg, _ = DIMS
    N = 10
    for name, make in TABLES.items():
        tab = make()
        for E in ROWS[nch][:3] if name == "random" else ROWS[nch][2:3]:
            ai, bi, ci = _index_maps(gen, E, N)
            A, Ar = _ints(gen, (N, nch, da), dtype)
            B, Br = _ints(gen, (E, db), dtype)
            C, Cr = _ints(gen, (E, nch, dg), dtype)
            meta = ETPMeta(E, ai=ai.cuda(), bi=bi.cuda(), ci=ci.cuda(),
                           n_a_rows=N)
            out = etp_indexed(A, B, C, tab, meta)
            ref = _ref_general(Ar[ai], Br[bi], Cr[ci], tab)
            _check(out, ref, tab, dtype, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("nch", NCH)
def test_csr_exact(dtype, nch):
    """etp_indexed with a rowptr: positions summed per output row."""
    gen = torch.Generator().manual_seed(300 + nch)
    da, db, dg, _ = DIMS
    N = 10
    for counts in (CSR_COUNTS, (0, 0, 0)):
        E = sum(counts)
        rowptr = torch.tensor((0,) + counts).cumsum(0).cuda()
        for name, make in TABLES.items():
            tab = make()
            ai, bi, ci = _index_maps(gen, E, N)
            A, Ar = _ints(gen, (N, nch, da), dtype)
            B, Br = _ints(gen, (E, db), dtype)
            C, Cr = _ints(gen, (E, nch, dg), dtype)
            meta = ETPMeta(E, ai=ai.cuda(), bi=bi.cuda(), ci=ci.cuda(),
                           rowptr=rowptr, n_a_rows=N)
            out = etp_indexed(A, B, C, tab, meta)
            ref = _csr_sum(_ref_general(Ar[ai], Br[bi], Cr[ci], tab),
                           counts)
            _check(out, ref, tab, dtype, max(counts))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("nch", NCH)
def test_reduce_idx_exact(dtype, nch):
    """_etp_reduce_idx: per-position b-type output; A through ai, C
    through ci, D through the CSR's row of each position (or, without
    a CSR, D's own rows)."""
    gen = torch.Generator().manual_seed(400 + nch)
    da, _, dg, do = DIMS
    N = 10
    lim = 2 if dtype == torch.float16 else 3
    counts = CSR_COUNTS
    E = sum(counts)
    rowptr = torch.tensor((0,) + counts).cumsum(0).cuda()
    r_of_pos = torch.repeat_interleave(torch.arange(len(counts)),
                                       torch.tensor(counts))
    for name, make in TABLES.items():
        tab = make()
        ai, _, ci = _index_maps(gen, E, N)
        A, Ar = _ints(gen, (N, nch, da), dtype, lim)
        C, Cr = _ints(gen, (E, nch, dg), dtype, lim)
        D, Dr = _ints(gen, (len(counts), nch, do), dtype, lim)
        meta = ETPMeta(E, ai=ai.cuda(), ci=ci.cuda(), rowptr=rowptr,
                       n_a_rows=N)
        out = _etp_reduce_idx(A, C, D, tab, meta)
        ref = _ref_reduce(Ar[ai], Cr[ci], Dr[r_of_pos], tab)
        _check(out, ref, tab, dtype, nch)
        # no CSR: D is per position
        D, Dr = _ints(gen, (E, nch, do), dtype, lim)
        meta = ETPMeta(E, ai=ai.cuda(), ci=ci.cuda(), n_a_rows=N)
        out = _etp_reduce_idx(A, C, D, tab, meta)
        _check(out, _ref_reduce(Ar[ai], Cr[ci], Dr, tab), tab, dtype, nch)


@pytest.mark.parametrize("nch", NCH)
def test_reduce_over_budget_exact(nch):
    """fp64 slices of (16 + 8 + 12 + 3) | 1 = 39 words at the reduce's
    block of 512 need 512 * 39 * 8 B > 150 KiB, so this shape runs on
    the instance that reads its operands through L1."""
    dims = (16, 3, 8, 12)
    assert 512 * ((sum(dims)) | 1) * 8 > 150 * 1024
    tab = _random_table(dims, seed=5)
    gen = torch.Generator().manual_seed(500 + nch)
    dtype = torch.float64
    for E in ROWS[nch]:
        A, Ar = _ints(gen, (E, nch, dims[0]), dtype)
        C, Cr = _ints(gen, (E, nch, dims[2]), dtype)
        D, Dr = _ints(gen, (E, nch, dims[3]), dtype)
        out = etp_reduce(A, C, D, tab)
        _check(out, _ref_reduce(Ar, Cr, Dr, tab), tab, dtype, nch)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("nch", [64, 128])
def test_deterministic_routes(dtype, nch):
    """On general data every output of etp_general and of the CSR form
    has one writer, and at 64 | nch each etp_reduce output gets one
    atomic add per wave, two at the most, which commute: two runs agree
    bit for bit."""
    gen = torch.Generator().manual_seed(600 + nch)
    da, db, dg, do = DIMS
    tab = _random_table()
    counts = CSR_COUNTS
    E, N = sum(counts), 10

    def normal(*shape):
        return torch.randn(*shape, generator=gen).to(dtype).cuda()

    ai, bi, ci = _index_maps(gen, E, N)
    meta = ETPMeta(E, ai=ai.cuda(), bi=bi.cuda(), ci=ci.cuda(),
                   rowptr=torch.tensor((0,) + counts).cumsum(0).cuda(),
                   n_a_rows=N)
    An, A = normal(N, nch, da), normal(E, nch, da)
    B, C, D = normal(E, db), normal(E, nch, dg), normal(E, nch, do)
    for fn in (lambda: etp_general(A, B, C, tab),
               lambda: etp_indexed(An, B, C, tab, meta),
               lambda: etp_reduce(A, C, D, tab)):
        first, second = fn(), fn()
        assert torch.isfinite(first).all()
        assert torch.equal(first, second)
