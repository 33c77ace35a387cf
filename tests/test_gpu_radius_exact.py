"""Exact tests of the radius kernels of `csrc/radius.hip`
(`radius_tiled_kernel`, open and periodic, and `radius_cells_kernel`)
and of their host side in `ops/geometry.py`, against the int64
references of _exact_radius.py, which do not go through the project's
CPU path.

Lattice method: positions, cells and the cutoff sit on a dyadic
lattice on which every correct evaluation of d2 is exact in fp32, so
the reference fixes the edge multiset, pairs at d2 == r2 and coincident
atoms included, and the comparison is equality.  The cap is checked
against its contract (closest k, exact ties free) for every
destination.  Random floats are checked with the band derived in
_exact_radius.py; inputs built to sit in the band (spacing equal to
the cutoff) must give the same edges on the cell-list and the tiled
kernel.

Layouts: totals of 255, 256, 257 and 513 atoms around the 256-atom work
group and j-tile, graphs across those boundaries, runs of single-atom
graphs, graph ids without atoms, 64 graphs of 5 atoms in one block,
N = 0, both values of `loop`.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

import _exact_radius as R  # noqa: E402
from _exact_radius import DTYPES, F32, F64, dtype_id  # noqa: E402
from hydragnn_amd.ops import geometry  # noqa: E402
from hydragnn_amd.ops.geometry import (  # noqa: E402
    radius_graph, radius_graph_pbc)

DEV = "cuda"
TILED_LAYOUTS = [n for n in R.OPEN_LAYOUTS if n != "cells600"]


@pytest.fixture
def tiled(monkeypatch):
    monkeypatch.setenv("HYDRAGNN_CELL_LIST_MIN", str(10 ** 9))


@pytest.fixture
def cells(monkeypatch):
    """A few hundred atoms take the cell list; `taken` counts the calls
    that did not fall back to the tiled kernel."""
    monkeypatch.setenv("HYDRAGNN_CELL_LIST_MIN", "64")
    taken = []
    inner = geometry._radius_pairs_cell_list

    def spy(*args):
        res = inner(*args)
        taken.append(res is not None)
        return res

    monkeypatch.setattr(geometry, "_radius_pairs_cell_list", spy)
    return taken


# ---------------------------------------------------------------------------
# tiled kernel, open boundary
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("use_batch", [True, False])
@pytest.mark.parametrize("name", TILED_LAYOUTS)
def test_tiled_lattice(tiled, name, use_batch, loop, dtype):
    R.check_open(radius_graph, DEV, dtype, name, use_batch, loop)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_tiled_lattice_translated(tiled, dtype):
    a = R.check_open(radius_graph, DEV, dtype, "n513", True, False)
    b = R.check_open(radius_graph, DEV, dtype, "n513", True, False,
                     translate=1024.0)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_tiled_empty(tiled, dtype):
    pos = torch.zeros(0, 3, dtype=dtype, device=DEV)
    for batch in (None, torch.zeros(0, dtype=torch.long, device=DEV)):
        for loop in (False, True):
            ei = radius_graph(pos, 1.0, batch=batch, loop=loop)
            assert ei.shape == (2, 0) and ei.dtype == torch.long


# ---------------------------------------------------------------------------
# cell-list kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("name", ["cells600", "one300", "n257"])
def test_cells_lattice(cells, name, loop, dtype):
    """Dyadic r, several cells per axis, atoms exactly on cell faces."""
    R.check_open(radius_graph, DEV, dtype, name, False, loop)
    assert cells == [True]


def _ids(pos, r, n):
    return R.edge_ids(radius_graph(pos, r, max_num_neighbors=n), n)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("offset", [1.7, 5.1])
@pytest.mark.parametrize("r", [0.7, 1.1, 2.5])
@pytest.mark.parametrize("shape", ["line", "grid"])
def test_cells_spacing_equals_cutoff(monkeypatch, cells, shape, r, offset,
                                     dtype):
    """Neighbours at a distance that rounds to either side of r, their
    quotient by the cell edge to either side of an integer: the cell
    list finds exactly the tiled kernel's edges, and both keep to the
    banded reference."""
    pos = R.adversarial_points(shape, r, offset, dtype)
    n = len(pos)
    must, may = R.banded_ref(pos, r)
    got_cells = _ids(pos.to(DEV), r, n)
    assert cells == [True]
    monkeypatch.setenv("HYDRAGNN_CELL_LIST_MIN", str(10 ** 9))
    got_tiled = _ids(pos.to(DEV), r, n)
    assert cells == [True]        # not called again
    assert R.same_multiset(got_cells, got_tiled)
    R.check_banded(got_tiled, must, may, dtype, limit=False)
    R.check_banded(got_cells, must, may, dtype, limit=False)


# ---------------------------------------------------------------------------
# periodic kernel
# ---------------------------------------------------------------------------
def _pbc_both(dtype, name, pbc, **kw):
    """GPU against the reference, CPU against the reference, and the two
    multisets against each other."""
    gpu = R.check_pbc(radius_graph_pbc, DEV, dtype, name, pbc, **kw)
    cpu = R.check_pbc(radius_graph_pbc, "cpu", dtype, name, pbc, **kw)
    assert R.same_multiset(gpu, cpu)
    return gpu


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("pbc", R.PBC_MASKS, ids=str)
@pytest.mark.parametrize("name", ["cubic", "triclinic"])
def test_pbc_lattice(name, pbc, dtype):
    _pbc_both(dtype, name, pbc)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_pbc_cutoff_beyond_box(dtype):
    _pbc_both(dtype, "small", (1, 1, 1))
    _pbc_both(dtype, "small", (1, 0, 1))


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_pbc_single_atom(dtype):
    kw = dict(r_units=8, coincident=False)
    assert len(_pbc_both(dtype, "single", (1, 1, 1), **kw)) == 6
    assert len(_pbc_both(dtype, "single", (1, 1, 1), loop=True, **kw)) == 7


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("name", ["cubic", "triclinic", "small"])
def test_pbc_loop(name, dtype):
    pbc = (1, 1, 1)
    n = len(R.pbc_case(name, False)[0])
    plain = _pbc_both(dtype, name, pbc)
    looped = _pbc_both(dtype, name, pbc, loop=True)
    i = np.arange(n)
    selfs = R.encode(i, i, n, np.zeros((n, 3)))
    assert not np.isin(selfs, plain).any()
    assert R.same_multiset(looped, np.concatenate([plain, selfs]))


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("unwrapped", [False, True])
@pytest.mark.parametrize("name,k", [("cubic", 3), ("triclinic", 5),
                                    ("small", 20)])
def test_pbc_cap_small(name, k, unwrapped, dtype):
    P, C, _ = R.pbc_case(name, unwrapped)
    ref = R.ref_pbc_case(name, unwrapped, (1, 1, 1), R.R_UNITS)
    assert R.check_cap_pbc(radius_graph_pbc, DEV, dtype, P, C, R.UNIT,
                           R.R_UNITS, k, ref) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_pbc_cap_many_images(dtype):
    P, C, _ = R.pbc_case("two_atoms", False)
    ref = R.ref_pbc(P, C, (1, 1, 1), 32)
    deg = np.bincount(ref[1])
    assert R.check_cap_pbc(radius_graph_pbc, DEV, dtype, P, C, R.UNIT, 32,
                           60, ref) == 2
    assert R.check_cap_pbc(radius_graph_pbc, DEV, dtype, P, C, R.UNIT, 32,
                           int(deg.max()), ref) == 0


# ---------------------------------------------------------------------------
# closest-k cap at 2048 atoms: fp32 on the 2^-6 lattice, box 4, r = 2,
# k = 8.  Distinct distances differ by far less than the ulp of a float
# key that carries the destination index.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("batched", [False, True])
def test_cap_tiled(tiled, batched):
    assert R.check_cap_open(radius_graph, DEV, F32, batched) > 500


def test_cap_cells(cells):
    assert R.check_cap_open(radius_graph, DEV, F32, False) == R.CAP_N
    assert cells == [True]


def test_cap_pbc():
    P, C, ref = R.cap_pbc_case()
    assert R.check_cap_pbc(radius_graph_pbc, DEV, F32, P, C, R.CAP_UNIT,
                           R.CAP_R, R.CAP_K, ref) == R.CAP_N


@pytest.mark.parametrize("path", ["tiled", "tiled_batched", "cells"])
def test_cap_not_binding(monkeypatch, path):
    """max_num_neighbors >= degree keeps everything."""
    monkeypatch.setenv("HYDRAGNN_CELL_LIST_MIN",
                       "64" if path == "cells" else str(10 ** 9))
    batched = path == "tiled_batched"
    _, _, (_, cdst, _) = R.cap_open_case(batched)
    k = int(np.bincount(cdst).max())
    assert R.check_cap_open(radius_graph, DEV, F32, batched, k=k) == 0


def test_cap_pbc_not_binding():
    P, C, _ = R.pbc_case("cubic", True)
    ref = R.ref_pbc_case("cubic", True, (1, 1, 1), R.R_UNITS)
    k = int(np.bincount(ref[1]).max())
    assert R.check_cap_pbc(radius_graph_pbc, DEV, F32, P, C, R.UNIT,
                           R.R_UNITS, k, ref) == 0


# ---------------------------------------------------------------------------
# random floats, banded
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,translate", [(F32, 0.0), (F64, 0.0),
                                             (F32, 1000.0)],
                         ids=["float32", "float64", "float32+1000"])
def test_tiled_banded(tiled, dtype, translate):
    n, r = 600, 2.0
    pos = R.random_points("tiled", n, 10.0, dtype, translate)
    batch = np.repeat(np.arange(2), n // 2)
    must, may = R.banded_ref(pos, r, batch=batch)
    ei = radius_graph(pos.to(DEV), r, batch=torch.from_numpy(batch).to(DEV),
                      max_num_neighbors=n)
    R.check_banded(R.edge_ids(ei, n), must, may, dtype)
    assert R.dst_major(ei)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_cells_banded(cells, dtype):
    n, r = 600, 2.0
    pos = R.random_points("cells", n, 10.0, dtype)
    must, may = R.banded_ref(pos, r)
    ei = radius_graph(pos.to(DEV), r, max_num_neighbors=n)
    assert cells == [True]
    R.check_banded(R.edge_ids(ei, n), must, may, dtype)
    assert R.dst_major(ei)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_pbc_banded(dtype):
    r, pbc = 2.5, (True, True, True)
    pos, cell = R.banded_pbc_case(dtype)
    must, may = R.banded_ref(pos, r, cell=cell, pbc=pbc)
    out = radius_graph_pbc(pos.to(DEV), r, cell.to(DEV), pbc=pbc)
    R.check_banded(R.pbc_ids(out, pos, cell), must, may, dtype)
    assert R.dst_major(out[0])
