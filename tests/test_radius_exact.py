"""Exact tests of the CPU radius-graph builders of `ops/geometry.py`
(`_radius_graph_torch` through `radius_graph`, and `radius_graph_pbc`)
against the int64 references of _exact_radius.py, which do not go
through the project's code.

Positions, cells and the cutoff sit on a dyadic lattice on which every
correct evaluation of d2 is exact, so the reference fixes the edge
multiset completely, pairs at d2 == r2 and coincident atoms included,
and every comparison is an equality.  The cap is checked against its
contract (closest k, exact ties free) for every destination.  The
contract pinned here: membership is d2 <= r2, the cap keeps the k
closest, output is dst-major, and periodic positions may be unwrapped.
"""

import numpy as np
import pytest
import torch

import _exact_radius as R
from _exact_radius import DTYPES, F32, F64, dtype_id
from hydragnn_amd.ops.geometry import radius_graph, radius_graph_pbc

DEV = "cpu"
LAYOUTS = ("n257", "straddle", "singles", "empty_ids", "many_small")


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("use_batch", [True, False])
@pytest.mark.parametrize("name", LAYOUTS)
def test_open_lattice(name, use_batch, loop, dtype):
    R.check_open(radius_graph, DEV, dtype, name, use_batch, loop)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("name", LAYOUTS)
def test_open_lattice_translated(name, dtype):
    """The same lattice moved by an exactly representable 1024 along
    every axis: every difference is unchanged, so is the edge set."""
    a = R.check_open(radius_graph, DEV, dtype, name, True, False)
    b = R.check_open(radius_graph, DEV, dtype, name, True, False,
                     translate=1024.0)
    assert torch.equal(a, b)


def test_open_empty():
    ei = radius_graph(torch.zeros(0, 3), 1.0)
    assert ei.shape == (2, 0) and ei.dtype == torch.long


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("batched", [False, True])
def test_open_cap(batched, dtype):
    capped = R.check_cap_open(radius_graph, DEV, dtype, batched)
    assert capped > 500       # the cap binds on most destinations


@pytest.mark.parametrize("batched", [False, True])
def test_open_cap_not_binding(batched):
    """max_num_neighbors >= degree keeps everything."""
    _, _, (_, cdst, _) = R.cap_open_case(batched)
    k = int(np.bincount(cdst).max())
    assert R.check_cap_open(radius_graph, DEV, F32, batched, k=k) == 0


# ---------------------------------------------------------------------------
# periodic
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("pbc", R.PBC_MASKS, ids=str)
@pytest.mark.parametrize("name", ["cubic", "triclinic"])
def test_pbc_lattice(name, pbc, dtype):
    """Every mask with 1 to 3 periodic directions, wrapped and with each
    atom displaced by lattice vectors in [-2, 2]."""
    R.check_pbc(radius_graph_pbc, DEV, dtype, name, pbc)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_pbc_cutoff_beyond_box(dtype):
    """r = 1.25 in a cell of edge 1: two images per direction."""
    R.check_pbc(radius_graph_pbc, DEV, dtype, "small", (1, 1, 1))
    R.check_pbc(radius_graph_pbc, DEV, dtype, "small", (1, 0, 1))


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_pbc_single_atom(dtype):
    """n = 1, r equal to the cell edge: exactly the six face images."""
    ids = R.check_pbc(radius_graph_pbc, DEV, dtype, "single", (1, 1, 1),
                      r_units=8, coincident=False)
    assert len(ids) == 6
    ids = R.check_pbc(radius_graph_pbc, DEV, dtype, "single", (1, 1, 1),
                      r_units=8, loop=True, coincident=False)
    assert len(ids) == 7


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("name", ["cubic", "triclinic", "small"])
def test_pbc_loop(name, dtype):
    """loop=True adds the n zero-shift self edges and nothing else."""
    pbc = (1, 1, 1)
    n = len(R.pbc_case(name, False)[0])
    plain = R.check_pbc(radius_graph_pbc, DEV, dtype, name, pbc)
    looped = R.check_pbc(radius_graph_pbc, DEV, dtype, name, pbc, loop=True)
    i = np.arange(n)
    selfs = R.encode(i, i, n, np.zeros((n, 3)))
    assert not np.isin(selfs, plain).any()
    assert R.same_multiset(looped, np.concatenate([plain, selfs]))


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("unwrapped", [False, True])
@pytest.mark.parametrize("name,k", [("cubic", 3), ("triclinic", 5),
                                    ("small", 20)])
def test_pbc_cap(name, k, unwrapped, dtype):
    P, C, _ = R.pbc_case(name, unwrapped)
    ref = R.ref_pbc_case(name, unwrapped, (1, 1, 1), R.R_UNITS)
    assert R.check_cap_pbc(radius_graph_pbc, DEV, dtype, P, C, R.UNIT,
                           R.R_UNITS, k, ref) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_pbc_cap_many_images(dtype):
    """Two atoms, cell edge 2, r = 4: more than 27 images, and a cap of
    60 between n * 27 = 54 and the true degree."""
    P, C, _ = R.pbc_case("two_atoms", False)
    ref = R.ref_pbc(P, C, (1, 1, 1), 32)
    deg = np.bincount(ref[1])
    assert deg.min() > 60
    assert R.check_cap_pbc(radius_graph_pbc, DEV, dtype, P, C, R.UNIT, 32,
                           60, ref) == 2
    # a cap at the degree keeps everything
    assert R.check_cap_pbc(radius_graph_pbc, DEV, dtype, P, C, R.UNIT, 32,
                           int(deg.max()), ref) == 0


def test_pbc_empty():
    ei, sh = radius_graph_pbc(torch.zeros(0, 3), 1.0, torch.eye(3))
    assert ei.shape == (2, 0) and sh.shape == (0, 3)
