"""Shared pieces of the exact tests of the radius-graph builders
(test_radius_exact.py on the CPU paths, test_gpu_radius_exact.py on
the HIP kernels): case builders and references that do not go through
`hydragnn_amd.ops.geometry`.  The checks take the functions under test
as arguments.

Exact-lattice method.  Coordinates, cell rows and the cutoff are
integers times `unit` (2^-3 for membership, 2^-6 for the cap), and the
builders assert (`assert_exact`), in lattice units, that
    A < 2^22   and   r^2 < 2^24,
A being the largest absolute coordinate with the shift images of the
reference's range and the translation included.  Every stored value,
every `pos + shift` and every difference is then an integer below
2^24: exact in fp32 (and fp64).  A pair whose d2 is below 2^24, which
covers every pair within the cutoff, has exact squares and an exact
three-term sum, with or without fused multiply-add and in any order.
A pair whose d2 is 2^24 or more evaluates to 2^24 or more, because
rounding is monotone, every term is non-negative and 2^24 is
representable: it cannot pass for an edge.  r is exact, so r*r is, and
sqrt(d2) <= r agrees with d2 <= r2.  The int64 reference therefore
fixes the edge multiset completely, pairs with d2 == r2 included, and
the comparison is equality.

Cap contract.  Per destination, with d2_k the k-th smallest exact d2
among its candidates: min(k, degree) edges are kept, every candidate
with d2 < d2_k is kept and nothing with d2 > d2_k.  Any choice among
exact ties passes.

Banded method, for ordinary floats.  The reference d2 is exact
(rational arithmetic on the stored inputs for every pair that fp64
places near the cutoff).  The kernel's d2 differs from it as follows,
u = eps / 2 being the unit roundoff, M the largest absolute
coordinate, shifts included, d ~ r:
    component  fl(x_j - x_i): one rounding, u |dx|.  With a shift, the
               shift rounded to the dtype, the addition and the
               subtraction: 2 u M + u |dx|;
    d2         2 sum |dx| |err(dx)| <= 2 sqrt(3) d (2 u M + u d), then
               one rounding per product and two sums: 3 u d2;
    r2         (dtype)(r * r): u r2.
Total u (6.93 M r + 7.5 r2) = eps (3.5 M r + 3.7 r2) to first order;
the band is |d2 - r2| <= 4 eps (r M + r2), with M = 0 for the paths
that add no shift (their error does not grow with the coordinates).
Pairs outside the band must match exactly; pairs inside may go either
way.
"""

import functools
from fractions import Fraction

import numpy as np
import torch

F32 = torch.float32
F64 = torch.float64
DTYPES = [F32, F64]
EPS = {F32: 2.0 ** -23, F64: 2.0 ** -52}

UNIT = 2.0 ** -3          # membership lattice
R_UNITS = 10              # 10^2 = 10^2+0+0 = 8^2+6^2+0: boundary pairs
CAP_UNIT = 2.0 ** -6      # cap lattice
S_MAX = 32                # |integer shift| bound of `encode`


def dtype_id(dtype):
    return str(dtype).split(".")[-1]


def seed_of(*key):
    """A seed that does not depend on the interpreter's hash salt."""
    s = 0
    for ch in "/".join(str(k) for k in key):
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


def rng(*key):
    return np.random.RandomState(seed_of(*key))


def assert_exact(max_abs, r_units):
    """The bound of the module docstring, in lattice units."""
    assert max_abs < 2 ** 22 and r_units ** 2 < 2 ** 24, (max_abs, r_units)


def as_pos(P, unit, dtype, dev="cpu"):
    """Lattice integers -> positions; exact in `dtype` by assert_exact."""
    t = torch.from_numpy(np.asarray(P, dtype=np.float64) * unit)
    assert torch.equal(t.to(dtype).to(F64), t)
    return t.to(device=dev, dtype=dtype)


# ---------------------------------------------------------------------------
# ids: one int64 per (src, dst, integer shift)
# ---------------------------------------------------------------------------
def encode(src, dst, n, S=None):
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    key = dst * n + src
    if S is not None:
        S = np.asarray(S, dtype=np.int64).reshape(-1, 3)
        assert S.size == 0 or np.abs(S).max() <= S_MAX
        b = 2 * S_MAX + 1
        for a in range(3):
            key = key * b + (S[:, a] + S_MAX)
    return key


def same_multiset(got, want):
    return np.array_equal(np.sort(got), np.sort(want))


def dst_major(edge_index):
    d = edge_index[1]
    return bool((d[1:] >= d[:-1]).all())


# ---------------------------------------------------------------------------
# open boundary: layouts, cases, int64 reference
# ---------------------------------------------------------------------------
# graph sizes per layout; a 0 is a graph id without atoms.  The work
# group and the j-tile of the tiled kernel both hold 256 atoms.
OPEN_LAYOUTS = {
    "n255": [255],
    "n256": [256],
    "n257": [257],
    "n513": [200, 113, 200],          # graphs across 256 and 512
    "one300": [300],                  # more than one j-tile
    "straddle": [250, 12, 250, 9],    # small graphs on the boundaries
    "singles": [1] * 40 + [30] + [1] * 3,
    "empty_ids": [20, 0, 35, 0, 0, 10, 0],   # middle and end
    "many_small": [5] * 64,           # 51 graphs in the first block
    # for the cell list: six cells of edge r per axis, the minimum
    # corner at the origin, so that every coordinate that is a multiple
    # of r (one atom in six per axis) lies exactly on a cell face
    "cells600": [600],
}


@functools.lru_cache(maxsize=None)
def open_case(name):
    """(P [N, 3] int64, batch [N] int64).  Every graph lives in the same
    corner of space, so graphs overlap and only `batch` separates them.
    The first graph of 5 or more atoms carries a coincident pair and
    up to six planted boundary vectors."""
    g = rng("open", name)
    P, batch = [], []
    planted = False
    for gid, n in enumerate(OPEN_LAYOUTS[name]):
        if n == 0:
            continue
        side = int(np.ceil(R_UNITS * (n / 3.0) ** (1.0 / 3.0)))
        p = g.randint(0, side + 1, size=(n, 3)).astype(np.int64)
        if n >= 5 and not planted:
            planted = True
            p[1] = p[0]
            for row, v in zip(range(2, n), ((10, 0, 0), (8, 6, 0),
                                            (0, 6, 8), (0, -10, 0),
                                            (-6, 0, 8), (0, 0, 10))):
                p[row] = p[0] + v
        if name == "cells600":
            p[8] = 0
            p[9:12] = [[10, 20, 30], [50, 50, 50], [30, 0, 60]]
            p[12:, 0] -= p[12:, 0] % 10 == 1    # more atoms on x faces
        P.append(p)
        batch.append(np.full(n, gid, dtype=np.int64))
    P, batch = np.concatenate(P), np.concatenate(batch)
    assert_exact(np.abs(P).max() + 1024 / UNIT, R_UNITS)
    return P, batch


def d2_matrix(P):
    """[N, N] int64 squared distances."""
    d2 = np.zeros((len(P), len(P)), dtype=np.int64)
    for a in range(3):
        d = P[:, a][None, :] - P[:, a][:, None]
        d2 += d * d
    return d2


def ref_open(P, r_units, batch=None, loop=False):
    """(mask [dst, src], d2 [N, N]) in int64 arithmetic."""
    d2 = d2_matrix(P)
    m = d2 <= r_units * r_units
    if not loop:
        np.fill_diagonal(m, False)
    if batch is not None:
        m &= batch[:, None] == batch[None, :]
    return m, d2


def edge_ids(edge_index, n):
    e = edge_index.detach().cpu().numpy()
    assert e.shape[0] == 2 and e.dtype == np.int64
    assert e.size == 0 or (e.min() >= 0 and e.max() < n)
    return encode(e[0], e[1], n)


def check_open(fn, dev, dtype, name, use_batch, loop, translate=0.0):
    """Lattice membership of one layout: the edge set is the int64
    reference's, boundary and coincident pairs included, dst-major."""
    P, batch = open_case(name)
    n = len(P)
    b = batch if use_batch else None
    m, d2 = ref_open(P, R_UNITS, b, loop)
    off = ~np.eye(n, dtype=bool)
    assert (m & (d2 == R_UNITS ** 2)).sum() >= 6, "boundary pairs"
    assert (m & (d2 == 0) & off).sum() >= 2, "coincident pair"
    pos = as_pos(P + int(translate / UNIT), UNIT, dtype, dev)
    ei = fn(pos, R_UNITS * UNIT,
            batch=None if b is None else torch.from_numpy(b).to(dev),
            max_num_neighbors=n, loop=loop)
    dd, ss = np.nonzero(m)
    assert same_multiset(edge_ids(ei, n), encode(ss, dd, n)), \
        f"{name} {dtype} batch={use_batch} loop={loop} +{translate}"
    assert dst_major(ei)
    return ei


# ---------------------------------------------------------------------------
# cap contract
# ---------------------------------------------------------------------------
def cap_contract(cand_id, cand_dst, cand_d2, got_id, k, n):
    """The contract of the module docstring, for every destination."""
    assert len(np.unique(got_id)) == len(got_id), "duplicate edges"
    assert np.isin(got_id, cand_id).all(), "edge beyond the cutoff"
    kept = np.isin(cand_id, got_id)
    order = np.lexsort((cand_d2, cand_dst))
    dst, d2, kept = cand_dst[order], cand_d2[order], kept[order]
    deg = np.bincount(dst, minlength=n)
    start = np.cumsum(deg) - deg
    d2k = np.full(n, np.iinfo(np.int64).max)
    full = deg > k
    d2k[full] = d2[start[full] + k - 1]
    got_deg = np.bincount(dst[kept], minlength=n)
    assert np.array_equal(got_deg, np.minimum(deg, k)), "kept counts"
    closer = d2 < d2k[dst]
    assert kept[closer].all(), \
        f"{(~kept[closer]).sum()} closer candidates dropped"
    assert not kept[d2 > d2k[dst]].any(), \
        f"{kept[d2 > d2k[dst]].sum()} kept beyond the k-th distance"
    return int(full.sum())


CAP_N, CAP_BOX, CAP_R, CAP_K = 2048, 256, 128, 8      # CAP_UNIT units


@functools.lru_cache(maxsize=None)
def cap_open_case(batched):
    """2048 points on the 2^-6 lattice of a box of edge 4, r = 2, as
    one graph or as 64 graphs of 32; returns P, batch and the reference
    candidates (id, dst, d2)."""
    P = rng("cap_open").randint(0, CAP_BOX + 1,
                                size=(CAP_N, 3)).astype(np.int64)
    assert_exact(CAP_BOX, CAP_R)
    batch = np.repeat(np.arange(64), 32) if batched else None
    m, d2 = ref_open(P, CAP_R, batch, False)
    dd, ss = np.nonzero(m)
    return P, batch, (encode(ss, dd, CAP_N), dd, d2[dd, ss])


def check_cap_open(fn, dev, dtype, batched, k=CAP_K):
    P, batch, (cid, cdst, cd2) = cap_open_case(batched)
    ei = fn(as_pos(P, CAP_UNIT, dtype, dev), CAP_R * CAP_UNIT,
            batch=None if batch is None
            else torch.from_numpy(batch).to(dev),
            max_num_neighbors=k)
    capped = cap_contract(cid, cdst, cd2, edge_ids(ei, CAP_N), k, CAP_N)
    assert dst_major(ei)
    return capped


# ---------------------------------------------------------------------------
# periodic: cells, cases, int64 brute force over integer shifts
# ---------------------------------------------------------------------------
CELLS = {                                    # rows, in lattice units
    "cubic": np.diag([24, 24, 24]),
    "triclinic": np.array([[24, 0, 0], [4, 20, 0], [0, -4, 28]]),
    "small": np.diag([8, 8, 8]),             # r / h = 1.25: n_img >= 2
    "single": np.diag([8, 8, 8]),            # n = 1: self images only
    "two_atoms": np.diag([16, 16, 16]),      # cap case, r = 32 units
}
PBC_MASKS = [m for m in np.ndindex(2, 2, 2) if any(m)]


def _adjugate(C):
    """Integer adj(C) with C @ adj(C) = det(C) I."""
    adj = np.zeros((3, 3), dtype=np.int64)
    for i in range(3):
        for j in range(3):
            minor = np.delete(np.delete(C, i, 0), j, 1)
            adj[j, i] = (-1) ** (i + j) * (
                minor[0, 0] * minor[1, 1] - minor[0, 1] * minor[1, 0])
    return adj


def wrap_exact(P, C):
    """Each point moved by lattice vectors into the unit cell, in
    integers: floor(P adj(C) / det) per lattice direction."""
    det = int(round(np.linalg.det(C)))
    num = P @ _adjugate(C)
    assert np.array_equal(num @ C, det * P)
    w = np.floor_divide(num * np.sign(det), abs(det))
    return P - w @ C


@functools.lru_cache(maxsize=None)
def pbc_case(name, unwrapped, pbc=(1, 1, 1)):
    """(P int64 [n, 3], C int64 [3, 3], D int64 [n, 3]): P = P_wrapped +
    D @ C with D = 0 (wrapped) or integer lattice vectors in [-2, 2]
    along the periodic directions."""
    g = rng("pbc", name)
    C = CELLS[name].astype(np.int64)
    if name == "single":
        P = np.array([[3, 5, 7]], dtype=np.int64)
    elif name == "two_atoms":
        P = np.array([[1, 2, 3], [9, 11, 6]], dtype=np.int64)
    else:
        n, hi = (12, 8) if name == "small" else (24, 29)
        P = g.randint(0, hi, size=(n, 3)).astype(np.int64)
        P[0] = (2, 2, 2)
        P[1] = P[0]                                   # coincident
        for row, v in zip(range(2, 7), ((10, 0, 0), (8, 6, 0), (0, 6, 8),
                                        (14, 0, 0), (0, 0, 18))):
            P[row] = P[0] + v     # the last two: boundary through images
        P = wrap_exact(P, C)
    D = np.zeros_like(P)
    if unwrapped:
        D = rng("pbc_shift", name).randint(-2, 3, size=P.shape)
        D = D.astype(np.int64) * np.array(pbc, dtype=np.int64)
    return P + D @ C, C, D


def _shift_ranges(P, C, pbc, r_units):
    """Per direction ceil(r / h_i) + ceil(spread of the fractional
    coordinates) + 1, h_i = V / |a_j x a_k|: an edge has
    |f_dst - f_src + S|_i h_i <= r, so |S_i| <= r / h_i + spread_i; the
    + 1 covers the float evaluation of h and of the spread."""
    Cf = C.astype(np.float64)
    vol = abs(np.linalg.det(Cf))
    frac = P.astype(np.float64) @ np.linalg.inv(Cf)
    out = []
    for i in range(3):
        if not pbc[i]:
            out.append(0)
            continue
        j, k = (i + 1) % 3, (i + 2) % 3
        h = vol / np.linalg.norm(np.cross(Cf[j], Cf[k]))
        out.append(int(np.ceil(r_units / h)
                       + np.ceil(np.ptp(frac[:, i])) + 1))
    return out


def ref_pbc(P, C, pbc, r_units, loop=False):
    """(src, dst, S [E, 3], d2 [E]) int64: every (src, dst, S) with
    |P[dst] - P[src] + S @ C|^2 <= r^2, S within `_shift_ranges`, and
    without (i, i, 0) unless `loop`.  A shift is skipped only when a
    cartesian component of S @ C alone exceeds r plus the extent of the
    points along that axis, which no pair can make up for."""
    n = len(P)
    R = _shift_ranges(P, C, pbc, r_units)
    ext = np.ptp(P, axis=0)
    amax = np.abs(P).max() + sum(R[i] * np.abs(C[i]).max()
                                 for i in range(3))
    assert_exact(amax, r_units)
    nP = (P * P).sum(1)
    out = [[], [], [], []]
    for S in np.ndindex(*(2 * x + 1 for x in R)):
        S = np.array(S, dtype=np.int64) - np.array(R)
        sc = S @ C
        if (np.abs(sc) > r_units + ext).any():
            continue
        Q = P + sc                                 # dst side
        # d2[src, dst] = |Q[dst]|^2 + |P[src]|^2 - 2 P[src] . Q[dst]
        d2 = (Q * Q).sum(1)[None, :] + nP[:, None] - 2 * (P @ Q.T)
        m = d2 <= r_units * r_units
        if not loop and not S.any():
            np.fill_diagonal(m, False)
        ss, dd = np.nonzero(m)
        out[0].append(ss)
        out[1].append(dd)
        out[2].append(np.broadcast_to(S, (len(ss), 3)))
        out[3].append(d2[ss, dd])
    return tuple(np.concatenate(x) for x in out)


@functools.lru_cache(maxsize=None)
def ref_pbc_case(name, unwrapped, pbc, r_units, loop=False):
    P, C, _ = pbc_case(name, unwrapped, pbc)
    return ref_pbc(P, C, pbc, r_units, loop)


def run_pbc(fn, dev, dtype, P, C, unit, r_units, pbc, loop=False, k=None):
    """Calls the builder under test and returns (src, dst, S) with S the
    integer shifts recovered through the inverse cell; requires
    edge_shifts == S @ cell bit for bit in the position dtype, indices
    in range and dst-major order."""
    n = len(P)
    pos = as_pos(P, unit, dtype, dev)
    cell = as_pos(C, unit, dtype, dev)
    kw = {} if k is None else {"max_num_neighbors": k}
    ei, sh = fn(pos, r_units * unit, cell, pbc=tuple(bool(x) for x in pbc),
                loop=loop, **kw)
    assert sh.dtype == dtype and sh.shape == (ei.shape[1], 3)
    assert dst_major(ei)
    e = ei.cpu().numpy()
    assert e.size == 0 or (e.min() >= 0 and e.max() < n)
    c64 = cell.cpu().to(F64)
    S = torch.round(sh.cpu().to(F64) @ torch.linalg.inv(c64))
    assert torch.equal((S @ c64).to(dtype), sh.cpu()), "shift not S @ cell"
    return e[0], e[1], S.numpy().astype(np.int64)


def check_pbc(fn, dev, dtype, name, pbc, r_units=R_UNITS, loop=False,
              min_boundary=6, coincident=True):
    """Lattice membership of one periodic case, wrapped and unwrapped:
    the multiset of (src, dst, S) is the brute-force reference's, and
    the unwrapped result, its shifts corrected by the displacement, is
    the wrapped one.  Returns the ids of the wrapped result."""
    ids = {}
    for unwrapped in (False, True):
        P, C, D = pbc_case(name, unwrapped, tuple(pbc))
        n = len(P)
        rs, rd, rS, rd2 = ref_pbc_case(name, unwrapped, pbc, r_units, loop)
        assert (rd2 == r_units ** 2).sum() >= min_boundary, "boundary"
        if coincident:
            assert ((rd2 == 0) & (rs != rd)).sum() >= 2, "coincident"
        s, d, S = run_pbc(fn, dev, dtype, P, C, UNIT, r_units, pbc, loop)
        msg = f"{name} pbc={pbc} {dtype} unwrapped={unwrapped} loop={loop}"
        assert same_multiset(encode(s, d, n, S), encode(rs, rd, n, rS)), msg
        # P = P_w + D C: S_w = S + D[dst] - D[src]
        ids[unwrapped] = encode(s, d, n, S + D[d] - D[s])
    assert same_multiset(ids[True], ids[False]), f"{name} pbc={pbc} unwrap"
    return ids[False]


def check_cap_pbc(fn, dev, dtype, P, C, unit, r_units, k, ref=None):
    n = len(P)
    rs, rd, rS, rd2 = ref if ref is not None else \
        ref_pbc(P, C, (1, 1, 1), r_units)
    s, d, S = run_pbc(fn, dev, dtype, P, C, unit, r_units, (1, 1, 1), k=k)
    return cap_contract(encode(rs, rd, n, rS), rd, rd2,
                        encode(s, d, n, S), k, n)


@functools.lru_cache(maxsize=None)
def cap_pbc_case():
    """The points of `cap_open_case` in a periodic cubic cell of edge 4
    (no point lies on the far faces), with the reference candidates."""
    P = rng("cap_pbc").randint(0, CAP_BOX, size=(CAP_N, 3)).astype(np.int64)
    C = np.diag([CAP_BOX] * 3).astype(np.int64)
    return P, C, ref_pbc(P, C, (1, 1, 1), CAP_R)


# ---------------------------------------------------------------------------
# banded method
# ---------------------------------------------------------------------------
def band_width(dtype, r, M):
    """4 eps (r M + r^2), derived in the module docstring."""
    return 4.0 * EPS[dtype] * (r * M + r * r)


def _exact_d2(pi, pj, S, cell):
    """|pj - pi + S @ cell|^2 as a Fraction of the stored values."""
    tot = Fraction(0)
    for a in range(3):
        v = Fraction(float(pj[a])) - Fraction(float(pi[a]))
        if S is not None:
            for b in range(3):
                v += int(S[b]) * Fraction(float(cell[b, a]))
        tot += v * v
    return tot


def banded_ref(pos, r, batch=None, cell=None, pbc=None):
    """Reference on stored float inputs (CPU tensors of the dtype under
    test).  Returns (must, may): ids of the pairs with exact d2 < r2 -
    band, and of those within the band.  fp64 sorts the pairs; every
    pair it puts within 64 bands of the cutoff is redone in rationals,
    fp64's own error being orders below one band (fp32) or below 64
    bands (fp64)."""
    dtype = pos.dtype
    p = pos.to(F64).numpy()
    n = len(p)
    r2 = Fraction(float(r)) ** 2
    if cell is None:
        shifts, c, M = [None], None, 0.0
    else:
        c = cell.to(F64).numpy()
        R = _shift_ranges(p, c, pbc, r)
        shifts = [np.array(S) - np.array(R)
                  for S in np.ndindex(*(2 * x + 1 for x in R))]
        M = np.abs(p).max() + sum(R[i] * np.abs(c[i]).max()
                                  for i in range(3))
    band = band_width(dtype, r, M)
    must, may = [], []
    for S in shifts:
        q = p if S is None else p + S @ c
        diff = q[None, :, :] - p[:, None, :]          # [src, dst, 3]
        d2 = (diff * diff).sum(-1)
        ok = np.ones((n, n), dtype=bool)
        if S is None or not S.any():
            np.fill_diagonal(ok, False)
        if batch is not None:
            ok &= batch[:, None] == batch[None, :]
        near = ok & (np.abs(d2 - float(r2)) <= 64 * band)
        inside = ok & (d2 < float(r2)) & ~near
        ss, dd = np.nonzero(inside)
        must.append(encode(ss, dd, n, None if S is None
                           else np.broadcast_to(S, (len(ss), 3))))
        for i, j in zip(*np.nonzero(near)):
            gap = _exact_d2(p[i], p[j], S, c) - r2
            key = encode([i], [j], n, None if S is None else S[None])
            if abs(gap) <= band:
                may.append(key)
            elif gap < 0:
                must.append(key)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)
    return cat(must), cat(may)


def check_banded(got, must, may, dtype, limit=True):
    """must <= got <= must + may; the band holds at most 1 % of the
    edges in fp32 and none in fp64 unless `limit` is off (adversarial
    inputs sit in the band on purpose)."""
    if limit:
        assert len(may) <= (0.01 * len(must) if dtype == F32 else 0), \
            (len(may), len(must))
    assert len(must) > 100 or not limit
    assert len(np.unique(got)) == len(got)
    assert np.isin(must, got).all(), "an edge outside the band is missing"
    assert np.isin(got, np.concatenate([must, may])).all(), \
        "an edge beyond the band"


def random_points(key, n, box, dtype, translate=0.0):
    g = torch.Generator()
    g.manual_seed(seed_of("banded", key))
    p = torch.rand(n, 3, generator=g, dtype=F64) * box + translate
    return p.to(dtype)


BANDED_CELL = [[6.0, 0.0, 0.0], [0.5, 5.5, 0.0], [0.0, 0.3, 6.2]]


def banded_pbc_case(dtype, n=64):
    g = torch.Generator()
    g.manual_seed(seed_of("banded_pbc"))
    cell = torch.tensor(BANDED_CELL, dtype=F64)
    frac = torch.rand(n, 3, generator=g, dtype=F64) * 0.98 + 0.01
    return (frac @ cell).to(dtype), cell.to(dtype)


def pbc_ids(fn_out, pos, cell):
    """ids of a periodic result on float inputs; S through the inverse
    cell and rounding."""
    ei, sh = fn_out
    S = torch.round(sh.cpu().to(F64) @ torch.linalg.inv(cell.cpu().to(F64)))
    e = ei.cpu().numpy()
    return encode(e[0], e[1], len(pos), S.numpy().astype(np.int64))


def adversarial_points(shape, r, offset, dtype):
    """A line ("line", 200 points) or a 6 x 6 x 6 grid ("grid") whose
    spacing equals the cutoff, every coordinate offset + k r evaluated
    in fp64 and rounded once to `dtype`."""
    if shape == "line":
        x = torch.arange(200, dtype=F64) * r + offset
        p = torch.stack([x, torch.full_like(x, offset),
                         torch.full_like(x, offset)], dim=1)
    else:
        k = torch.arange(6, dtype=F64) * r + offset
        p = torch.cartesian_prod(k, k, k)
    return p.to(dtype)
