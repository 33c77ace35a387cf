"""MACE building blocks.

Functional parity with /root/reference/hydragnn/utils/model/mace_utils/
modules/blocks.py:151-981 and radial.py:33-258: radial embedding
(Bessel/Gaussian/Chebyshev x polynomial cutoff, optional Agnesi/Soft
distance transforms), the residual interaction block (linear_up ->
edge-wise uvu tensor product with radial-MLP weights -> scatter-sum /
avg_num_neighbors -> linear + per-l skip), the equivariant product
basis (symmetric contraction + residual), and linear/nonlinear
multihead readouts.

Feature layout: [N, C, D] dense uniform-multiplicity tower,
D = (lmax+1)^2 (what reshape_irreps produces in the reference).
"""

from __future__ import annotations

import math
from typing import List, Optional

import torch
from torch import nn

from ...ops import (
    bessel_basis,
    chebyshev_basis,
    gather,
    gaussian_basis,
    polynomial_cutoff,
    scatter,
)
from ...ops.mfma_linear import MFMALinear
from .o3 import IrrepsLinear, dim, tp_paths, wigner_3j
from .symmetric_contraction import SymmetricContraction


class RadialEmbeddingBlock(nn.Module):
    """Radial basis x polynomial cutoff (reference blocks.py:151-187):
    the cutoff is evaluated on the RAW edge length; the optional
    Agnesi/Soft distance transform is applied only to the basis input."""

    def __init__(self, r_max: float, num_bessel: int = 8,
                 num_polynomial_cutoff: int = 5,
                 radial_type: str = "bessel",
                 distance_transform: Optional[str] = None):
        super().__init__()
        self.r_max = r_max
        self.num_bessel = num_bessel
        self.p = float(num_polynomial_cutoff)
        self.radial_type = (radial_type or "bessel").lower()
        if distance_transform == "Agnesi":
            self.distance_transform = AgnesiTransform()
        elif distance_transform == "Soft":
            self.distance_transform = SoftTransform()
        else:
            self.distance_transform = None
        if self.radial_type == "bessel":
            self.bessel_weights = nn.Parameter(
                torch.arange(1, num_bessel + 1, dtype=torch.float)
                * math.pi / r_max)
            self.out_dim = num_bessel
        elif self.radial_type == "gaussian":
            offsets = torch.linspace(0.0, r_max, num_bessel)
            self.register_buffer("offsets", offsets)
            self.coeff = -0.5 / float(offsets[1] - offsets[0]) ** 2
            self.out_dim = num_bessel
        elif self.radial_type == "chebyshev":
            self.out_dim = num_bessel
        else:
            raise ValueError(f"unknown radial_type {radial_type}")

    def forward(self, lengths: torch.Tensor,
                z: Optional[torch.Tensor] = None,
                edge_index: Optional[torch.Tensor] = None) -> torch.Tensor:
        cutoff = polynomial_cutoff(lengths, self.r_max, self.p)
        r = lengths
        if self.distance_transform is not None:
            r = self.distance_transform(lengths, z=z,
                                        edge_index=edge_index)
        if self.radial_type == "bessel":
            rb = bessel_basis(r, self.r_max, self.bessel_weights.to(r.dtype))
        elif self.radial_type == "gaussian":
            rb = gaussian_basis(r, self.offsets.view(1, -1).to(r.dtype),
                                self.coeff)
        else:
            rb = chebyshev_basis(r, self.r_max, self.num_bessel)
        return rb * cutoff


class EdgeTensorProduct(nn.Module):
    """Edge-wise uvu tensor product with per-edge per-path weights:
    m_e[c, m3] = sum_paths w_e[c, path] * W3j . (x_src[c, l1] (x) Y_e[l2])
    (reference blocks.py:329-412 conv_tp).  The einsum form maps to
    batched GEMMs; the fused HIP kernel replaces it on GPU."""

    def __init__(self, lmax_node: int, lmax_edge: int, lmax_out: int):
        super().__init__()
        self.paths = tp_paths(lmax_node, lmax_edge, lmax_out)
        self.lmax_out = lmax_out
        self.num_paths = len(self.paths)
        self.d1 = dim(lmax_node)
        self.d2 = dim(lmax_edge)
        self.d3 = dim(lmax_out)
        # One combined coupling matrix: rows = (m1, m2) outer pairs,
        # cols = concatenated per-path m3 blocks.  The per-edge TP then
        # collapses to outer-product + ONE GEMM + masked column
        # reduction — batched-GEMM-shaped for MFMA instead of a kernel
        # per path.
        cols = sum(2 * l3 + 1 for (_, _, l3) in self.paths)
        Wcat = torch.zeros(self.d1 * self.d2, cols)
        path_of_col = torch.zeros(cols, dtype=torch.long)
        m3_of_col = torch.zeros(cols, dtype=torch.long)
        c0 = 0
        for p, (l1, l2, l3) in enumerate(self.paths):
            W = wigner_3j(l1, l2, l3).float()  # [2l1+1, 2l2+1, 2l3+1]
            for a in range(2 * l1 + 1):
                for b in range(2 * l2 + 1):
                    row = (l1 * l1 + a) * self.d2 + (l2 * l2 + b)
                    Wcat[row, c0:c0 + 2 * l3 + 1] = W[a, b]
            path_of_col[c0:c0 + 2 * l3 + 1] = p
            m3_of_col[c0:c0 + 2 * l3 + 1] = torch.arange(
                l3 * l3, (l3 + 1) ** 2)
            c0 += 2 * l3 + 1
        self.register_buffer("Wcat", Wcat)
        self.register_buffer("path_of_col", path_of_col)
        self.register_buffer("m3_of_col", m3_of_col)
        self.num_cols = cols
        # fused-kernel entry table (ops/etp.py): one entry per nonzero
        # Wigner coefficient, (a=m1 slot, b=m2 slot, g=path, o=m3 slot)
        from ...ops.etp import ETPTable
        ents, cfs = [], []
        for p, (l1, l2, l3) in enumerate(self.paths):
            W = wigner_3j(l1, l2, l3).float()
            nz = (W.abs() > 1e-12).nonzero()
            for (m1, m2, m3) in nz.tolist():
                ents.append((l1 * l1 + m1, l2 * l2 + m2, p,
                             l3 * l3 + m3))
                cfs.append(float(W[m1, m2, m3]))
        self.etp_table = ETPTable(
            torch.tensor(ents, dtype=torch.long),
            torch.tensor(cfs), (self.d1, self.d2, self.num_paths,
                                self.d3))

    def forward(self, x_src: torch.Tensor, Y: torch.Tensor,
                weights: torch.Tensor) -> torch.Tensor:
        """x_src [E, C, D_node], Y [E, D_edge],
        weights [E, C, num_paths] -> [E, C, D_out].

        GPU: one fused HIP kernel (ops/etp.py) computes the whole
        contraction at the memory-bound roofline, including both
        autograd passes of force training.  CPU/fp64: fold Y into the
        coupling table first (WY [E, D1, cols], no channel dim) then a
        batched GEMM over edges — avoids materializing the
        E x C x D1 x D2 outer product."""
        from ...ops.etp import _kernel_ok, etp_general
        if _kernel_ok(self.etp_table, x_src, Y, weights):
            return etp_general(x_src, Y, weights, self.etp_table)
        E, C, _ = x_src.shape
        W3 = self.Wcat.to(x_src.dtype).view(self.d1, self.d2,
                                            self.num_cols)
        WY = torch.einsum("eb,abc->eac", Y, W3)        # [E, D1, cols]
        raw = torch.bmm(x_src, WY)                     # [E, C, cols]
        w_exp = weights.index_select(2, self.path_of_col)
        scaled = raw * w_exp
        out = x_src.new_zeros(E, C, self.d3)
        out.index_add_(2, self.m3_of_col, scaled)
        return out


class RealAgnosticResidualInteractionBlock(nn.Module):
    """linear_up -> gather -> edge TP (radial-MLP weights) ->
    scatter-sum / avg_num_neighbors -> linear -> (+ per-l skip)."""

    # extra radial-MLP input features beyond the radial embedding
    # (the Att subclass appends 2C down-projected endpoint scalars)
    _radial_extra = 0

    def __init__(self, num_channels: int, lmax_node: int, lmax_edge: int,
                 lmax_out: int, radial_dim: int,
                 avg_num_neighbors: float,
                 radial_mlp: Optional[List[int]] = None):
        super().__init__()
        self.avg_num_neighbors = avg_num_neighbors
        self.linear_up = IrrepsLinear(num_channels, num_channels, lmax_node)
        self.conv_tp = EdgeTensorProduct(lmax_node, lmax_edge, lmax_out)
        from ...ops.mfma_linear import MFMALinear as SplitKLinear
        self._setup_extra(num_channels)
        hidden = radial_mlp or [64, 64, 64]
        mods = []
        prev = radial_dim + self._radial_extra
        for h in hidden:
            mods += [SplitKLinear(prev, h), nn.SiLU()]
            prev = h
        mods.append(
            SplitKLinear(prev, num_channels * self.conv_tp.num_paths))
        self.radial_mlp = nn.Sequential(*mods)
        self.num_channels = num_channels
        self.linear = IrrepsLinear(num_channels, num_channels, lmax_out)
        self.skip_linear = IrrepsLinear(num_channels, num_channels,
                                        min(lmax_node, lmax_out))
        self.lmax_out = lmax_out
        self.lmax_node = lmax_node

    def _setup_extra(self, num_channels: int):
        pass

    def _radial_tail(self, h: torch.Tensor) -> torch.Tensor:
        """radial_mlp[1:] on the first layer's pre-activation h: each
        SiLU -> Linear pair that qualifies runs as one fused act_linear
        (ops/act_linear.py), the others as the modules themselves."""
        from ...ops import act_linear as al
        tail = self.radial_mlp[1:]
        if not (al.fused_route() and h.dim() == 2 and h.is_cuda
                and h.dtype == torch.bfloat16 and not al.use_eager()
                and len(tail) % 2 == 0):
            return tail(h)
        for act, lin in zip(tail[0::2], tail[1::2]):
            if (type(act) is nn.SiLU and isinstance(lin, nn.Linear)
                    and lin.weight.dtype == torch.bfloat16
                    and al.in_envelope(h.shape[0], lin.out_features,
                                       lin.in_features)):
                h = al.act_linear(h, lin.weight, lin.bias)
            else:
                h = lin(act(h))
        return h

    def _edge_weights(self, node_feats, src, dst, edge_radial, etp_meta):
        return self._radial_tail(self.radial_mlp[0](edge_radial))

    def forward(self, node_feats: torch.Tensor, edge_index: torch.Tensor,
                edge_sh: torch.Tensor, edge_radial: torch.Tensor,
                edges_sorted: bool = False,
                etp_meta=None) -> torch.Tensor:
        from ...ops.etp import _kernel_ok, etp_indexed
        src, dst = edge_index[0], edge_index[1]
        n, c, _ = node_feats.shape
        x = self.linear_up(node_feats)
        w = self._edge_weights(node_feats, src, dst, edge_radial,
                               etp_meta).view(
            -1, c, self.conv_tp.num_paths)
        import os
        if etp_meta is not None and _kernel_ok(
                self.conv_tp.etp_table, x, edge_sh, w) and \
                os.environ.get("HYDRAGNN_FUSED_ETP", "0") == "1":
            # fused gather + tensor product + segment sum (one kernel;
            # gradients stay in the fused family — ops/etp.py)
            m = etp_indexed(x, edge_sh, w, self.conv_tp.etp_table,
                            etp_meta)
        else:
            src_csr = getattr(etp_meta, "src_csr", None) \
                if etp_meta is not None else None
            x_src = gather(x.reshape(n, -1), src,
                           backward_csr=src_csr).view(-1, c,
                                                      x.shape[-1])
            mji = self.conv_tp(x_src, edge_sh, w)
            m = scatter(mji.reshape(mji.shape[0], -1), dst, n, "sum",
                        sorted_index=edges_sorted).view(n, c, -1)
        m = m / self.avg_num_neighbors
        # skip: per-l linear on the input, padded to lmax_out.  Returned
        # SEPARATELY (reference blocks.py:379-412): the product basis
        # contracts the message alone and adds sc as a residual in its
        # own linear's epilogue.
        sc = self.skip_linear(node_feats[:, :, :dim(min(self.lmax_node,
                                                        self.lmax_out))])
        want = dim(self.lmax_out)
        if sc.shape[-1] < want:
            sc = torch.nn.functional.pad(sc, (0, want - sc.shape[-1]))
        return self.linear(m), sc


class RealAgnosticAttResidualInteractionBlock(
        RealAgnosticResidualInteractionBlock):
    """The reference MACEStack's default interaction (reference
    blocks.py:311): the per-edge tensor-product weights attend to BOTH
    endpoints — the radial-MLP input is [radial embedding,
    down-projected sender scalars, down-projected receiver scalars].
    Everything downstream (TP, aggregation, skip) matches the residual
    block."""

    def _setup_extra(self, num_channels: int):
        self._radial_extra = 2 * num_channels
        self.linear_down = MFMALinear(num_channels, num_channels,
                                      bias=False)

    def _edge_weights(self, node_feats, src, dst, edge_radial, etp_meta):
        down = self.linear_down(node_feats[:, :, 0])  # [N, C] scalars
        src_csr = getattr(etp_meta, "src_csr", None) \
            if etp_meta is not None else None
        dst_csr = getattr(etp_meta, "dst_csr", None) \
            if etp_meta is not None else None
        # first MLP layer is linear, so split it: the endpoint-scalar
        # contributions are computed per NODE (N-sized GEMMs) and
        # gathered as 64-wide outputs — identical numerics to
        # cat([radial, down[src], down[dst]]) @ W1^T at ~1/13 the GEMM
        # work (E >> N)
        from ...ops.splitk_linear import _SplitKLinearFn
        lin1 = self.radial_mlp[0]
        W1 = lin1.weight
        rd = W1.shape[1] - 2 * down.shape[1]
        c = down.shape[1]
        # split-K weight grads: F.linear's dW here is a [64, E] @
        # [E, 8] GEMM with K = num_edges — hipBLASLt runs it on
        # (M/16)x(N/16) workgroups, a serial-K crawl (measured
        # ~1.4 ms/step at b1024)
        if edge_radial.is_cuda:
            h = _SplitKLinearFn.apply(edge_radial, W1[:, :rd],
                                      lin1.bias)
            h_s = _SplitKLinearFn.apply(down, W1[:, rd:rd + c], None)
            h_d = _SplitKLinearFn.apply(down, W1[:, rd + c:], None)
        else:
            h = torch.nn.functional.linear(edge_radial, W1[:, :rd],
                                           lin1.bias)
            h_s = torch.nn.functional.linear(down, W1[:, rd:rd + c])
            h_d = torch.nn.functional.linear(down, W1[:, rd + c:])
        h = h + gather(h_s, src, backward_csr=src_csr) \
            + gather(h_d, dst, backward_csr=dst_csr)
        return self._radial_tail(h)


class EquivariantProductBasisBlock(nn.Module):
    def __init__(self, num_channels: int, lmax_in: int, lmax_out: int,
                 correlation: int, num_elements: int):
        super().__init__()
        self.symmetric_contractions = SymmetricContraction(
            lmax_in, lmax_out, correlation, num_channels, num_elements)
        self.linear = IrrepsLinear(num_channels, num_channels, lmax_out)

    def forward(self, node_feats: torch.Tensor, node_elem: torch.Tensor,
                sc: Optional[torch.Tensor] = None,
                elem_csr=None) -> torch.Tensor:
        out = self.symmetric_contractions(node_feats, node_elem,
                                          elem_csr=elem_csr)
        want = self.linear.lmap.numel()
        add = sc[:, :, :want] if sc is not None else None
        return self.linear(out, add=add)


class LinearReadoutBlock(nn.Module):
    """Scalar readout from the l=0 channel (reference blocks.py:442)."""

    def __init__(self, num_channels: int, out_dim: int):
        super().__init__()
        self.linear = MFMALinear(num_channels, out_dim)

    def forward(self, node_feats: torch.Tensor) -> torch.Tensor:
        return self.linear(node_feats[:, :, 0])


class NonLinearReadoutBlock(nn.Module):
    def __init__(self, num_channels: int, hidden: int, out_dim: int,
                 act=None):
        super().__init__()
        self.linear_1 = MFMALinear(num_channels, hidden)
        self.act = act or nn.SiLU()
        self.linear_2 = MFMALinear(hidden, out_dim)

    def forward(self, node_feats: torch.Tensor) -> torch.Tensor:
        return self.linear_2(self.act(self.linear_1(node_feats[:, :, 0])))


# ---------------------------------------------------------------------------
# Reference-named radial/embedding module wrappers
# (reference utils/model/mace_utils/modules/radial.py and blocks.py) —
# thin Modules over this framework's differentiable basis ops so a
# migrating user finds the classes they imported.
# ---------------------------------------------------------------------------
class PolynomialCutoff(nn.Module):
    def __init__(self, r_max: float, p: int = 6):
        super().__init__()
        self.r_max = float(r_max)
        self.p = float(p)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return polynomial_cutoff(x, self.r_max, self.p)


class GaussianBasis(nn.Module):
    def __init__(self, r_max: float, num_basis: int = 128,
                 trainable: bool = False):
        super().__init__()
        offsets = torch.linspace(0.0, r_max, num_basis)
        if trainable:
            self.offsets = nn.Parameter(offsets)
        else:
            self.register_buffer("offsets", offsets)
        self.coeff = -0.5 / float(offsets[1] - offsets[0]) ** 2

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return gaussian_basis(x, self.offsets.view(1, -1).to(x.dtype),
                              self.coeff)


class ChebychevBasis(nn.Module):
    def __init__(self, r_max: float, num_basis: int = 8):
        super().__init__()
        self.r_max = float(r_max)
        self.num_basis = num_basis

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return chebyshev_basis(x, self.r_max, self.num_basis)


# Cordero et al. 2008 single-bond covalent radii in Angstrom, indexed by
# atomic number (index 0 = placeholder); 0.2 where no published value.
COVALENT_RADII = [
    0.2,
    0.31, 0.28, 1.28, 0.96, 0.84, 0.76, 0.71, 0.66, 0.57, 0.58,
    1.66, 1.41, 1.21, 1.11, 1.07, 1.05, 1.02, 1.06,
    2.03, 1.76, 1.70, 1.60, 1.53, 1.39, 1.61, 1.52, 1.50, 1.24, 1.32,
    1.22, 1.22, 1.20, 1.19, 1.20, 1.20, 1.16,
    2.20, 1.95, 1.90, 1.75, 1.64, 1.54, 1.47, 1.46, 1.42, 1.39, 1.45,
    1.44, 1.42, 1.39, 1.39, 1.38, 1.39, 1.40,
    2.44, 2.15, 2.07, 2.04, 2.03, 2.01, 1.99, 1.98, 1.98, 1.96, 1.94,
    1.92, 1.92, 1.89, 1.90, 1.87, 1.87, 1.75, 1.70, 1.62, 1.51, 1.44,
    1.41, 1.36, 1.36, 1.32, 1.45, 1.46, 1.48, 1.40, 1.50, 1.50,
    2.60, 2.21, 2.15, 2.06, 2.00, 1.96, 1.90, 1.87, 1.80, 1.69,
] + [0.2] * 22  # Z=97..118 unknown


def _edge_r0(z, edge_index, covalent_radii, scale):
    """Per-edge covalent length scale: scale * (r_cov[Z_u] + r_cov[Z_v]).
    z holds 1-based atomic numbers per node."""
    zc = z.clamp(0, covalent_radii.numel() - 1)
    rc = covalent_radii.index_select(0, zc)
    return scale * (rc[edge_index[0]] + rc[edge_index[1]]).unsqueeze(-1)


class AgnesiTransform(nn.Module):
    """Agnesi distance transform (ACEpotentials.jl / JCP 2023; reference
    radial.py:161-208): r -> (1 + a (r/r0)^q / (1 + (r/r0)^(q-p)))^-1
    with r0 = mean covalent radius of the edge endpoints."""

    def __init__(self, q: float = 0.9183, p: float = 4.5791,
                 a: float = 1.0805, trainable: bool = False):
        super().__init__()
        t = torch.tensor
        if trainable:
            self.q, self.p, self.a = (nn.Parameter(t(q)),
                                      nn.Parameter(t(p)),
                                      nn.Parameter(t(a)))
        else:
            self.register_buffer("q", t(q))
            self.register_buffer("p", t(p))
            self.register_buffer("a", t(a))
        self.register_buffer("covalent_radii",
                             torch.tensor(COVALENT_RADII))

    def forward(self, x, node_attrs=None, edge_index=None,
                atomic_numbers=None, z=None):
        if z is None and node_attrs is not None and \
                atomic_numbers is not None:
            z = atomic_numbers[torch.argmax(node_attrs, dim=1)]
        if z is not None and edge_index is not None:
            r0 = _edge_r0(z, edge_index,
                          self.covalent_radii.to(x.dtype), 0.5)
        else:
            r0 = 1.0
        xs = x / r0
        return 1.0 / (1.0 + self.a * xs.pow(self.q)
                      / (1.0 + xs.pow(self.q - self.p)))


class SoftTransform(nn.Module):
    """Soft distance transform (reference radial.py:214-258):
    y = x + tanh(-(x/r0) - a (x/r0)^b)/2 + 1/2,
    r0 = (r_cov[Z_u] + r_cov[Z_v]) / 4."""

    def __init__(self, a: float = 0.2, b: float = 3.0,
                 trainable: bool = False):
        super().__init__()
        t = torch.tensor
        if trainable:
            self.a, self.b = nn.Parameter(t(a)), nn.Parameter(t(b))
        else:
            self.register_buffer("a", t(a))
            self.register_buffer("b", t(b))
        self.register_buffer("covalent_radii",
                             torch.tensor(COVALENT_RADII))

    def forward(self, x, node_attrs=None, edge_index=None,
                atomic_numbers=None, z=None):
        if z is None and node_attrs is not None and \
                atomic_numbers is not None:
            z = atomic_numbers[torch.argmax(node_attrs, dim=1)]
        if z is not None and edge_index is not None:
            r0 = _edge_r0(z, edge_index,
                          self.covalent_radii.to(x.dtype), 0.25)
        else:
            r0 = 1.0
        xs = x / r0
        return x + 0.5 * torch.tanh(-xs - self.a * xs.pow(self.b)) + 0.5


class LinearNodeEmbeddingBlock(nn.Module):
    """One-hot element -> channel embedding (reference blocks.py)."""

    def __init__(self, num_elements: int, num_channels: int):
        super().__init__()
        self.linear = nn.Linear(num_elements, num_channels, bias=False)

    def forward(self, node_attrs: torch.Tensor) -> torch.Tensor:
        return self.linear(node_attrs)


class AtomicEnergiesBlock(nn.Module):
    """Per-element reference energies: E0 contribution of each atom."""

    def __init__(self, atomic_energies):
        super().__init__()
        self.register_buffer(
            "atomic_energies",
            torch.as_tensor(atomic_energies, dtype=torch.get_default_dtype()))

    def forward(self, one_hot: torch.Tensor) -> torch.Tensor:
        return one_hot @ self.atomic_energies.view(-1, 1)


class ScaleShiftBlock(nn.Module):
    def __init__(self, scale: float, shift: float):
        super().__init__()
        self.register_buffer("scale", torch.tensor(float(scale)))
        self.register_buffer("shift", torch.tensor(float(shift)))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.scale * x + self.shift


# reference-named readout aliases
LinearMLPNode = LinearReadoutBlock
NonLinearMLPNode = NonLinearReadoutBlock
