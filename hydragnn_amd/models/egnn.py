"""E(n)-equivariant GNN stack (EGCL).

Re-implementation of the EGNN operator (Satorras et al. 2021) with the
reference's capability surface (/root/reference/hydragnn/models/
EGCLStack.py:22-300): edge MLP on [h_i, h_j, |r_ij|^2, e_ij], optional
coordinate update coord += mean_j(r_ij * phi_x(m_ij)) when equivariance
is on, node MLP on [h, sum_j m_ij]; PBC edge shifts supported.
"""

from __future__ import annotations

from typing import Optional

import torch
from torch import nn
from torch.nn import functional as F

from ..ops import act_linear as al
from ..ops.edge_affine import (MAX_EDGE_DIM, edge_pair_affine, fused_egnn,
                               wide_envelope)
from ..ops.segment_plan import SegmentPlan
from ..ops.mfma_linear import (MFMALinear, _bf16_ok, _eligible,
                               mfma_linear_bf16)
from ..ops._extension import use_eager

from ..ops import gather, get_edge_vectors_and_lengths, scatter
from .base import Base

# HYDRAGNN_EGNN_FUSED unset: see profiles/README.md for the measurement
FUSED_BY_DEFAULT = False


class E_GCL(nn.Module):
    def __init__(self, input_nf: int, output_nf: int, hidden_nf: int,
                 edge_dim: int = 0, equivariant: bool = False,
                 act=nn.SiLU()):
        super().__init__()
        self.equivariant = equivariant
        in_edge = 2 * input_nf + 1 + edge_dim
        self.edge_mlp = nn.Sequential(
            MFMALinear(in_edge, hidden_nf), act,
            MFMALinear(hidden_nf, hidden_nf), act)
        self.node_mlp = nn.Sequential(
            MFMALinear(input_nf + hidden_nf, hidden_nf), act,
            MFMALinear(hidden_nf, output_nf))
        if equivariant:
            layer = MFMALinear(hidden_nf, 1, bias=False)
            nn.init.xavier_uniform_(layer.weight, gain=0.001)
            self.coord_mlp = nn.Sequential(
                MFMALinear(hidden_nf, hidden_nf), act, layer)

    def _fused_edge_mlp(self, h, r2, edge_attr, edge_index, plans):
        """edge_mlp without the concatenation: the first layer splits by
        the blocks [W_i | W_j | w_r | W_e] of its weight into a node-side
        GEMM and `edge_pair_affine`; the second consumes the
        pre-activation on the fused SiLU GEMMs where they apply."""
        lin1, act, lin2 = self.edge_mlp[0], self.edge_mlp[1], self.edge_mlp[2]
        n, feat = h.shape
        if plans is None:
            plans = SegmentPlan.pair(edge_index, n,
                                     getattr(self, "_edges_sorted", False))
        hip_ok = h.is_cuda and not use_eager() and _bf16_ok(h)
        W = lin1.weight
        W_ij = torch.cat([W[:, :feat], W[:, feat:2 * feat]], dim=0)
        if hip_ok and _eligible(n, W_ij.shape[0], feat):
            P = mfma_linear_bf16(h, W_ij, None)
        else:
            P = F.linear(h, W_ij if torch.is_autocast_enabled()
                         else W_ij.to(h.dtype))
        # the parameter casts are differentiable ops out here, so second
        # order terms reach the fp32 leaves
        dt = P.dtype
        z = edge_pair_affine(
            P, r2.to(dt), None if edge_attr is None else edge_attr.to(dt),
            W[:, 2 * feat].to(dt),
            None if edge_attr is None else W[:, 2 * feat + 1:].to(dt),
            None if lin1.bias is None else lin1.bias.to(dt),
            plans[0], plans[1])
        hidden = lin2.out_features
        if (isinstance(act, nn.SiLU) and al.fused_route()
                and z.is_cuda and z.dtype == torch.bfloat16
                and not use_eager()
                and al.in_envelope(z.shape[0], hidden, hidden)):
            bias = lin2.bias
            return self.edge_mlp[3](al.act_linear(
                z, lin2.weight.to(dt), None if bias is None else bias.to(dt)))
        return self.edge_mlp[3](lin2(act(z)))

    def _wide_kernels(self, h, edge_dim):
        """Whether `_fused_edge_mlp` would run the MFMA pair-affine
        kernels on edge attributes wider than MAX_EDGE_DIM: a device
        tensor, not forced eager, `P` in bf16 or f16, (H, D) inside
        `wide_envelope`.  Anything else would land on the torch doubles
        and keeps the concatenation."""
        if not h.is_cuda or use_eager():
            return False
        if _bf16_ok(h):              # mfma_linear_bf16 or a bf16 F.linear
            dt = torch.bfloat16
        elif torch.is_autocast_enabled():
            dt = torch.get_autocast_dtype("cuda")
        else:
            dt = h.dtype
        return wide_envelope(dt, self.edge_mlp[0].out_features, edge_dim)

    def forward(self, h, pos, edge_index, edge_attr=None, edge_shifts=None,
                plans=None):
        src, dst = edge_index[0], edge_index[1]
        vec, lengths = get_edge_vectors_and_lengths(pos, edge_index,
                                                    edge_shifts)
        r2 = (lengths ** 2)
        edge_dim = 0 if edge_attr is None else edge_attr.shape[-1]
        if fused_egnn(FUSED_BY_DEFAULT) and (
                edge_dim <= MAX_EDGE_DIM or self._wide_kernels(h, edge_dim)):
            m = self._fused_edge_mlp(h, r2, edge_attr, edge_index, plans)
        else:
            hi = gather(h, dst)
            hj = gather(h, src)
            parts = [hi, hj, r2.to(h.dtype)]
            if edge_attr is not None:
                parts.append(edge_attr)
            m = self.edge_mlp(torch.cat(parts, dim=-1))
        if self.equivariant:
            trans = vec.to(h.dtype) * self.coord_mlp(m)
            pos = pos + scatter(
                trans, dst, h.shape[0], "mean",
                sorted_index=getattr(self, "_edges_sorted", False)
            ).to(pos.dtype)
        agg = scatter(m, dst, h.shape[0], "sum",
                      sorted_index=getattr(self, "_edges_sorted", False))
        h = self.node_mlp(torch.cat([h, agg], dim=-1))
        return h, pos


class _EGCLWrapper(nn.Module):
    def __init__(self, conv: E_GCL):
        super().__init__()
        self.conv = conv

    def forward(self, inv_node_feat, equiv_node_feat, edge_index,
                edge_attr=None, edge_shifts=None, plans=None, **kwargs):
        h, pos = self.conv(inv_node_feat, equiv_node_feat, edge_index,
                           edge_attr=edge_attr, edge_shifts=edge_shifts,
                           plans=plans)
        return h, pos


class EGCLStack(Base):
    _hipgraph_capture_safe = True  # uses only the given edge_index
    def __init__(self, edge_dim: Optional[int] = None,
                 max_neighbours: Optional[int] = None, **kwargs):
        self.is_edge_model = True
        self.egnn_equivariance = bool(kwargs.get("equivariance"))
        super().__init__(edge_dim=edge_dim, **kwargs)

    def get_conv(self, input_dim, output_dim, edge_dim=None):
        return _EGCLWrapper(E_GCL(
            input_dim, output_dim, output_dim,
            edge_dim=edge_dim or 0,
            equivariant=self.egnn_equivariance))

    def _embedding(self, data):
        conv_args = {
            "edge_index": data.edge_index,
            "edge_shifts": data.get("edge_shifts"),
        }
        if self.use_edge_attr:
            conv_args["edge_attr"] = data.edge_attr
        x = data.x
        if x is not None and not torch.is_floating_point(x):
            x = x.float()
        if self.use_global_attn and not self.is_equivariant_attn:
            x, conv_args = self._gps_encode(data, x, conv_args)
        if fused_egnn(FUSED_BY_DEFAULT):
            conv_args["plans"] = SegmentPlan.pair(
                data.edge_index, data.pos.shape[0],
                getattr(self, "_edges_sorted", False))
        return x, data.pos, conv_args

    def __str__(self):
        return "EGCLStack"


def unsorted_segment_sum(data, segment_ids, num_segments):
    """Reference EGCLStack helper name; HIP scatter underneath."""
    return scatter(data, segment_ids, num_segments, "sum")
