"""What the segment ops share on the Python side (``gather_mul``,
``painn_message``, ``edge_affine``, ``pna_aggr``): the ``SegmentPlan``
that groups edges into CSR rows, the accumulator dtype, the kernels'
envelope, the tri-state flag reader of the model stacks and the path
counter.  A new segment op starts here and from csrc/segment_common.h.
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from ._extension import use_eager
from .scatter import _rowptr_from_sorted

__all__ = ["SegmentPlan", "acc_dtype", "KERNEL_DTYPES", "kernel_route",
           "env_default", "PathCounter"]

KERNEL_DTYPES = (torch.float32, torch.float64, torch.bfloat16,
                 torch.float16)


def acc_dtype(dtype: torch.dtype) -> torch.dtype:
    """fp32 for the half types, the dtype itself otherwise."""
    return torch.float32 if dtype in (torch.bfloat16, torch.float16) \
        else dtype


def kernel_route(t: torch.Tensor, n_edges: int) -> bool:
    """The envelope every segment kernel shares; an op with a narrower
    one adds its clauses on top."""
    return (t.is_cuda and not use_eager() and t.dtype in KERNEL_DTYPES
            and n_edges < 2 ** 31)


def env_default(name: str, default: bool) -> bool:
    """Tri-state flag: unset leaves ``default``, "0" is False and any
    other value True.  Read at call time."""
    value = os.environ.get(name)
    return default if value is None else value != "0"


class PathCounter(dict):
    """Calls per route of one op, over a fixed set of keys."""

    def __init__(self, *keys: str):
        super().__init__((k, 0) for k in keys)

    def hit(self, key: str) -> None:
        self[key] = self[key] + 1      # an unknown key raises KeyError

    def snapshot(self) -> dict:
        return dict(self)

    def reset(self) -> None:
        for k in self:
            self[k] = 0


class SegmentPlan:
    """One grouping of E edges into ``size`` rows: ``index[e]`` is the
    row of edge e.  ``csr()`` gives ``(perm | None, rowptr[size + 1])``
    with ``perm = argsort(index, stable=True)`` (None for a sorted
    index), built on first use and kept.  Nothing here syncs with the
    host."""

    def __init__(self, index: torch.Tensor, size: int,
                 sorted_index: bool = False, _identity: bool = False):
        if index.dim() != 1:
            raise ValueError("index must be [E]")
        if index.dtype != torch.long:
            index = index.long()
        self.index = index.contiguous()
        self.size = int(size)
        self.sorted_index = bool(sorted_index) or _identity
        self.is_identity = _identity
        self._csr: Optional[Tuple[Optional[torch.Tensor],
                                  torch.Tensor]] = None

    @classmethod
    def from_index(cls, index: torch.Tensor, size: int,
                   sorted_index: bool = False) -> "SegmentPlan":
        return cls(index, size, sorted_index)

    @classmethod
    def identity(cls, n_edges: int, device=None) -> "SegmentPlan":
        """index = arange(E): row e holds edge e alone."""
        plan = cls(torch.arange(n_edges, device=device), n_edges,
                   _identity=True)
        plan._csr = (None, torch.arange(n_edges + 1, device=device))
        return plan

    @classmethod
    def pair(cls, edge_index: torch.Tensor, num_nodes: int,
             edges_sorted: bool = False):
        """The (src, dst) plans of one batch's edges over its nodes,
        shared by every layer of a forward; ``edges_sorted`` says that
        ``edge_index[1]`` ascends."""
        return (cls(edge_index[0], num_nodes),
                cls(edge_index[1], num_nodes, bool(edges_sorted)))

    @property
    def n_edges(self) -> int:
        return self.index.shape[0]

    def csr(self):
        if self._csr is None:
            with torch.no_grad():
                if self.sorted_index:
                    perm, sidx = None, self.index
                else:
                    perm = torch.argsort(self.index, stable=True)
                    sidx = self.index.index_select(0, perm)
                self._csr = (perm, _rowptr_from_sorted(sidx, self.size))
        return self._csr


def check_plans(src, dst) -> None:
    if not (isinstance(src, SegmentPlan) and isinstance(dst, SegmentPlan)):
        raise TypeError("src and dst must be SegmentPlans")
    if src.n_edges != dst.n_edges:
        raise ValueError(
            f"the plans group {src.n_edges} and {dst.n_edges} edges")
