"""ops/segment_plan.py on the CPU: the (src, dst) pair of plans, the
tri-state flag reader behind the stacks' fused_* switches, the path
counter, and that the op modules share one SegmentPlan and one
acc_dtype."""

import importlib

import pytest
import torch

from hydragnn_amd.ops import (edge_affine, pna_aggr, segment_linear,
                              segment_plan)
from hydragnn_amd.ops.segment_plan import (PathCounter, SegmentPlan,
                                           acc_dtype, env_default)

# `ops.gather_mul` and `ops.painn_message` name the exported functions
gather_mul_mod = importlib.import_module("hydragnn_amd.ops.gather_mul")
painn_message_mod = importlib.import_module("hydragnn_amd.ops.painn_message")

# E = 7 edges over N = 4 nodes, row 2 of the destinations empty
SORTED = torch.tensor([[3, 0, 1, 2, 0, 3, 1],
                       [0, 0, 1, 1, 1, 3, 3]])
UNSORTED = torch.tensor([[3, 0, 1, 2, 0, 3, 1],
                         [3, 0, 1, 3, 1, 0, 1]])
EMPTY = torch.zeros(2, 0, dtype=torch.long)


def _same_plan(got, want):
    assert torch.equal(got.index, want.index)
    assert (got.size, got.n_edges) == (want.size, want.n_edges)
    assert got.sorted_index == want.sorted_index
    assert got.is_identity == want.is_identity
    (gp, gr), (wp, wr) = got.csr(), want.csr()
    assert (gp is None) == (wp is None)
    if gp is not None:
        assert torch.equal(gp, wp)
    assert torch.equal(gr, wr)


@pytest.mark.parametrize("edge_index,is_sorted", [
    (SORTED, True), (UNSORTED, False), (EMPTY, True), (EMPTY, False)],
    ids=["sorted", "unsorted", "empty-sorted", "empty-unsorted"])
def test_pair_is_the_two_from_index_calls(edge_index, is_sorted):
    n = 4
    src, dst = SegmentPlan.pair(edge_index, n, is_sorted)
    _same_plan(src, SegmentPlan.from_index(edge_index[0], n))
    _same_plan(dst, SegmentPlan.from_index(edge_index[1], n,
                                           sorted_index=is_sorted))
    # the CSR itself: row 2 of the sorted destinations is empty
    perm, rowptr = dst.csr()
    order = edge_index[1] if perm is None else edge_index[1][perm]
    assert torch.equal(order, edge_index[1].sort(stable=True).values)
    assert rowptr.tolist() == [
        int((edge_index[1] < i).sum()) for i in range(n + 1)]
    if edge_index is SORTED:
        assert perm is None and rowptr.tolist() == [0, 2, 5, 5, 7]


def test_pair_defaults_to_unsorted():
    _, dst = SegmentPlan.pair(SORTED, 4)
    assert not dst.sorted_index and dst.csr()[0] is not None


FLAGS = [(gather_mul_mod.fused_messages, "HYDRAGNN_GATHER_MUL"),
         (painn_message_mod.fused_painn, "HYDRAGNN_PAINN_FUSED"),
         (edge_affine.fused_egnn, "HYDRAGNN_EGNN_FUSED")]


@pytest.mark.parametrize("fused,name", FLAGS, ids=[n for _, n in FLAGS])
def test_fused_flags_are_tri_state(fused, name, monkeypatch):
    monkeypatch.delenv(name, raising=False)
    assert fused(True) is True and fused(False) is False
    assert env_default(name, True) is True
    monkeypatch.setenv(name, "0")
    assert fused(True) is False and fused(False) is False
    for value in ("1", ""):
        monkeypatch.setenv(name, value)
        assert fused(True) is True and fused(False) is True
    # read at call time, and only under the op's own name
    monkeypatch.delenv(name)
    monkeypatch.setenv(name + "_X", "0")
    assert fused(True) is True


def test_pna_flag_defaults_on(monkeypatch):
    monkeypatch.delenv("HYDRAGNN_PNA_FUSED", raising=False)
    assert pna_aggr.fused_pna() is True
    monkeypatch.setenv("HYDRAGNN_PNA_FUSED", "0")
    assert pna_aggr.fused_pna() is False
    monkeypatch.setenv("HYDRAGNN_PNA_FUSED", "1")
    assert pna_aggr.fused_pna() is True


def test_path_counter():
    c = PathCounter("fwd", "composition")
    c.hit("fwd")
    c.hit("fwd")
    c.hit("composition")
    snap = c.snapshot()
    assert snap == {"fwd": 2, "composition": 1} and type(snap) is dict
    snap["fwd"] = 99                       # a copy
    assert c.snapshot()["fwd"] == 2
    with pytest.raises(KeyError):
        c.hit("bwd")
    assert "bwd" not in c.snapshot()
    c.reset()
    assert c.snapshot() == {"fwd": 0, "composition": 0}


def test_op_counters_keep_their_keys():
    assert set(gather_mul_mod.path_counts()) == {"sum", "mul", "composition"}
    assert set(painn_message_mod.path_counts()) == {
        "fwd", "bwd_node", "bwd_edge", "composition"}
    assert set(edge_affine.path_counts()) == {
        "fwd", "node", "edge", "param", "composition"}
    assert set(pna_aggr.path_counts()) == {
        "fwd", "bwd", "bwd2", "composition"}
    pna_aggr.reset_path_counts()
    pna_aggr.count_composition()
    assert pna_aggr.path_counts()["composition"] == 1
    pna_aggr.reset_path_counts()
    assert pna_aggr.path_counts()["composition"] == 0


def test_one_plan_class_and_one_acc_dtype():
    assert gather_mul_mod.SegmentPlan is segment_plan.SegmentPlan
    for mod in (gather_mul_mod, pna_aggr, segment_linear):
        assert mod.acc_dtype is segment_plan.acc_dtype
    assert acc_dtype(torch.bfloat16) == acc_dtype(torch.float16) \
        == acc_dtype(torch.float32) == torch.float32
    assert acc_dtype(torch.float64) == torch.float64
