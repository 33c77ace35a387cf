"""Microbenchmark of the fused gather-multiply-sum against the
composition of generic ops it replaces in the models, forward and
forward + backward, timed by device events:

  schnet_md17   the CFConv message of one `md17_shape` batch (the
                `schnet_mlip` config of bench_configs.py), F = 64,
                fp32 and bf16; composition: gather, multiply, scatter
                with the batch's sorted_index flag;
  dimenet_trip  the triplet sum of one `dimenet_fp64` batch (E edges,
                T triplets read from the batch), F = 64, fp64;
                composition: gather, multiply, atomic scatter.

The two routes alternate round by round on the same tensors; the line
of a case gives the median of the rounds and their min / max, so the
spread is visible next to the ratio.  The plans are built once, before
the timed window, as the models build them once per batch; the time of
building them (the argsort of the unsorted side and two row pointers)
is reported on its own.

Usage: python scripts/bench_gather_mul.py [--rounds 7] [--iters 50]
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(__file__))

from hydragnn_amd.data import Batch  # noqa: E402
from hydragnn_amd.ops import gather, scatter  # noqa: E402
from hydragnn_amd.ops.gather_mul import (SegmentPlan,  # noqa: E402
                                         gather_mul_sum, path_counts,
                                         reset_path_counts)

FEAT = 64


def _events(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters      # us per call


def _case(label, dtype, src, dst, m, n, dst_sorted, comp_sorted, rounds,
          iters):
    """dst_sorted: what the fused route's dst plan is told;
    comp_sorted: what the models' composition tells scatter."""
    dev = src.device
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randn(m, FEAT, generator=g).to(dev, dtype).requires_grad_(True)
    w = torch.randn(src.numel(), FEAT, generator=g).to(
        dev, dtype).requires_grad_(True)
    cot = torch.randn(n, FEAT, generator=g).to(dev, dtype)

    def plans():
        sp = SegmentPlan.from_index(src, m)
        dp = SegmentPlan.from_index(dst, n, sorted_index=dst_sorted)
        sp.csr()
        dp.csr()
        return sp, dp

    sp, dp = plans()

    def fused():
        return gather_mul_sum(x, w, sp, dp)

    def comp():
        return scatter(gather(x, src) * w, dst, n, "sum",
                       sorted_index=comp_sorted)

    def fwd(f):
        with torch.no_grad():
            f()

    def fwd_bwd(f):
        x.grad = w.grad = None
        f().backward(cot)

    reset_path_counts()
    times = {k: [] for k in ("fused_fwd", "comp_fwd", "fused_fwd_bwd",
                             "comp_fwd_bwd")}
    for f in (fused, comp):                       # warm-up, every shape
        for _ in range(5):
            fwd(f)
            fwd_bwd(f)
    torch.cuda.synchronize()
    for _ in range(rounds):
        times["fused_fwd"].append(_events(lambda: fwd(fused), iters))
        times["comp_fwd"].append(_events(lambda: fwd(comp), iters))
        times["fused_fwd_bwd"].append(_events(lambda: fwd_bwd(fused), iters))
        times["comp_fwd_bwd"].append(_events(lambda: fwd_bwd(comp), iters))
    assert path_counts()["composition"] == 0
    plan_us = statistics.median(_events(plans, 10) for _ in range(3))
    with torch.no_grad():
        diff = float((fused().double() - comp().double()).abs().max())
    row = {"case": label, "dtype": str(dtype).split(".")[-1],
           "M": m, "E": int(src.numel()), "N": n, "F": FEAT,
           "dst_sorted": bool(dst_sorted),
           "composition_sorted": bool(comp_sorted),
           "rounds": rounds, "iters": iters,
           "plan_build_us": round(plan_us, 1),
           "max_abs_diff_fused_vs_comp": diff}
    for k, v in times.items():
        row[k + "_us"] = {"median": round(statistics.median(v), 1),
                          "min": round(min(v), 1), "max": round(max(v), 1)}
    for k in ("fwd", "fwd_bwd"):
        row["speedup_" + k] = round(
            statistics.median(times["comp_" + k])
            / statistics.median(times["fused_" + k]), 3)
    print(json.dumps(row), flush=True)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=7)
    parser.add_argument("--iters", type=int, default=50)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gather_mul.py times device kernels: "
                         "no GPU found")
    import bench_configs as C
    from hydragnn_amd.models.dimenet import triplets
    dev = torch.device("cuda:0")

    cfg = C.CONFIGS["schnet_mlip"]
    batch = Batch.from_data_list(cfg["data"](cfg["local_batch"]))
    ei = batch.edge_index.to(dev)
    srt = bool(batch.get("edges_sorted_", False))
    for dtype in (torch.float32, torch.bfloat16):
        _case("schnet_md17", dtype, ei[0].contiguous(), ei[1].contiguous(),
              batch.num_nodes, batch.num_nodes, srt, srt, args.rounds,
              args.iters)

    cfg = C.CONFIGS["dimenet_fp64"]
    batch = Batch.from_data_list(cfg["data"](cfg["local_batch"]))
    ei = batch.edge_index.to(dev)
    idx_kj, idx_ji = triplets(ei, batch.num_nodes)
    n_edges = ei.shape[1]
    # idx_ji ascends by construction; the fused route says so, the
    # models' composition does not and takes the atomic route
    _case("dimenet_trip", torch.float64, idx_kj, idx_ji, n_edges, n_edges,
          True, False, args.rounds, args.iters)


if __name__ == "__main__":
    main()
