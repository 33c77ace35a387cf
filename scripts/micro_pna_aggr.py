"""Micro-benchmark of the fused PNA aggregation: forward, first-order
backward and second-order backward of DegreeScalerAggregation with the
four default aggregators and scalers at E ~ 1e6, F = 64, timed with
device events.  HYDRAGNN_PNA_FUSED=0 times the composition of generic
scatter ops instead.

Usage: python scripts/micro_pna_aggr.py [--edges 1000000] [--feat 64]
           [--dtype fp32|bf16] [--iters 20] [--unsorted]
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

from hydragnn_amd.models.layers import DegreeScalerAggregation  # noqa: E402
from hydragnn_amd.ops import path_counts  # noqa: E402


def timed(fn, iters, warmup=3):
    """Median milliseconds per call over `iters` timed calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    times.sort()
    return times[len(times) // 2]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--edges", type=int, default=1_000_000)
    parser.add_argument("--feat", type=int, default=64)
    parser.add_argument("--avg-degree", type=int, default=16)
    parser.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    parser.add_argument("--iters", type=int, default=20)
    parser.add_argument("--unsorted", action="store_true",
                        help="shuffled edges: the perm route")
    args = parser.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    dtype = torch.float32 if args.dtype == "fp32" else torch.bfloat16
    g = torch.Generator().manual_seed(5)
    n = args.edges // args.avg_degree
    index = torch.randint(0, n, (args.edges,), generator=g)
    if not args.unsorted:
        index = index.sort().values
    index = index.to(dev)
    mod = DegreeScalerAggregation(
        ["mean", "min", "max", "std"],
        ["identity", "amplification", "attenuation", "linear"],
        torch.bincount(torch.bincount(index.cpu(), minlength=n))).to(dev)
    mod._edges_sorted = not args.unsorted
    x = torch.randn(args.edges, args.feat, generator=g).to(dev, dtype)
    x.requires_grad_(True)
    w = torch.randn(n, 16 * args.feat, generator=g).to(dev, dtype)
    w.requires_grad_(True)
    c = torch.randn(args.edges, args.feat, generator=g).to(dev, dtype)

    def fwd():
        with torch.no_grad():
            return mod(x, index, n)

    out = mod(x, index, n)

    def bwd():
        return torch.autograd.grad(out, x, w, retain_graph=True)

    (dx,) = torch.autograd.grad(out, x, w, create_graph=True)

    def bwd2():
        return torch.autograd.grad(dx, (x, w), c, retain_graph=True)

    res = {"edges": args.edges, "rows": n, "feat": args.feat,
           "dtype": args.dtype, "sorted": not args.unsorted,
           "fused": os.environ.get("HYDRAGNN_PNA_FUSED", "1") != "0",
           "fwd_ms": timed(fwd, args.iters),
           "bwd_ms": timed(bwd, args.iters),
           "bwd2_ms": timed(bwd2, args.iters),
           "path_counts": path_counts()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
