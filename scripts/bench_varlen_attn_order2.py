#!/usr/bin/env python
"""Op-level force-style step of segment-varlen attention: forward,
``autograd.grad(create_graph=True)``, then backward of the squared
gradient -- the second-order HIP kernels (default) against the torch
recompute route (``HYDRAGNN_VARLEN_ATTN_BWD2=0``).

H = 4, head_dim = 16, fp32 and bf16, at two batch shapes: 32 graphs of
80 rows, and 28 graphs of 40 rows plus 4 of 400.  The two routes
alternate in one process; each repeat times a window of at least
``--seconds`` with device events after a warm-up of both routes.  Prints
one JSON line per (shape, dtype) with every repeat's ms/step.

    python scripts/bench_varlen_attn_order2.py --repeats 3 --seconds 1.0
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(
    __file__))))

from hydragnn_amd.ops.varlen_attn import varlen_attention_fn  # noqa: E402

SHAPES = {"32x80": [80] * 32, "28x40+4x400": [40] * 28 + [400] * 4}
H, DH = 4, 16
SWITCH = "HYDRAGNN_VARLEN_ATTN_BWD2"


def make_step(sizes, dtype):
    torch.manual_seed(0)
    s = torch.tensor(sizes)
    ptr = torch.zeros(len(sizes) + 1, dtype=torch.long)
    ptr[1:] = s.cumsum(0)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), s).cuda()
    ptr = ptr.cuda()
    n = sum(sizes)
    q, k, v = (torch.randn(n, H, DH, device="cuda", dtype=dtype)
               .requires_grad_(True) for _ in range(3))
    w = torch.randn(n, H, DH, device="cuda", dtype=dtype)

    def step():
        out = varlen_attention_fn(q, k, v, ptr, batch)
        first = torch.autograd.grad((out * w).sum(), (q, k, v),
                                    create_graph=True)
        loss = sum(g.float().square().sum() for g in first)
        return torch.autograd.grad(loss, (q, k, v))

    return step


def set_route(kernel):
    if kernel:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = "0"


def timed(step, seconds, chunk):
    """ms/step over a window of at least ``seconds``."""
    start, stop = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    steps, total = 0, 0.0
    while total < seconds * 1e3:
        start.record()
        for _ in range(chunk):
            step()
        stop.record()
        stop.synchronize()
        total += start.elapsed_time(stop)
        steps += chunk
    return total / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    assert args.repeats >= 3 and args.seconds >= 1.0
    for name, sizes in SHAPES.items():
        for dtype in (torch.float32, torch.bfloat16):
            step = make_step(sizes, dtype)
            for kernel in (True, False):
                set_route(kernel)
                for _ in range(args.warmup):
                    step()
            torch.cuda.synchronize()
            ms = {"kernel": [], "torch": []}
            for _ in range(args.repeats):
                for kernel in (True, False):
                    set_route(kernel)
                    ms["kernel" if kernel else "torch"].append(
                        round(timed(step, args.seconds, args.chunk), 4))
            set_route(True)
            med = {r: sorted(x)[len(x) // 2] for r, x in ms.items()}
            print(json.dumps({
                "shape": name, "dtype": str(dtype).split(".")[1],
                "rows": sum(sizes), "heads": H, "head_dim": DH,
                "ms_per_step_kernel": ms["kernel"],
                "ms_per_step_torch": ms["torch"],
                "median_kernel": med["kernel"],
                "median_torch": med["torch"],
                "torch_over_kernel": round(med["torch"] / med["kernel"],
                                           3)}), flush=True)


if __name__ == "__main__":
    main()
