"""The two radial-MLP evaluations of the flagship config alone
(`RealAgnosticAttResidualInteractionBlock._edge_weights` of both
interactions), at the batch-1024 shapes: N = 21 * 1024 nodes,
E = 332,668 edges, C = 64, bf16, seeded random src and a sorted dst.
Each iteration runs the forward, the create_graph gradient with respect
to the radial embedding (the force pass) and the backward of a loss on
that gradient; eager, ITERS times after two warm-up iterations.

Run it under `rocprofv3 --kernel-trace --stats` to attribute kernels to
the block (profiles/README.md, "Fused SiLU-linear");
`HYDRAGNN_ACT_LINEAR=0` traces the composition.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hydragnn_amd.models.mace.blocks import (  # noqa: E402
    RealAgnosticAttResidualInteractionBlock)

ITERS = int(os.environ.get("ITERS", "5"))
N = int(os.environ.get("NODES", str(21 * 1024)))
E = int(os.environ.get("EDGES", "332668"))
C, RADIAL = 64, 8
dev = "cuda:0"
torch.manual_seed(0)
# (lmax_node, lmax_edge, lmax_out) of the two interactions
blocks = [RealAgnosticAttResidualInteractionBlock(
    C, lmax_node, 2, 1, RADIAL, 20.0).to(dev, torch.bfloat16)
    for lmax_node in (0, 1)]
src = torch.randint(0, N, (E,), device=dev)
dst = torch.randint(0, N, (E,), device=dev).sort().values
feats = [torch.randn(N, C, (l + 1) ** 2, device=dev, dtype=torch.bfloat16)
         for l in (0, 1)]
radial = torch.randn(E, RADIAL, device=dev, dtype=torch.bfloat16)
outs = [torch.randn(E, C * b.conv_tp.num_paths, device=dev,
                    dtype=torch.bfloat16) for b in blocks]


def step():
    loss = 0
    x = radial.detach().requires_grad_(True)
    for blk, f, r in zip(blocks, feats, outs):
        w = blk._edge_weights(f, src, dst, x, None)
        e = (w * r).float().sum()
        (gx,) = torch.autograd.grad(e, x, create_graph=True)
        loss = loss + e + (gx.float() ** 2).sum()
    loss.backward()


for _ in range(2):
    step()
torch.cuda.synchronize()
t0 = torch.cuda.Event(enable_timing=True)
t1 = torch.cuda.Event(enable_timing=True)
t0.record()
for _ in range(ITERS):
    step()
t1.record()
torch.cuda.synchronize()
paths = [b.conv_tp.num_paths for b in blocks]
print(f"radial_mlp_block: {t0.elapsed_time(t1) / ITERS:.3f} ms/iter eager, "
      f"N={N} E={E} paths={paths} ITERS={ITERS} (+2 warm-up)")
