"""The two product-block contractions of the flagship config alone, at
the batch-1024 shapes: forward, force pass (create_graph) and loss
backward, eager, ITERS times after two warm-up iterations.

Run it under `rocprofv3 --kernel-trace --stats` to attribute kernels to
the symmetric contraction (profiles/README.md, "Fused symmetric
contraction"); `HYDRAGNN_SYMCON=0` traces the composition.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hydragnn_amd.models.mace.symmetric_contraction import (  # noqa: E402
    SymmetricContraction)

ITERS = int(os.environ.get("ITERS", "5"))
N, C = int(os.environ.get("NODES", str(21 * 1024))), 64
dev = "cuda:0"
torch.manual_seed(0)
mods = [SymmetricContraction(1, 1, 2, C, 118).to(dev, torch.bfloat16),
        SymmetricContraction(1, 0, 2, C, 118).to(dev, torch.bfloat16)]
# hydrogen, carbon, oxygen
elem = torch.tensor([0, 5, 7], device=dev)[
    torch.randint(0, 3, (N,), device=dev)]
xs = [torch.randn(N, C, 4, device=dev, dtype=torch.bfloat16) * 0.5
      for _ in mods]
rs = [torch.randn(N, C, d, device=dev, dtype=torch.bfloat16)
      for d in (4, 1)]
elem_csr = mods[0].element_sort(elem)


def step():
    loss = 0
    for m, x, r in zip(mods, xs, rs):
        x = x.detach().requires_grad_(True)
        out = m(x, elem, elem_csr=elem_csr)
        e = (out * r).float().sum()
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
print(f"symcon_block: {t0.elapsed_time(t1) / ITERS:.3f} ms/iter eager, "
      f"N={N} ITERS={ITERS} (+2 warm-up)")
