"""Micro-bench the default single-output ETP instances (general,
channel reduce, CSR form) on the run-time-table kernels at the headline
shape: median time per call and achieved bandwidth vs the HBM roofline.

    python scripts/micro_etp_reduce.py [reduce_block]

`reduce_block` sets HYDRAGNN_ETP_REDUCE_BLOCK, the block size of the
channel reduce (64, 128, 256 or 512)."""

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))

import torch  # noqa: E402


def median_us(call, warmup=10, iters=50):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3)
    return sorted(times)[len(times) // 2]


def run(reduce_block=None):
    if reduce_block is not None:
        os.environ["HYDRAGNN_ETP_REDUCE_BLOCK"] = str(reduce_block)
    from hydragnn_amd.models.mace.blocks import EdgeTensorProduct
    from hydragnn_amd.ops import etp as etp_mod

    tp = EdgeTensorProduct(2, 2, 2)  # lmax config of the headline
    table = tp.etp_table
    da, db, dg, do = table.dims
    E, C = 332358, 64
    N = E // 26  # nodes of the CSR form, about 26 edges each
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)

    def rand(*shape):
        return torch.randn(*shape, generator=g).bfloat16().to(dev)

    A, An = rand(E, C, da), rand(N, C, da)
    B, Cw, D = rand(E, db), rand(E, C, dg), rand(E, C, do)
    src = torch.randint(0, N, (E,), generator=g).to(dev)
    dst = torch.randint(0, N, (E,), generator=g).sort().values
    rowptr = torch.zeros(N + 1, dtype=torch.long)
    rowptr[1:] = torch.bincount(dst, minlength=N).cumsum(0)
    rowptr = rowptr.to(dev)
    ext = etp_mod.get_extension(required=True)
    ent, coefs = table.device_tensors(dev)

    row = 2 * C  # bytes of one bf16 (position, channel-row) per element
    cases = {
        "general": (
            lambda: ext.etp_general(A, B, Cw, ent, coefs, do,
                                    static_id=-1),
            E * (row * (da + dg + do) + 2 * db)),
        "reduce": (
            lambda: ext.etp_reduce(A, Cw, D, ent, coefs, db),
            E * (row * (da + dg + do) + 2 * db)),
        "csr": (
            lambda: ext.etp_nodesum(An, B, Cw, ent, coefs, do, rowptr,
                                    src),
            E * (row * (da + dg) + 2 * db) + N * row * do),
    }
    result = {"dims": [da, db, dg, do], "n_ent": table.entries.shape[0],
              "E": E, "C": C, "reduce_block": reduce_block or 512}
    for name, (call, nbytes) in cases.items():
        us = median_us(call)
        result[name + "_us"] = round(us, 1)
        print(f"{name:8s} {us:8.1f} us  {nbytes / us / 1e3:7.1f} GB/s  "
              f"({nbytes / 1e9:.2f} GB/call)")
    print(json.dumps(result))


if __name__ == "__main__":
    run(int(sys.argv[1]) if len(sys.argv) > 1 else None)
