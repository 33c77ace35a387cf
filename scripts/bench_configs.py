"""Secondary benchmark configs (BASELINE.json configs[2..4]): PaiNN
multi-head QM9-shape, EGNN + GPS global attention, DimeNet fp64 with
gradient checkpointing on periodic cells; and the PNA family: PNAEq as
an MLIP (energy + forces, double backward) and PNAPlus on QM9-shaped
molecules, both through DegreeScalerAggregation (HYDRAGNN_PNA_FUSED=0
times the composition instead); and SchNet as an MLIP on the same
MD17-shaped molecules, through the fused gather-multiply-sum
(HYDRAGNN_GATHER_MUL=0 times the composition; this also switches
dimenet_fp64).  The driver's contract bench
(bench.py) stays MACE; this script produces the per-config evidence
lines.

Usage: python scripts/bench_configs.py --config painn_qm9 --steps 10
"""

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

from hydragnn_amd.data import Batch
from hydragnn_amd.models.create import create_model, resolve_precision
from hydragnn_amd.train import get_autocast_and_scaler, get_head_indices
from hydragnn_amd.utils.datasets.synthetic import lj_dataset


def qm9_shape_multihead(num_samples, seed=23):
    """QM9-shaped molecules with graph + node targets + Laplacian PE."""
    from hydragnn_amd.data import Data
    from hydragnn_amd.ops import radius_graph, scatter
    g = torch.Generator().manual_seed(seed)
    ds = []
    for _ in range(num_samples):
        n = 18
        pos = torch.randn(n, 3, generator=g) * 1.5
        ei = radius_graph(pos, 4.0, max_num_neighbors=20)
        u = torch.rand(n, 1, generator=g)
        nbr = scatter(u[ei[0]], ei[1], n, "mean")
        y = torch.cat([nbr.mean().view(1), nbr.view(-1)]).view(-1, 1)
        d = Data(x=u, pos=pos, edge_index=ei, y=y,
                 y_loc=torch.tensor([[0, 1, 1 + n]]))
        d.num_nodes = n
        ds.append(d)
    return ds


def _graph_only(d):
    """Keep the graph target of a `qm9_shape_multihead` sample."""
    d.y = d.y[:1]
    d.y_loc = torch.tensor([[0, 1]])
    return d


def oc20_shape(num_samples, seed=29, with_pe=False):
    """OC20-shaped surfaces: ~80 atoms, periodic slab."""
    from hydragnn_amd.preprocess import add_laplacian_pe
    ds = lj_dataset(num_samples=num_samples, num_atoms=80,
                    cell_size=12.0, radius=4.0, pbc=True, seed=seed)
    if with_pe:
        for d in ds:
            add_laplacian_pe(d, 3)
    return ds


def degree_histogram(dataset):
    """In-degree histogram of a dataset: the `pna_deg` of the PNA
    stacks."""
    hist = torch.zeros(1, dtype=torch.long)
    for d in dataset:
        deg = torch.bincount(d.edge_index[1], minlength=d.num_nodes)
        h = torch.bincount(deg)
        if h.numel() > hist.numel():
            h[:hist.numel()] += hist
            hist = h
        else:
            hist[:h.numel()] += h
    return hist.tolist()


def md17_shape(num_samples):
    from hydragnn_amd.utils.datasets.synthetic import md17_shape_dataset
    return md17_shape_dataset(num_samples=num_samples, radius=5.0,
                              max_neighbours=32, seed=37)


_NODE_HEAD = {"node": [{"type": "branch-0", "architecture": {
    "num_headlayers": 2, "dim_headlayers": [64, 64], "type": "mlp"}}]}
_GRAPH_HEAD = {"graph": [{"type": "branch-0", "architecture": {
    "num_sharedlayers": 1, "dim_sharedlayers": 64, "num_headlayers": 2,
    "dim_headlayers": [64, 64]}}]}

CONFIGS = {
    "pnaeq_mlip": dict(
        label="PNAEq MLIP energy+forces, MD17-shape, fp32",
        precision="fp32", local_batch=256, mlip=True,
        data=md17_shape,
        model=dict(mpnn_type="PNAEq", input_dim=1, hidden_dim=64,
                   output_dim=[1], output_type=["node"],
                   output_heads=_NODE_HEAD, task_weights=[1.0],
                   num_conv_layers=3, radius=5.0, num_radial=20,
                   max_neighbours=32, equivariance=True,
                   activation_function="silu",
                   enable_interatomic_potential=True, energy_weight=1.0,
                   energy_peratom_weight=0.0, force_weight=10.0)),
    "schnet_mlip": dict(
        label="SchNet MLIP energy+forces, MD17-shape, fp32",
        precision="fp32", local_batch=256, mlip=True,
        data=md17_shape,
        model=dict(mpnn_type="SchNet", input_dim=1, hidden_dim=64,
                   output_dim=[1], output_type=["node"],
                   output_heads=_NODE_HEAD, task_weights=[1.0],
                   num_conv_layers=3, radius=5.0, num_gaussians=50,
                   num_filters=64, max_neighbours=32,
                   activation_function="silu",
                   enable_interatomic_potential=True, energy_weight=1.0,
                   energy_peratom_weight=0.0, force_weight=10.0)),
    "pnaplus_qm9": dict(
        label="PNAPlus graph head, QM9-shape, bf16",
        precision="bf16", local_batch=256, mlip=False,
        data=lambda b: [_graph_only(d) for d in qm9_shape_multihead(b)],
        model=dict(mpnn_type="PNAPlus", input_dim=1, hidden_dim=64,
                   output_dim=[1], output_type=["graph"],
                   output_heads=_GRAPH_HEAD, task_weights=[1.0],
                   num_conv_layers=3, radius=4.0, num_radial=5,
                   envelope_exponent=5, max_neighbours=20,
                   activation_function="relu")),
    "painn_qm9": dict(
        label="PaiNN multi-head (graph+node) QM9-shape",
        precision="bf16", local_batch=256, mlip=False,
        data=lambda b: qm9_shape_multihead(b),
        model=dict(mpnn_type="PAINN", input_dim=1, hidden_dim=64,
                   output_dim=[1, 1], output_type=["graph", "node"],
                   output_heads={
                       "graph": [{"type": "branch-0", "architecture": {
                           "num_sharedlayers": 1, "dim_sharedlayers": 64,
                           "num_headlayers": 2,
                           "dim_headlayers": [64, 64]}}],
                       "node": [{"type": "branch-0", "architecture": {
                           "num_headlayers": 2,
                           "dim_headlayers": [64, 64],
                           "type": "mlp"}}]},
                   task_weights=[1.0, 1.0], num_conv_layers=3,
                   radius=4.0, num_radial=20, max_neighbours=20,
                   equivariance=True, activation_function="silu")),
    "egnn_gps": dict(
        label="EGNN + GPS global attention, OC20-shape, bf16",
        precision="bf16", local_batch=32, mlip=False,
        data=lambda b: oc20_shape(b, with_pe=True),
        model=dict(mpnn_type="EGNN", input_dim=1, hidden_dim=64,
                   output_dim=[1], output_type=["graph"],
                   output_heads={"graph": [{
                       "type": "branch-0", "architecture": {
                           "num_sharedlayers": 1, "dim_sharedlayers": 64,
                           "num_headlayers": 2,
                           "dim_headlayers": [64, 64]}}]},
                   task_weights=[1.0], num_conv_layers=3, radius=4.0,
                   max_neighbours=30, equivariance=True, pe_dim=3,
                   global_attn_engine="gps",
                   global_attn_type="multihead", global_attn_heads=4,
                   activation_function="silu")),
    "egnn_gps_performer": dict(
        label="EGNN + GPS Performer attention, OC20-shape, bf16",
        precision="bf16", local_batch=32, mlip=False,
        data=lambda b: oc20_shape(b, with_pe=True),
        model=dict(mpnn_type="EGNN", input_dim=1, hidden_dim=64,
                   output_dim=[1], output_type=["graph"],
                   output_heads={"graph": [{
                       "type": "branch-0", "architecture": {
                           "num_sharedlayers": 1, "dim_sharedlayers": 64,
                           "num_headlayers": 2,
                           "dim_headlayers": [64, 64]}}]},
                   task_weights=[1.0], num_conv_layers=3, radius=4.0,
                   max_neighbours=30, equivariance=True, pe_dim=3,
                   global_attn_engine="gps",
                   global_attn_type="performer", global_attn_heads=4,
                   activation_function="silu")),
    "dimenet_fp64": dict(
        label="DimeNet fp64 + grad checkpointing, periodic cells",
        precision="fp64", local_batch=4, mlip=False,
        # 1024-atom FeSi-shape cells at the 216-atom run's density
        # (12^3 for 216 -> 20.25^3 for 1024); BASELINE configs[4]
        data=lambda b: lj_dataset(num_samples=b, num_atoms=1024,
                                  cell_size=20.25, radius=3.0,
                                  pbc=True, seed=31,
                                  dtype=torch.float64),
        model=dict(mpnn_type="DimeNet", input_dim=1, hidden_dim=64,
                   output_dim=[1], output_type=["graph"],
                   output_heads={"graph": [{
                       "type": "branch-0", "architecture": {
                           "num_sharedlayers": 1, "dim_sharedlayers": 64,
                           "num_headlayers": 2,
                           "dim_headlayers": [64, 64]}}]},
                   task_weights=[1.0], num_conv_layers=2, radius=3.0,
                   num_radial=6, num_spherical=7, basis_emb_size=8,
                   int_emb_size=64, out_emb_size=128,
                   num_before_skip=1, num_after_skip=2,
                   max_neighbours=30, conv_checkpointing=True)),
}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", default="painn_qm9",
                        choices=sorted(CONFIGS))
    parser.add_argument("--steps", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--batch", type=int, default=None)
    args = parser.parse_args()
    cfg = CONFIGS[args.config]
    use_cuda = torch.cuda.is_available()
    device = "cuda:0" if use_cuda else "cpu"
    torch.manual_seed(7)

    batch_size = args.batch or cfg["local_batch"]
    prec, param_dtype, _ = resolve_precision(cfg["precision"])
    data = cfg["data"](batch_size)
    model_args = dict(cfg["model"])
    if model_args["mpnn_type"] in ("PNA", "PNAPlus", "PNAEq"):
        model_args["pna_deg"] = degree_histogram(data)
    model = create_model(use_gpu=False, loss_function_type="mse",
                         **model_args)
    model = model.to(device=device, dtype=param_dtype)
    batch = Batch.from_data_list(data).to(device)
    for key in list(batch.keys()):
        v = batch[key]
        if torch.is_tensor(v) and torch.is_floating_point(v):
            batch[key] = v.to(param_dtype)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    autocast, _ = get_autocast_and_scaler(cfg["precision"])
    head_index = None if cfg["mlip"] else get_head_indices(model, batch)

    def step():
        opt.zero_grad(set_to_none=True)
        if cfg["mlip"]:
            batch.pos.requires_grad_(True)
        with autocast:
            pred = model(batch)
            if cfg["mlip"]:
                loss, _ = model.energy_force_loss(pred, batch,
                                                  create_graph=True)
            else:
                loss, _ = model.loss(pred, batch.y, head_index)
        loss.backward()
        opt.step()
        return loss

    for _ in range(args.warmup):
        step()
    if use_cuda:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    if use_cuda:
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({
        "metric": f"graphs/sec training ({cfg['label']})",
        "value": batch_size * args.steps / dt,
        "unit": "graphs/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1000,
        "higher_is_better": True,
        "dtype": cfg["precision"],
        "data": "synthetic",
        "config": {"model": cfg["label"], "global_batch": batch_size},
    }))


if __name__ == "__main__":
    main()
