"""Compile-time ETP tables (csrc/etp_static_tables.inc): the committed
header is what the generator writes, holds exactly the tables of the
flagship's edge tensor products, and the lookup that guards the static
kernels matches nothing else.  CPU only."""

import os
import subprocess
import sys

import torch

from hydragnn_amd.models.mace.blocks import EdgeTensorProduct
from hydragnn_amd.ops.etp import ETPTable
from hydragnn_amd.ops.etp_static import (
    HEADER, lookup, parse_header, static_tables)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATOR = os.path.join(REPO, "scripts", "gen_etp_static_tables.py")
TRIPLES = [(0, 2, 1), (1, 2, 1)]


def _bits(coefs):
    return coefs.to(torch.float32).contiguous().view(torch.int32)


def _random_table(seed=0, da=4, db=9, dg=6, do=16, n_ent=40):
    # same table as tests/test_gpu_etp.py
    g = torch.Generator().manual_seed(seed)
    ents = torch.stack([
        torch.randint(0, da, (n_ent,), generator=g),
        torch.randint(0, db, (n_ent,), generator=g),
        torch.randint(0, dg, (n_ent,), generator=g),
        torch.randint(0, do, (n_ent,), generator=g),
    ], dim=1)
    coefs = torch.randn(n_ent, generator=g)
    return ETPTable(ents, coefs, (da, db, dg, do))


def test_generator_reproduces_committed_header(tmp_path):
    out = tmp_path / "tables.inc"
    subprocess.run([sys.executable, GENERATOR, "--out", str(out)],
                   check=True, cwd=REPO)
    with open(HEADER, "rb") as f:
        committed = f.read()
    assert out.read_bytes() == committed


def test_header_holds_the_edge_tensor_product_tables():
    with open(HEADER) as f:
        parsed = parse_header(f.read())
    assert len(parsed) == len(TRIPLES)
    for tid, (triple, st) in enumerate(zip(TRIPLES, parsed)):
        table = EdgeTensorProduct(*triple).etp_table
        assert st.id == tid
        assert st.name == "ETPStatic_%d_%d_%d" % triple
        assert st.dims == table.dims
        assert st.entries.shape == table.entries.shape
        assert torch.equal(st.entries, table.entries)
        assert table.coefs.dtype == torch.float32
        assert torch.equal(_bits(st.coefs), _bits(table.coefs))
    assert [t.id for t in static_tables()] == list(range(len(TRIPLES)))


def test_lookup_finds_both_tables():
    for tid, triple in enumerate(TRIPLES):
        table = EdgeTensorProduct(*triple).etp_table
        assert lookup(table.entries, table.coefs, table.dims) == tid
        assert table.static_id == tid
        assert table.static_id == tid  # cached on the object


def test_lookup_rejects_everything_else():
    assert _random_table().static_id == -1

    tp121 = EdgeTensorProduct(1, 2, 1).etp_table
    # one coefficient moved by one fp32 ulp
    coefs = tp121.coefs.clone()
    coefs[10] = torch.nextafter(coefs[10], torch.tensor(2.0))
    assert (_bits(coefs) != _bits(tp121.coefs)).sum() == 1
    assert ETPTable(tp121.entries, coefs, tp121.dims).static_id == -1

    # two entries swapped (with their coefficients: the same form, but
    # not the same table)
    order = list(range(tp121.entries.shape[0]))
    order[3], order[12] = order[12], order[3]
    swapped = ETPTable(tp121.entries[order], tp121.coefs[order],
                       tp121.dims)
    assert not torch.equal(swapped.entries, tp121.entries)
    assert swapped.static_id == -1

    # wrong dims, and a role permutation, do their own lookup
    assert lookup(tp121.entries, tp121.coefs, (4, 9, 5, 5)) == -1
    assert tp121.perm("obga").static_id == -1
