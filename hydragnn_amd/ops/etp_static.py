"""Static (compile-time) ETP tables: the Python view of
csrc/etp_static_tables.inc.

The static-table kernels (csrc/etp_static.hip) have their entry tables
compiled in, so a launch may use them only for a table that is EXACTLY
one of those: same dims, same entries in the same order, same fp32
coefficient bits.  This module parses the committed header — the very
text the compiler reads — and matches an `ETPTable`'s CPU copies against
it.  No GPU and no extension needed.
"""

from __future__ import annotations

import functools
import os
import re
from typing import List, NamedTuple, Tuple

import torch

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc",
                      "etp_static_tables.inc")


class StaticTable(NamedTuple):
    name: str
    id: int
    dims: Tuple[int, int, int, int]
    entries: torch.Tensor   # [N, 4] int64, columns a, b, g, o
    coefs: torch.Tensor     # [N] float32


def _int_array(body: str, name: str) -> List[int]:
    m = re.search(r"constexpr int %s\[N\] = \{([^}]*)\}" % name, body)
    return [int(v) for v in m.group(1).split(",") if v.strip()]


def parse_header(text: str) -> List[StaticTable]:
    """Tables of a generated header, in file order."""
    tables = []
    for m in re.finditer(r"struct (\w+) \{(.*?)\n\};", text, re.S):
        name, body = m.group(1), m.group(2)
        tid = int(re.search(r"constexpr int ID = (\d+);", body).group(1))
        dims = tuple(int(v) for v in re.search(
            r"DA = (\d+), DB = (\d+), DG = (\d+), DO = (\d+);",
            body).groups())
        n = int(re.search(r"constexpr int N = (\d+);", body).group(1))
        cols = [_int_array(body, c) for c in "ABGO"]
        cm = re.search(r"constexpr float COEF\[N\] = \{([^}]*)\}", body)
        coefs = [float.fromhex(v.strip().rstrip("f"))
                 for v in cm.group(1).split(",") if v.strip()]
        assert all(len(c) == n for c in cols) and len(coefs) == n, name
        # float.fromhex gives the double with the literal's value; the
        # literals are fp32 values, so this conversion is exact
        tables.append(StaticTable(
            name, tid, dims,
            torch.tensor(cols, dtype=torch.int64).t().contiguous()
            .reshape(n, 4),
            torch.tensor(coefs, dtype=torch.float64).to(torch.float32)))
    return tables


@functools.lru_cache(maxsize=None)
def static_tables() -> Tuple[StaticTable, ...]:
    with open(HEADER) as f:
        return tuple(parse_header(f.read()))


def lookup(entries: torch.Tensor, coefs: torch.Tensor, dims) -> int:
    """Id of the static table equal to (entries, coefs, dims) in dims,
    entry count, every index and every coefficient bit; -1 if none."""
    entries = entries.to(torch.int64).cpu()
    bits = coefs.to(torch.float32).cpu().contiguous().view(torch.int32)
    dims = tuple(int(d) for d in dims)
    for t in static_tables():
        if (t.dims == dims and tuple(t.entries.shape) == tuple(entries.shape)
                and torch.equal(t.entries, entries)
                and torch.equal(t.coefs.view(torch.int32), bits)):
            return t.id
    return -1
