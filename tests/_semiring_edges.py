"""The cases of the semiring class-edge ladder (test infrastructure): tests/test_gpu_semiring_edges.py runs them on the
device, tests/test_semiring_edges_host.py holds the conditions on their inputs without one.  Importing this creates no
context.

A case is a rung, a side, a value type and a semiring.  The rungs are the edges of csrc/mhs_valplan.hpp's val_class
that the plus-times ladders already hold: four that move with the sum bytes (the tables of tests/test_gpu_smooth.py at
8 sum bytes for float64 and of tests/test_gpu_values_f32.py for float32, imported) and the two count edges of the team
class (tests/test_gpu_values_batched.py's TEAM_EDGES), each "at" the cap and one "above" it.  Every case is EDGE_COPIES
rows of _util.edge_val(n, span, products): n - 1 columns from the row's first one and a last entry at column
first + span - 1 that a single product reaches -- the last slot of a searched slice, the last column of a direct span,
the first row that leaves a class.

The values are the exact regime's of tests/test_gpu_subgrad.py (exact_values at SEED): integers in [-3, 3] and a few
infinities.  conditions() asserts on the numpy reference alone that such a case can say something: no NaN product,
entries with ties, a winner in the last entry of most rows, and entries that are reached but hold the identity."""
import functools

import numpy as np

from oracle import oracle as orc
from _util import EDGE_COPIES, csr_of, edge_val, expand
import test_gpu_semiring as fwd
import test_gpu_subgrad as sub
from test_gpu_smooth import EDGES as EDGES_BY_SUM_BYTES
from test_gpu_values_batched import TEAM_EDGES, val_class
from test_gpu_values_f32 import BYTE_EDGES, EDGES as EDGES_F32

SEMIRINGS = fwd.SEMIRINGS
DTYPES = ("float64", "float32")
SUM_BYTES = {"float64": 8, "float32": 4}
RUNGS = tuple(BYTE_EDGES) + tuple(TEAM_EDGES)
SIDES = ("at", "above")
SEED = 300
assert RUNGS == ("wave_direct_span", "wave_search_n", "block_direct_span", "block_search_n", "team_n", "team_products")
assert set(BYTE_EDGES) == set(EDGES_BY_SUM_BYTES[8])


def rung(name, side, dtype):
    """(n, span, products, class) of one side (0: at, 1: above) of a rung under a plan of `dtype`."""
    if name in TEAM_EDGES:
        edge = TEAM_EDGES[name]
    else:
        edge = EDGES_BY_SUM_BYTES[8][name] if dtype == "float64" else EDGES_F32[name]
    n, span, products = edge[side]
    return n, span, products, edge[2][side]


@functools.lru_cache(maxsize=None)
def pattern(n, span, products):
    """(A, B, Cp, Ci, kept products) of edge_val(n, span, products), built once for every type and semiring."""
    A, B = (csr_of(t) for t in edge_val(n, span, products))
    Cp, Ci, _ = orc.spgemm(A.ptr, A.col, np.ones(A.nnz), B.ptr, B.col, np.ones(B.nnz), B.N)
    return A, B, Cp, Ci, expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)


def exact_case(sr, n, span, products, dtype):
    """The exact regime of a case on the host: (av, bv, Cval, win, T) -- the values, the sequential forward in `dtype`,
    the winning products and the winners per entry."""
    A, B, Cp, Ci, pqs = pattern(n, span, products)
    av, bv = sub.exact_values(sr, A, B, SEED)
    c = fwd.reference(sr, pqs, av, bv, len(Ci), dtype)
    win, T = sub.winners(sr, pqs, av, bv, c, dtype)
    return av, bv, c, win, T


def conditions(name, sr, n, span, products, dtype, exact):
    """What a case's exact-regime values must be for its comparisons to mean something; numpy only.  Returns the
    counts (entries with ties, rows whose last entry has a winner, reached entries without a winner)."""
    A, B, Cp, Ci, (p, q, s) = pattern(n, span, products)
    av, bv, c, win, T = exact
    assert A.M == EDGE_COPIES and np.all(np.diff(Cp) == n), "every row has the rung's n entries"
    assert np.all(Ci[Cp[1:] - 1].astype(np.int64) - Ci[Cp[:-1]] + 1 == span), "... over the rung's span"
    assert np.all(np.diff(B.ptr)[A.col].reshape(A.M, -1).sum(1) == products), "... from the rung's products"
    a, b = av.astype(fwd.NP[dtype])[p], bv.astype(fwd.NP[dtype])[q]
    with np.errstate(invalid="ignore"):
        prod = np.minimum(a, b) if sr == "max_min" else a + b
    assert not np.isnan(prod).any(), "no product is NaN: the forward is bit-identical everywhere"
    m = np.bincount(s, minlength=len(Ci))
    assert m.min() >= 1, "every entry is reached"
    last = Cp[1:].astype(np.int64) - 1
    assert np.all(m[last] == 1), "the row's last entry, at column first + span - 1, is a single product"
    ties, last_won, no_winner = int((T >= 2).sum()), int((T[last] >= 1).sum()), int((T == 0).sum())
    assert ties >= 1, "the case needs an entry with ties"
    assert last_won >= 6, f"the last entry has a winner in {last_won} of {A.M} rows: the slot every guard is about"
    assert np.all(c[T == 0] == fwd.IDENTITY[sr]), "a reached entry without a winner holds the identity"
    if name != "team_products":
        assert no_winner >= 1, "the case needs a reached entry without a winner"
    return ties, last_won, no_winner
