"""GPU tests of the edge ladder: rows exactly on every bin and class edge, checked with exact sums.

Every kernel family takes its rows by an LDS budget or a work cap of csrc/mhs_shape.hpp (full call) or
csrc/mhs_valplan.hpp (values-only call and its backward).  tests/golden/shape_edges.json (printed from those
headers by tests/shape_edges.cpp; tests/test_shape_edges_host.py keeps the two equal) names, per rung, the last
row parameter that stays in a bin and the first that leaves it; the generators of tests/_util.py build, per
side, a matrix of EDGE_COPIES rows with exactly those parameters (checked on the CPU in the same host test).
All values are integers of +-{1, 2, 3}, so every sum is exact in any order: row_ptr, col_idx AND the values
must equal the oracle's (np.array_equal), and the call's census (Timing.num_bins / sym_bins, the plan's
info()["rows"]) must show the edge rows in the bin the headers name for that side, none in the other side's."""
import functools
import os

import numpy as np
import pytest
import torch

import mhspgemm
from oracle import oracle as orc
from _util import EDGE_COPIES, edge_case, edge_rows, edge_values, expand, filled, load_edges, ref_grad, upload

pytestmark = pytest.mark.gpu

EDGES = load_edges()
SIDES = ("last", "first")
NUMERIC = [("numeric", r["name"], s) for r in EDGES["numeric"] for s in SIDES]
DENSE = [("dense", r["name"], s) for r in EDGES["dense"] for s in SIDES]
SYMBOLIC = [("symbolic", r["name"], s) for r in EDGES["symbolic"] for s in SIDES]
VALUES = [("values", r["name"], s) for r in EDGES["values"] for s in SIDES]


def rung(group, name):
    return next(r for r in EDGES[group] if r["name"] == name)


@functools.lru_cache(maxsize=None)
def case(group, name, side):
    """One side of a rung: A, B (host CSR, read only) and the oracle's C, computed once for every test of it."""
    r = rung(group, name)
    At, Bt = edge_case("val", r[side]["params"]) if group == "values" else edge_case(r["family"], r[side]["params"], r["R"])
    A, B = mhspgemm.CSR(*At), mhspgemm.CSR(*Bt)
    C = orc.spgemm(A.ptr, A.col, A.val, B.ptr, B.col, B.val, B.N)
    return A, B, C


def exact_call(tool, A, B, C):
    """C = A*B on the device: pattern and values equal to the oracle's, bit for bit."""
    Cp, Ci, Cv = C
    A.H2D(tool.device)
    B.H2D(tool.device)
    D, t = mhspgemm.spgemm(tool, A, B)
    try:
        p, c, v = D.to_host()
    finally:
        D.release()
    assert np.array_equal(p, Cp), "row_ptr"
    assert np.array_equal(c, Ci), "col_idx"
    bad = np.nonzero(v != Cv)[0]
    assert len(bad) == 0, f"{len(bad)} values differ from the exact sums, first at {bad[:5]}: {v[bad[:5]]} != {Cv[bad[:5]]}"
    assert t.nnzC == Cp[-1] and t.flop == orc.flop(A.col, B.ptr)
    return t


# ------------------------------------------------------------------ the full call ---
@pytest.mark.parametrize("group,name,side", NUMERIC + SYMBOLIC)
def test_edge_full_call(tool, group, name, side):
    r = rung(group, name)
    A, B, C = case(group, name, side)
    t = exact_call(tool, A, B, C)
    if not r["count"]:  # both sides in one bin (ranked | wide, count | bitonic rank): the result only
        return
    key, bins, census = (("num_bin", EDGES["num_bins"], t.num_bins) if r["count"] == "num" else
                         ("sym_bin", EDGES["sym_bins"], t.sym_bins))
    here, there = r[side][key], r["first" if side == "last" else "last"][key]
    assert census[bins[here]] >= EDGE_COPIES, (here, census)  # (a group counts once, at its head)
    assert here == there or census[bins[there]] == 0, (there, census)
    if r["count"] == "num" and r["R"] > 1:
        grouped = t.num_bins[EDGES["num_bins"]["NUM_WSG"]] + t.num_bins[EDGES["num_bins"]["NUM_W16G"]]
        assert grouped == (EDGE_COPIES if r[side]["grouped"] else 0), t.num_bins


# ---------------------------------- the values-only call and its backward on a kept plan ---
@functools.lru_cache(maxsize=None)
def plan_reference(group, name, side):
    """Fresh integer values and cotangent, the oracle's C values for them and the bincount gradients."""
    A, B, (Cp, Ci, _) = case(group, name, side)
    av, bv, G = edge_values(A.nnz, 11), edge_values(B.nnz, 12), edge_values(len(Ci), 13)
    _, _, Cv = orc.spgemm(A.ptr, A.col, av, B.ptr, B.col, bv, B.N)
    pqs = expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)
    assert len(pqs[0]) == orc.flop(A.col, B.ptr)
    return av, bv, G, Cv, ref_grad(pqs, av, bv, G, A.nnz, B.nnz)


@pytest.mark.parametrize("group,name,side", NUMERIC + VALUES)
def test_edge_values_plan(tool, group, name, side):
    A, B, (Cp, Ci, _) = case(group, name, side)
    av, bv, G, Cv, (wA, wB) = plan_reference(group, name, side)
    A.H2D(tool.device)
    B.H2D(tool.device)
    Cd = mhspgemm.CSR(A.M, B.N, Cp, Ci, np.zeros(len(Ci)))
    Cd.H2D(tool.device)
    plan = mhspgemm.ValuesPlan(tool, A, B, Cd)
    try:
        info = plan.info()
        dav, dbv = upload(tool, av), upload(tool, bv)
        out, oA, oB = filled(tool, len(Ci)), filled(tool, A.nnz), filled(tool, B.nnz)
        plan.run(dav, dbv, out=out)
        dA, dB = plan.grad(upload(tool, G), dav, dbv, out_A=oA, out_B=oB)
        torch.cuda.synchronize()
        got, gA, gB = out.cpu().numpy(), dA.cpu().numpy(), dB.cpu().numpy()
    finally:
        plan.close()
    assert info["products"] == info["kept_products"] == orc.flop(A.col, B.ptr) and info["nnzC"] == len(Ci)
    assert np.array_equal(got, Cv), f"{np.count_nonzero(got != Cv)} values of the kept-pattern call differ from the exact sums"
    assert np.array_equal(gA, wA), f"dA: {np.count_nonzero(gA != wA)} entries differ from the exact sums"
    assert np.array_equal(gB, wB), f"dB: {np.count_nonzero(gB != wB)} entries differ from the exact sums"
    if group == "values":
        r = rung(group, name)
        here, there = r[side]["class_index"], r["first" if side == "last" else "last"]["class_index"]
        assert info["rows"][here] == EDGE_COPIES and info["rows"][there] == 0 and sum(info["rows"]) == A.M, info


# --------------------- the numeric rungs under the two switches no other test selects ---
# MHS_NO_MCACHE=1: symbolic keeps no tile masks, numeric walks the tiles itself -- the path rows take in
# production when their masks spilled out.  MHS_DENSE_SPAN=512: rows spanning at most 512 tiles take a dense
# accumulator; band rungs at the dense budgets (num_need_dense) join the ladder.  Results only: no bin asserts.
def switched_tool(tool, var, value):
    old = os.environ.get(var)
    os.environ[var] = value  # (read at context creation)
    try:
        return mhspgemm.Tool(tool.device)
    finally:
        if old is None:
            del os.environ[var]
        else:
            os.environ[var] = old


@pytest.fixture(scope="module")
def no_mcache_tool(tool):
    t2 = switched_tool(tool, "MHS_NO_MCACHE", "1")
    yield t2
    t2.close()


@pytest.fixture(scope="module")
def dense_span_tool(tool):
    t2 = switched_tool(tool, "MHS_DENSE_SPAN", str(EDGES["dense"][0]["dense_span"]))
    yield t2
    t2.close()


@pytest.mark.parametrize("group,name,side", NUMERIC)
def test_edge_numeric_without_mask_cache(no_mcache_tool, group, name, side):
    exact_call(no_mcache_tool, *case(group, name, side))


@pytest.mark.parametrize("group,name,side", NUMERIC + DENSE)
def test_edge_numeric_dense_span(dense_span_tool, group, name, side):
    exact_call(dense_span_tool, *case(group, name, side))


# ---------------------------------------------------------------------- row counts ---
# One below, at and one above the scan's block of SCAN_ITEMS rows (M = SCAN_ITEMS: the sentinel item M alone in
# the second block), four blocks, and around 2^19 rows, from where the scan takes 4096-row blocks and the probe
# and the symbolic fork start.
SCAN = EDGES["constants"]["SCAN_ITEMS"]


@pytest.mark.parametrize("M", [SCAN - 1, SCAN, SCAN + 1, 4 * SCAN, (1 << 19) - 1, 1 << 19, (1 << 19) + 1])
def test_edge_row_count(tool, M):
    At, Bt = edge_rows(M)
    A, B = mhspgemm.CSR(*At), mhspgemm.CSR(*Bt)
    C = orc.spgemm(A.ptr, A.col, A.val, B.ptr, B.col, B.val, B.N)
    exact_call(tool, A, B, C)
    A.d_release_csr()
    B.d_release_csr()
