"""GPU tests that hold every FP64 value path to its rounding bound (include/mhspgemm.h, tests/_util.py).

An FP64 output entry summed from m kept products, S the sum of their absolute values, lies within
gamma_m * S of the exact sum (u = 2^-53), whatever the order and whether the products are fused; the tests
assert 1.01 * m * 2^-53 * S against sums taken in long double (assert_f64_bound).  A float temporary, a value
staged through a 4-byte slot or a cotangent read as float in a double instantiation is 2^29 outside it.

The full call (mhs_spgemm) runs here on every numeric path a context can be switched to, each case with a
census assert -- a case whose path did not run proves nothing -- and with two value families: the signed
narrow one of new_values and wide_values (full mantissas over 41 binades).  The values plans (forward, dA, dB;
plain, masked product / dot / auto) run with wide values; tests/test_gpu_values.py, test_gpu_masked.py and
test_gpu_values_grad.py hold them to the same bound with the narrow family."""
import functools
import os

import numpy as np
import pytest
import torch

import mhspgemm
from mhspgemm import _lib as L
from mhspgemm import synth
from oracle import oracle as orc
from _util import (assert_f64_bound, bin_zoo, csr_of, device_csr, edge_val, exact_forward, exact_grad, expand, filled,
                   group_zoo, load_edges, near_zoo, new_values, random_csr, run_zoo, tiny_zoo, upload, wide_values)
from test_gpu_masked import rect_pair, thinned_mask_with_strangers
from test_gpu_parity import _perturbed_fem
from test_gpu_values_grad import reduction_case, triangle_case

pytestmark = pytest.mark.gpu

TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL, DOT = 1, 2, 3, 4, 5, 6, 7
NUM_WSG = 6  # mhs_shape.hpp's NumBin
FAMILIES = ("narrow", "wide")


def values(family, n, seed):
    return new_values(n, seed, signed=True) if family == "narrow" else wide_values(n, seed)


# ------------------------------------------------------------------ the full call ---
@functools.lru_cache(maxsize=None)
def pattern(name):
    """The operand patterns of a case, (A, B) as tuples (M, N, ptr, col); B is None for A*A."""
    if name == "fem_5_5_13":
        F = synth.fem_grid(5, 5, 13, 3, seed=5)
    elif name == "fem_5_4_9":
        F = synth.fem_grid(5, 4, 9, dof=3)
    elif name == "perturbed_fem":
        F = _perturbed_fem(7, 6, 24, 0.03, seed=31)
    else:
        At, Bt = {"bin_zoo": bin_zoo, "tiny_zoo": lambda: tiny_zoo(7), "run_zoo": lambda: run_zoo(5),
                  "group_zoo": lambda: group_zoo(3), "near_zoo": near_zoo}[name]()
        return At[:4], Bt[:4]
    return (F.M, F.N, F.ptr, F.col), None


@functools.lru_cache(maxsize=None)
def reference(name, family):
    """The case's operands with the family's values on its patterns, the oracle's pattern of C and the exact
    (ref_ld, m, S) -- computed once for every context the case runs on, and read only."""
    At, Bt = pattern(name)
    A = mhspgemm.CSR(*At, values(family, len(At[3]), 17))
    B = A if Bt is None else mhspgemm.CSR(*Bt, values(family, len(Bt[3]), 1017))
    Cp, Ci, _ = orc.spgemm(A.ptr, A.col, A.val, B.ptr, B.col, B.val, B.N)
    exact = exact_forward(A, B, Cp, Ci, A.val, B.val)
    assert exact[1].min(initial=1) >= 1 and exact[1].sum() == orc.flop(A.col, B.ptr)
    return A, B, Cp, Ci, exact


def judged_call(t, name, family, what):
    A, B, Cp, Ci, exact = reference(name, family)
    C, tm = mhspgemm.spgemm(t, A, B)
    try:
        p, c, v = C.to_host()
    finally:
        C.release()
    assert np.array_equal(p, Cp), "row_ptr must be bit-exact"
    assert np.array_equal(c, Ci), "col_idx must be bit-exact"
    assert_f64_bound(v, *exact, f"full call, {what}, {family} values")
    assert tm.nnzC == Cp[-1] and tm.flop == orc.flop(A.col, B.ptr)
    return tm


def bin_zoo_census(t, tm, M):
    assert all(tm.sym_bins[i] > 0 for i in (0, 1, 2, 3, 4, 11)), tm.sym_bins
    assert all(tm.num_bins[i] > 0 for i in (0, 3, 4, 5, 12, 13, 14, 15)), tm.num_bins


def tiny_census(t, tm, M):
    assert all(tm.num_bins[i] > 0 for i in range(8, 12)), tm.num_bins


def nft_census(t, tm, M):
    assert t.stat("nft") > 0, t.stat("nft")


def run_zoo_census(t, tm, M):
    assert tm.num_bins[1] + tm.num_bins[14] > 0 and tm.num_bins[3] > 0, tm.num_bins


def group_zoo_census(t, tm, M):
    assert tm.num_bins[6] > 0, tm.num_bins


def near_zoo_census(t, tm, M):
    assert tm.num_bins[6] + tm.num_bins[7] > M // 10, tm.num_bins


def near_stat_census(t, tm, M):
    assert t.stat("near") == 1, t.stat("near")


def capped_grid_census(t, tm, M):
    assert tm.num_bins[NUM_WSG] == 325, tm.num_bins


def chunked_census(t, tm, M):
    assert t.chunked_calls() == 1, t.chunked_calls()


def no_census(t, tm, M):
    pass


NFT_ENV = {"MHS_NFT_OTHER_PCT": "100"}
DENSE_ENV = {"MHS_DENSE_SPAN": str(load_edges()["dense"][0]["dense_span"])}
CHUNK_ENV = {"MHS_MC_LIST": "2000", "MHS_SPILL_CAP": "65536"}  # (tests/test_gpu_group_walk.py::test_row_chunked_launches)

# id: (operands, environment read at context creation, options set on the context, census)
FULL_CALLS = {
    "bin_zoo": ("bin_zoo", {}, {}, bin_zoo_census),
    "tiny_zoo": ("tiny_zoo", {}, {}, tiny_census),
    "run_zoo": ("run_zoo", {}, {}, run_zoo_census),
    "group_zoo": ("group_zoo", {}, {}, group_zoo_census),
    "near_zoo": ("near_zoo", {}, {}, near_zoo_census),
    "perturbed_fem_near_union": ("perturbed_fem", {}, {}, near_stat_census),
    "tiny_zoo_numeric_first": ("tiny_zoo", NFT_ENV, {L.MHS_OPT_TINY_FIRST_ROWS: 0}, nft_census),
    "tiny_zoo_numeric_first_no_slots": ("tiny_zoo", {**NFT_ENV, "MHS_NFT_NO_SLOTS": "1"}, {L.MHS_OPT_TINY_FIRST_ROWS: 0},
                                        tiny_census),
    "bin_zoo_no_mask_cache": ("bin_zoo", {"MHS_NO_MCACHE": "1"}, {}, no_census),
    "bin_zoo_dense_span": ("bin_zoo", DENSE_ENV, {}, no_census),
    "fem_dense_span": ("fem_5_4_9", DENSE_ENV, {}, no_census),
    "bin_zoo_spill_lists_full": ("bin_zoo", {"MHS_MC_LIST": "16", "MHS_SPILL_CAP": "300"}, {}, no_census),
    "fem_capped_group_grid": ("fem_5_5_13", {}, {L.MHS_OPT_GROUP_GRID: 8}, capped_grid_census),
    "fem_row_chunked": ("fem_5_5_13", CHUNK_ENV, {L.MHS_OPT_GROUP_GRID: 8, L.MHS_OPT_MEM_BUDGET: 20}, chunked_census),
}


def fresh_tool(tool, env, options):
    """A context of its own for one case: the environment switches are read at its creation."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        t2 = mhspgemm.Tool(tool.device)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    for opt, value in options.items():
        t2.set_option(opt, value)
    return t2


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", list(FULL_CALLS))
def test_f64_full_call(tool, case, family):
    name, env, options, census = FULL_CALLS[case]
    A, B = reference(name, family)[:2]
    A.H2D(tool.device)
    if B is not A:
        B.H2D(tool.device)
    t2 = fresh_tool(tool, env, options)
    try:
        tm = judged_call(t2, name, family, case)
        census(t2, tm, A.M)
    finally:
        t2.close()
        A.d_release_csr()
        B.d_release_csr()


@pytest.mark.parametrize("family", FAMILIES)
def test_f64_full_call_speculated(tool, family):
    """The same call twice on the same device arrays: the second queues the first's numeric plan behind the scan
    (a hit), and it is the second call's C that is judged."""
    A = reference("fem_5_5_13", family)[0]
    A.H2D(tool.device)
    t2 = fresh_tool(tool, {}, {})
    try:
        C, _ = mhspgemm.spgemm(t2, A, A)
        C.release()
        assert t2.stat("spec") == 0
        judged_call(t2, "fem_5_5_13", family, "speculated second call")
        assert t2.stat("spec") == 1 and t2.stat("spec_miss") == 0, (t2.stat("spec"), t2.stat("spec_miss"))
    finally:
        t2.close()
        A.d_release_csr()


# ------------------------------------------- the values plans: forward, dA and dB ---
def pattern_of(A, B):
    Cp, Ci, _ = orc.spgemm(A.ptr, A.col, np.ones(A.nnz), B.ptr, B.col, np.ones(B.nnz), B.N)
    return Cp, Ci


def plan_check(tool, A, B, Cp, Ci, what, masked=False, form="auto", seed=1, between=None):
    """A plan of A*B on the pattern (Cp, Ci) with wide values and a wide cotangent: one forward and one backward
    call into NaN-filled buffers, all three outputs against the bound.  Returns info().  between: called after
    the forward (other work on the plan's context); the forward then runs again, into NaNs again, and is held
    to the bound like the first (the header promises no order of the forward's sums, so not to its bits)."""
    A.H2D(tool.device)
    if B is not A:
        B.H2D(tool.device)
    C = device_csr(tool, A.M, B.N, Cp, Ci)
    av, bv, G = wide_values(A.nnz, seed), wide_values(B.nnz, seed + 1000), wide_values(len(Ci), seed + 2000)
    plan = mhspgemm.ValuesPlan(tool, A, B, C, masked=masked, form=form)
    try:
        info = plan.info()
        dAv, dBv = upload(tool, av), upload(tool, bv)
        oC, oA, oB = filled(tool, len(Ci)), filled(tool, A.nnz), filled(tool, B.nnz)
        plan.run(dAv, dBv, out=oC)
        torch.cuda.synchronize()
        gC = [oC.cpu().numpy()]
        if between is not None:
            between()
            oC.fill_(float("nan"))
            plan.run(dAv, dBv, out=oC)
            torch.cuda.synchronize()
            gC.append(oC.cpu().numpy())
            assert plan.info() == info, f"{what}: the plan after other work on its context"
        plan.grad(upload(tool, G), dAv, dBv, out_A=oA, out_B=oB)
        torch.cuda.synchronize()
        gA, gB = oA.cpu().numpy(), oB.cpu().numpy()
    finally:
        plan.close()
    pqs = expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)
    assert len(pqs[0]) == info["kept_products"]
    exA, exB = exact_grad(pqs, av, bv, G, A.nnz, B.nnz)
    exC = exact_forward(A, B, Cp, Ci, av, bv)
    for k, g in enumerate(gC):
        assert_f64_bound(g, *exC, f"{what}, C, wide values" + ", after other work on the context" * k)
    assert_f64_bound(gA, *exA, f"{what}, dA, wide values")
    assert_f64_bound(gB, *exB, f"{what}, dB, wide values")
    return info


@functools.lru_cache(maxsize=None)
def plain_case(name):
    if name == "global_rows":  # two rows of 19,969 entries over a wide span: past a workgroup's LDS either way
        At, Bt = edge_val(19969, 1_000_000, 20000, copies=2)
    else:
        At, Bt = bin_zoo() if name == "bin_zoo" else tiny_zoo(7)
    A, B = csr_of(At), csr_of(Bt)
    return A, B, pattern_of(A, B)


_PLAIN_INFO = {}


def plain_info(tool, name):
    if name not in _PLAIN_INFO:
        A, B, (Cp, Ci) = plain_case(name)
        _PLAIN_INFO[name] = plan_check(tool, A, B, Cp, Ci, f"values plan, {name}", seed=3)
    return _PLAIN_INFO[name]


@pytest.mark.parametrize("name", ["bin_zoo", "tiny_zoo", "global_rows"])
def test_f64_plain_plan(tool, name):
    info = plain_info(tool, name)
    if name == "tiny_zoo":
        assert info["rows"][TEAM] > 0.5 * sum(info["rows"])
    if name == "global_rows":
        assert info["rows"][GLOBAL] == 2


def test_f64_plain_plans_every_class_has_rows(tool):
    rows = np.sum([plain_info(tool, n)["rows"] for n in ("bin_zoo", "tiny_zoo", "global_rows")], axis=0)
    for cls in (TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL):
        assert rows[cls] > 0, f"class {cls} has no rows"
    assert rows[DOT] == 0


@functools.lru_cache(maxsize=None)
def masked_case(name):
    if name == "triangle":
        Lt = triangle_case()
        return Lt, Lt, Lt.ptr, Lt.col
    (p, c, v), (Bp, Bc, Bv), (Cp, Ci) = rect_pair()
    A, B = mhspgemm.CSR(1500, 1000, p, c, v), mhspgemm.CSR(1000, 20_000, Bp, Bc, Bv)
    Mp, Mc, strangers = thinned_mask_with_strangers(Cp, Ci, B.N)
    assert strangers > 1000
    return A, B, Mp, Mc


@pytest.mark.parametrize("form", ["product", "dot", "auto"])
@pytest.mark.parametrize("case", ["triangle", "thinned_with_strangers"])
def test_f64_masked_plan(tool, case, form):
    A, B, Mp, Mc = masked_case(case)
    info = plan_check(tool, A, B, Mp, Mc, f"masked plan, {form} form, {case}", masked=True, form=form, seed=9)
    assert 0 < info["kept_products"] < info["products"], "the case needs products outside the mask"
    if form == "dot":
        assert info["rows"][DOT] > 0, info
    if form == "product":
        assert info["rows"][DOT] == 0, info
    _, _, s = expand(A.ptr, A.col, B.ptr, B.col, Mp, Mc, B.N)
    assert np.count_nonzero(np.bincount(s, minlength=len(Mc)) == 0) > 0, "mask entries no product reaches (m = 0)"


def test_f64_group_reduction_of_dA(tool):
    A, B, (Cp, Ci) = reduction_case()
    info = plan_check(tool, A, B, Cp, Ci, "values plan, reduction case", seed=5)
    rows = info["rows"]
    assert rows[WAVE_DIRECT] == 2 and rows[WAVE_SEARCH] == 2 and rows[BLOCK_DIRECT] == 1 and rows[BLOCK_SEARCH] == 1, info
    assert rows[TEAM] == 10, info


def test_f64_superset_pattern(tool):
    """C's pattern a strict superset of the product's: every 7th entry of A removed after the pattern was taken,
    so entries with m = 0 sit among reached ones in the rows of every class the pair has."""
    p, c, v = random_csr(600, 500, 7, 5)
    Bp, Bc, Bv = random_csr(500, 6000, 10, 6)
    B = mhspgemm.CSR(500, 6000, Bp, Bc, Bv)
    Cp, Ci = pattern_of(mhspgemm.CSR(600, 500, p, c, v), B)
    keep = np.ones(len(c), bool)
    keep[::7] = False
    rows = np.repeat(np.arange(600), np.diff(p))
    p2 = np.zeros(601, np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=600), out=p2[1:])
    A2 = mhspgemm.CSR(600, 500, p2.astype(np.int32), c[keep], v[keep])
    _, _, s = expand(A2.ptr, A2.col, B.ptr, B.col, Cp, Ci, B.N)
    m = np.bincount(s, minlength=len(Ci))
    assert 0 < np.count_nonzero(m == 0) < len(Ci) // 2
    info = plan_check(tool, A2, B, Cp, Ci, "values plan, superset pattern", seed=7)
    assert info["kept_products"] == info["products"] == len(s)
