"""GPU tests that hold every value path to IEEE propagation of Inf, NaN and stored zeros (include/mhspgemm.h,
tests/_util.py: the non-finite contract).

The oracle forms every kept product and nothing else.  A kernel breaks that silently by adding an explicit 0 * b
for padding, by skipping a stored zero or a product it takes to be zero, or by letting a lane, a row, a value set
or a dropped masked product reach a neighbour's sum: on finite data all of it is invisible, with one Inf in the
data it puts a NaN where the oracle has a number or a number where it has a NaN.  The contract is free of any
summation order: an entry is NaN if one of its kept products is NaN (0 * Inf, anything times NaN) or products of
both infinities occur, +Inf or -Inf if only that infinity occurs, and otherwise finite within 1.01 m u S of its
products' sum (u = 2^-53 against long-double sums; FP32 plans: u = 2^-24 against double sums on float32-rounded
inputs) and exactly 0.0 where m = 0.  tests/test_nonfinite_host.py holds the checker to the oracle and to ref_grad
on the inputs used here.  Finite magnitudes are wide_values' (FP32: [0.1, 1)): no finite partial sum overflows.

The one carve-out is the header's, on the backward: a zero cotangent times a non-finite value may give 0 or NaN
(test_carve_out_zero_cotangent); nothing here is stricter than that and nothing else is looser.  No tolerance
is measured.

The full call runs every entry of tests/test_gpu_f64_bound.py's FULL_CALLS (and perturbed_fem row-chunked) with
its census; the values plans run widths 1, 2 and 4 in both types through the batched entry points, which serve
every width."""
import functools

import numpy as np
import pytest
import torch

import mhspgemm
from mhspgemm import _lib as L
from oracle import oracle as orc
from _util import (FINITE, IS_NAN, NEG_INF, POS_INF, U32, U64, assert_nonfinite_reference, bin_zoo, classes_of, csr_of,
                   edge_val, edge_values, expand, inject_nonfinite, new_values, nonfinite_reference, product_classes,
                   tiny_zoo, wide_values)
import test_gpu_values_batched as fb
from test_gpu_f64_bound import (CHUNK_ENV, FULL_CALLS, chunked_census, fresh_tool, judged_call, masked_case, pattern,
                                reference)
from test_gpu_values_batched import BYTE_EDGES, PLANS, TEAM_EDGES, TYPES, make_plan, nans, pattern_of, up
from test_gpu_values_grad_batched import grad_reference

pytestmark = pytest.mark.gpu

TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL, DOT = 1, 2, 3, 4, 5, 6, 7
PRODUCT_CLASSES = (TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL)


def grouped(tm):
    return tm.num_bins[6] + tm.num_bins[7]


# ------------------------------------------------------------------ the full call ---
CALLS = dict(FULL_CALLS)
CALLS["perturbed_fem_row_chunked"] = ("perturbed_fem", CHUNK_ENV, {L.MHS_OPT_GROUP_GRID: 8, L.MHS_OPT_MEM_BUDGET: 20},
                                      chunked_census)
# near groups add explicit 0 * b products, so a call whose B holds a non-finite value dissolves them (near_groups'
# check of B's values, k_scan): these censuses change by design, and hold again on a finite call of the context
DISSOLVED = {("near_zoo", "B"), ("near_zoo", "both"), ("perturbed_fem_near_union", "one")}
SQUARE = {"fem_5_5_13", "fem_5_4_9", "perturbed_fem"}  # A*A: the one injection (injected() holds this to pattern())
FULL_CASES = [(case, inject) for case, (name, _, _, _) in CALLS.items()
              for inject in (("one",) if name in SQUARE else ("A", "B", "both"))]


@functools.lru_cache(maxsize=None)
def products(name):
    """The pattern of the case's C and its kept products (every product: the pattern is the product's own)."""
    A, B, Cp, Ci, _ = reference(name, "wide")
    return Cp, Ci, expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)


def contract_of(name, av, bv):
    Cp, Ci, (p, q, s) = products(name)
    return nonfinite_reference(s, av[p], bv[q], len(Ci), U64)


@functools.lru_cache(maxsize=None)
def injected(name, inject):
    """The case's operands with wide values (seeds 17 and 1017, as the finite tests) and non-finite values and
    stored zeros injected into A (seed 5), into B (seed 6) or into both, and the contract's reference."""
    A0, B0 = reference(name, "wide")[:2]
    assert (pattern(name)[1] is None) == (name in SQUARE) == (B0 is A0)
    A = mhspgemm.CSR(A0.M, A0.N, A0.ptr, A0.col, inject_nonfinite(A0.val, 5) if inject != "B" else A0.val)
    if B0 is A0:
        assert inject == "one"
        B = A
    else:
        B = mhspgemm.CSR(B0.M, B0.N, B0.ptr, B0.col, inject_nonfinite(B0.val, 6) if inject != "A" else B0.val)
    R = contract_of(name, A.val, B.val)
    assert np.count_nonzero(R[0] == FINITE) > len(R[0]) // 2 and all((R[0] == c).any() for c in (POS_INF, NEG_INF, IS_NAN))
    return A, B, R


def judged_nonfinite_call(t, A, B, name, R, what):
    Cp, Ci, _ = products(name)
    C, tm = mhspgemm.spgemm(t, A, B)
    try:
        p, c, v = C.to_host()
    finally:
        C.release()
    assert np.array_equal(p, Cp), "row_ptr must be bit-exact"
    assert np.array_equal(c, Ci), "col_idx must be bit-exact"
    assert_nonfinite_reference(v, R, f"full call, {what}")
    assert tm.nnzC == Cp[-1] and tm.flop == orc.flop(A.col, B.ptr)
    return tm


@pytest.mark.parametrize("case,inject", FULL_CASES, ids=[f"{c}-{i}" for c, i in FULL_CASES])
def test_nonfinite_full_call(tool, case, inject):
    name, env, options, census = CALLS[case]
    A, B, R = injected(name, inject)
    A.H2D(tool.device)
    if B is not A:
        B.H2D(tool.device)
    t2 = fresh_tool(tool, env, options)
    F = None
    try:
        tm = judged_nonfinite_call(t2, A, B, name, R, f"{case}, non-finite values in {inject}")
        print(f"{case}-{inject}: sym_bins {list(tm.sym_bins)} num_bins {list(tm.num_bins)}")
        if (case, inject) in DISSOLVED:
            assert grouped(tm) < A.M // 30, tm.num_bins  # (test_near_row_groups' MHS_NO_NEAR leg)
            F = reference(name, "wide")[:2]
            F[0].H2D(tool.device)
            if F[1] is not F[0]:
                F[1].H2D(tool.device)
            tm = judged_call(t2, name, "wide", f"{case}, a finite call after the non-finite one")
        census(t2, tm, A.M)
    finally:
        t2.close()
        for X in (A, B) + tuple(F or ()):
            X.d_release_csr()


def set_values_in_place(A, v):
    """New values in A's device array (the same address, as a caller's time step writes them)."""
    assert len(v) == A.d_val.numel()
    A.d_val.copy_(torch.from_numpy(np.ascontiguousarray(v, np.float64)))
    torch.cuda.synchronize()


def positions(nnz):
    return [0, 1, 63, 64, nnz // 3, nnz // 2, nnz - 65, nnz - 2, nnz - 1]


@functools.lru_cache(maxsize=None)
def one_bad_value(k):
    """perturbed_fem's wide values with exactly one non-finite value, the k-th of positions(): +Inf, -Inf, NaN in
    turn -- the first and the last slices, lanes and unrolled steps of near_groups' finiteness check and its tail."""
    A, _, Cp, Ci, exact = reference("perturbed_fem", "wide")
    v = A.val.copy()
    pos = positions(len(v))[k]
    v[pos] = (np.inf, -np.inf, np.nan)[k % 3]
    assert np.count_nonzero(~np.isfinite(v)) == 1
    p, q, s = products("perturbed_fem")[2]
    want = product_classes(s, v[p], v[q], len(Ci))
    touched = np.zeros(len(Ci), bool)
    touched[s[(p == pos) | (q == pos)]] = True
    # no value is zero, so every entry the bad value reaches is non-finite, and the others keep the products, and
    # with them the long-double sums, of the finite reference
    assert touched.any() and np.array_equal(touched, want != FINITE)
    return v, (want,) + tuple(x[~touched] for x in exact) + (U64,)


@pytest.mark.parametrize("fork", [False, True], ids=["default", "sym_fork"])
def test_nonfinite_one_bad_value_by_position(tool, fork):
    A = A0 = reference("perturbed_fem", "wide")[0]  # (judged_call runs the reference's own operand)
    A.H2D(tool.device)
    t2 = fresh_tool(tool, {"MHS_SYM_FORK": "1"} if fork else {}, {})
    try:
        for k, pos in enumerate(positions(A.nnz)):
            v, R = one_bad_value(k)
            set_values_in_place(A, v)
            tm = judged_nonfinite_call(t2, A, A, "perturbed_fem", R, f"one {v[pos]} at value {pos} of {A.nnz}")
            assert grouped(tm) < A.M // 30, (pos, tm.num_bins)
        set_values_in_place(A, A0.val)
        near = t2.stat("near")
        tm = judged_call(t2, "perturbed_fem", "wide", "a finite call after nine non-finite ones")
        assert grouped(tm) > 0 and t2.stat("near") == near + 1, (tm.num_bins, near, t2.stat("near"))
    finally:
        t2.close()
        A.d_release_csr()


def test_nonfinite_speculated_calls_across_a_flip(tool):
    """The values flip in place between finite and non-finite under speculated calls: the plan of a finite call has
    near groups, which a non-finite call must not run (and the other way round), so each flip is a miss and a
    rerun -- stats_same_plan compares Stats::nonfinite -- and each repeat a hit."""
    A0 = reference("perturbed_fem", "wide")[0]
    bad, _, R = injected("perturbed_fem", "one")
    A = A0  # (judged_call runs the reference's own operand)
    A.H2D(tool.device)
    t2 = fresh_tool(tool, {}, {})
    try:
        misses = []
        for call, finite in enumerate((True, True, False, False, True)):
            set_values_in_place(A, A0.val if finite else bad.val)
            near = t2.stat("near")
            if finite:
                tm = judged_call(t2, "perturbed_fem", "wide", f"call {call + 1} of the flip sequence, finite")
                assert grouped(tm) > 0 and t2.stat("near") == near + 1, (call, tm.num_bins)
            else:
                tm = judged_nonfinite_call(t2, A, A, "perturbed_fem", R, f"call {call + 1} of the flip sequence, non-finite")
                assert grouped(tm) < A.M // 30 and t2.stat("near") == near, (call, tm.num_bins)
            assert t2.stat("spec") == call, "every call after the first is speculated"
            misses.append(t2.stat("spec_miss"))
        assert misses == [0, 0, 1, 1, 2], misses
    finally:
        t2.close()
        A.d_release_csr()


# ------------------------------------------------------------------ the values plans ---
ALL_PLANS = [(dt, W) for dt in ("f64", "f32") for W in (1, 2, 4)]
assert set(PLANS) <= set(ALL_PLANS)
all_plans = pytest.mark.parametrize("dt,W", ALL_PLANS, ids=[f"{d}-w{w}" for d, w in ALL_PLANS])


def unit(dt):
    return U64 if dt == "f64" else U32


def finite_values(n, seed, dt):
    """Finite non-zero values as the plan's type holds them: wide_values for FP64, [0.1, 1) with a sign for FP32."""
    return wide_values(n, seed) if dt == "f64" else fb.rounded(new_values(n, seed, signed=True), dt)


def finite_sets(n, nb, seed, dt):
    return np.stack([finite_values(n, seed + 17 * b, dt) for b in range(nb)])


def injected_sets(n, nb, seed, dt, zeros=True):
    """nb value sets, each with its own values and its own non-finite positions (at most a third of a short array)."""
    least = min(6, max(1, n // 3))
    return np.stack([inject_nonfinite(finite_values(n, seed + 17 * b, dt), seed + 5 + b, least=least, zeros=zeros)
                     for b in range(nb)])


def forward(tool, plan, dt, av, bv):
    nb = max(av.shape[0] if av.ndim == 2 else 1, bv.shape[0] if bv.ndim == 2 else 1)
    out = nans(tool, (nb, plan.nnzC), dt)
    assert plan.run_batched(up(tool, av, dt), up(tool, bv, dt), out=out) is out
    torch.cuda.synchronize()
    return out.cpu().numpy()


def backward(tool, plan, dt, G, av, bv):
    oA, oB = nans(tool, (G.shape[0], plan.nnzA), dt), nans(tool, (G.shape[0], plan.nnzB), dt)
    plan.grad_batched(up(tool, G, dt), up(tool, av, dt), up(tool, bv, dt), out_A=oA, out_B=oB)
    torch.cuda.synchronize()
    return oA.cpu().numpy(), oB.cpu().numpy()


def row(v, b):
    return v if v.ndim == 1 else v[b]


def forward_reference(pqs, nC, av, bv, dt):
    p, q, s = pqs
    return nonfinite_reference(s, av[p], bv[q], nC, unit(dt))


def grad_references(pqs, nA, nB, av, bv, G, dt):
    p, q, s = pqs
    return nonfinite_reference(p, bv[q], G[s], nA, unit(dt)), nonfinite_reference(q, av[p], G[s], nB, unit(dt))


# 1. every class, forward and backward
def global_rows_n(dt, W):
    return fb.CAPS[W * TYPES[dt][2]][3] + 1  # one past the block-search cap of this plan's table


@functools.lru_cache(maxsize=None)
def class_input(name):
    if name.startswith("global_rows"):  # two rows past a workgroup's LDS at this width
        A, B = (csr_of(t) for t in edge_val(int(name.split("_")[-1]), fb.WIDE, int(name.split("_")[-1]) + 80, copies=2))
    elif name.startswith("wave_direct_rows"):  # eight rows at the wave-direct span of this width
        A, B = (csr_of(t) for t in edge_val(200, int(name.split("_")[-1]), 1000))
    else:
        A, B = (csr_of(t) for t in (bin_zoo() if name == "bin_zoo" else tiny_zoo(7)))
    Cp, Ci = pattern_of(A, B)
    return A, B, Cp, Ci, expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)


NB_MAX = 5  # W + 1 sets a plan: a full pass and the short tail pass


@functools.lru_cache(maxsize=None)
def class_sets(name, dt):
    """Three families of NB_MAX sets of an input, shared by the widths (a width uses the first W + 1) and read only:
    the forward's (values and stored zeros injected into A and B), the backward's with non-finite values and a
    finite non-zero cotangent, and the backward's with finite non-zero values and a non-finite cotangent."""
    A, B, Cp, Ci, pqs = class_input(name)
    nA, nB, nC = A.nnz, B.nnz, len(Ci)
    fwd = (injected_sets(nA, NB_MAX, 100, dt), injected_sets(nB, NB_MAX, 900, dt))
    by_values = (finite_sets(nC, NB_MAX, 500, dt), injected_sets(nA, NB_MAX, 100, dt, zeros=False),
                 injected_sets(nB, NB_MAX, 900, dt, zeros=False))
    by_cotangent = (injected_sets(nC, NB_MAX, 500, dt, zeros=False), finite_sets(nA, NB_MAX, 100, dt),
                    finite_sets(nB, NB_MAX, 900, dt))
    return fwd, by_values, by_cotangent


@functools.lru_cache(maxsize=None)
def class_refs(name, dt, b):
    A, B, Cp, Ci, pqs = class_input(name)
    (av, bv), (G1, a1, b1), (G2, a2, b2) = class_sets(name, dt)
    return (forward_reference(pqs, len(Ci), av[b], bv[b], dt), grad_references(pqs, A.nnz, B.nnz, a1[b], b1[b], G1[b], dt),
            grad_references(pqs, A.nnz, B.nnz, a2[b], b2[b], G2[b], dt))


_INFO = {}


def every_class(tool, name, dt, W):
    if (name, dt, W) not in _INFO:
        A, B, Cp, Ci, _ = class_input(name)
        (av, bv), (G1, a1, b1), (G2, a2, b2) = class_sets(name, dt)
        nb = W + 1
        plan = make_plan(tool, A, B, Cp, Ci, dt, W)
        try:
            info = plan.info()
            assert info["width"] == W
            gC = forward(tool, plan, dt, av[:nb], bv[:nb])
            gA1, gB1 = backward(tool, plan, dt, G1[:nb], a1[:nb], b1[:nb])
            gA2, gB2 = backward(tool, plan, dt, G2[:nb], a2[:nb], b2[:nb])
        finally:
            plan.close()
        for b in range(nb):
            rC, (rA1, rB1), (rA2, rB2) = class_refs(name, dt, b)
            what = f"{name} {dt} W={W} set {b}"
            cls = assert_nonfinite_reference(gC[b], rC, f"{what}, C")
            assert all((cls == c).any() for c in (FINITE, POS_INF, NEG_INF, IS_NAN)), what
            assert_nonfinite_reference(gA1[b], rA1, f"{what}, dA, non-finite values")
            assert_nonfinite_reference(gB1[b], rB1, f"{what}, dB, non-finite values")
            assert_nonfinite_reference(gA2[b], rA2, f"{what}, dA, non-finite cotangent")
            assert_nonfinite_reference(gB2[b], rB2, f"{what}, dB, non-finite cotangent")
            for r in (rA1, rB1, rA2, rB2):
                assert (r[0] != FINITE).any() and (r[0] == FINITE).any()
        print(f"{name} {dt} W={W}: rows per class {info['rows']}")
        _INFO[name, dt, W] = info
    return _INFO[name, dt, W]


def class_names(dt, W):
    """bin_zoo, tiny_zoo and the global rows of the width's table; and, because the zoos' rows leave the wave-direct
    class as the sum bytes grow (none is left at 32), eight rows at that class's span for the width."""
    return ["bin_zoo", "tiny_zoo", f"global_rows_{global_rows_n(dt, W)}", f"wave_direct_rows_{fb.CAPS[W * TYPES[dt][2]][0]}"]


@all_plans
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["bin_zoo", "tiny_zoo", "global_rows", "wave_direct_rows"])
def test_nonfinite_every_class(tool, which, dt, W):
    info = every_class(tool, class_names(dt, W)[which], dt, W)
    if which == 3:
        assert info["rows"][WAVE_DIRECT] == 8, info
    if which == 2:
        assert info["rows"][GLOBAL] == 2, info
    if which == 1:
        assert info["rows"][TEAM] > 0.5 * sum(info["rows"])


@all_plans
def test_nonfinite_every_class_has_rows(tool, dt, W):
    rows = np.sum([every_class(tool, name, dt, W)["rows"] for name in class_names(dt, W)], axis=0)
    for cls in PRODUCT_CLASSES:
        assert rows[cls] > 0, f"class {cls} has no rows at {dt} W={W}"
    assert rows[DOT] == 0


# 2. rows that are one class each: nothing crosses from a neighbouring row of the wave or block
def edges_of(sb):
    """The (at, above) rows of every class edge at sum bytes sb: the tables of tests/test_gpu_values_batched.py, and
    for 4 bytes (the unbatched FP32 plan) the same rungs on its caps."""
    if sb in BYTE_EDGES:
        table = {k: v[:2] for k, v in BYTE_EDGES[sb].items()}
    else:
        wd, ws, bd, bs = fb.CAPS[sb]
        table = {"wave_direct_span": ((200, wd, 1000), (200, wd + 1, 1000)),
                 "wave_search_n": ((ws, fb.WIDE, 2000), (ws + 1, fb.WIDE, 2000)),
                 "block_direct_span": ((3000, bd, 4000), (3000, bd + 1, 4000)),
                 "block_search_n": ((bs, fb.WIDE, bs + 100), (bs + 1, fb.WIDE, bs + 100))}
    table.update({k: v[:2] for k, v in TEAM_EDGES.items()})
    return table


def hand_placed(A, B, av, bv, n, products):
    """edge_val's copies with one non-finite value each in copies 0..4, each reaching one C entry; copies 5, 6, 7
    stay finite.  B row 3j holds copy j's first n - 1 columns, row 3j + 1 the first r of them again, row 3j + 2 its
    last column alone; A row j ends with the entry that points at row 3j + 2."""
    av, bv = av.copy(), bv.copy()
    r = (products - 1) % (n - 1)
    last_a = lambda j: A.ptr[j + 1] - 1  # noqa: E731  (the A entry of row j that points at B row 3j + 2)
    only_b = lambda j: B.ptr[3 * j + 2]  # noqa: E731  (the one entry of B row 3j + 2)
    assert all(A.col[last_a(j)] == 3 * j + 2 and B.ptr[3 * j + 3] - B.ptr[3 * j + 2] == 1 for j in range(5))
    bv[only_b(0)] = np.inf * np.sign(av[last_a(0)])    # copy 0: one product, +Inf
    av[last_a(1)] = -np.inf * np.sign(bv[only_b(1)])   # copy 1: one product, -Inf
    bv[B.ptr[6] + (n - 1) // 2] = np.nan               # copy 2: NaN in the middle of row 3j, under every repeat of it
    av[last_a(3)] = 0.0                                # copy 3: a stored zero against an Inf
    bv[only_b(3)] = np.inf
    bv[B.ptr[3 * 4 + 1] if r else B.ptr[3 * 4]] = -np.inf  # copy 4: the first entry of row 3j + 1 (of row 3j where it is empty)
    return av, bv


@all_plans
@pytest.mark.parametrize("side", [0, 1], ids=["at", "above"])
@pytest.mark.parametrize("name", fb.EDGE_NAMES)
def test_nonfinite_class_edges_rows_alone(tool, name, side, dt, W):
    sb = W * TYPES[dt][2]
    n, span, products = edges_of(sb)[name][side]
    A, B, Cp, Ci, (p, q, s) = fb.edge_rows_of(n, span, products)
    nb = W + 1
    sets = [hand_placed(A, B, edge_values(A.nnz, 50 + b), edge_values(B.nnz, 80 + b), n, products) for b in range(nb)]
    av, bv = np.stack([x for x, _ in sets]), np.stack([y for _, y in sets])
    plan = make_plan(tool, A, B, Cp, Ci, dt, W)
    try:
        info = plan.info()
        classes = [c for c in range(8) if info["rows"][c]]
        assert classes == [fb.val_class(n, span, products, sb)], (classes, info)
        got = forward(tool, plan, dt, av, bv)
    finally:
        plan.close()
    rows = np.repeat(np.arange(A.M), np.diff(Cp))
    for b in range(nb):
        want = product_classes(s, av[b][p], bv[b][q], len(Ci))
        bad = np.nonzero(want != FINITE)[0]
        assert len(bad) == 5 and rows[bad].tolist() == [0, 1, 2, 3, 4], "one entry in each of the first five copies"
        assert want[bad[0]] == POS_INF and want[bad[1]] == NEG_INF and want[bad[2]] == IS_NAN and want[bad[3]] == IS_NAN
        assert np.array_equal(classes_of(got[b]), want), f"set {b}: {rows[np.nonzero(classes_of(got[b]) != want)[0]]}"
        fin = want == FINITE
        keep = fin[s]
        exact = np.bincount(s[keep], av[b][p[keep]] * bv[b][q[keep]], len(Ci))  # integers: exact in either type
        assert np.array_equal(got[b].astype(np.float64)[fin], exact[fin]), f"set {b}: the finite entries, exactly"
    print(f"{name} side {side} {dt} W={W}: class {classes}")


# 3. masked plans: a dropped product reaches nothing
@functools.lru_cache(maxsize=None)
def mask_input(case):
    A, B, Mp, Mc = masked_case(case)
    Cp, Ci = pattern_of(A, B)
    kept = expand(A.ptr, A.col, B.ptr, B.col, Mp, Mc, B.N)
    every = expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)
    return A, B, Mp, Mc, kept, every


@functools.lru_cache(maxsize=None)
def mask_sets(case, dt):
    A, B, Mp, Mc, kept, (p, q, s) = mask_input(case)
    av, bv = injected_sets(A.nnz, NB_MAX, 400, dt), injected_sets(B.nnz, NB_MAX, 600, dt)
    a1, b1 = injected_sets(A.nnz, NB_MAX, 400, dt, zeros=False), injected_sets(B.nnz, NB_MAX, 600, dt, zeros=False)
    G = finite_sets(len(Mc), NB_MAX, 800, dt)
    return av, bv, a1, b1, G


@functools.lru_cache(maxsize=None)
def mask_refs(case, dt, b):
    """The references of set b on the kept products, and the mask entries of rows in which a non-finite product was
    dropped: they must come out in the class of their own products all the same."""
    A, B, Mp, Mc, kept, (p, q, s) = mask_input(case)
    av, bv, a1, b1, G = mask_sets(case, dt)
    rC = forward_reference(kept, len(Mc), av[b], bv[b], dt)
    with np.errstate(invalid="ignore"):
        w = av[b][p] * bv[b][q]
    Cp, Ci = pattern_of(A, B)
    N = B.N
    crow = np.repeat(np.arange(A.M, dtype=np.int64), np.diff(Cp))
    mkey = np.repeat(np.arange(A.M, dtype=np.int64), np.diff(Mp)) * N + Mc
    dropped = ~np.isin(crow[s] * N + Ci[s], mkey) & ~np.isfinite(w)
    assert dropped.sum() > 0, "non-finite products that fall outside the mask"
    beside = np.isin(mkey // N, np.unique(crow[s[dropped]]))
    clean = beside & (rC[0] == FINITE)
    assert clean.any(), "finite mask entries in the rows of dropped non-finite products"
    return rC, grad_references(kept, A.nnz, B.nnz, a1[b], b1[b], G[b], dt), int(dropped.sum()), int(clean.sum())


@all_plans
@pytest.mark.parametrize("form", ["product", "dot", "auto"])
@pytest.mark.parametrize("case", ["triangle", "thinned_with_strangers"])
def test_nonfinite_masked_forms(tool, case, form, dt, W):
    A, B, Mp, Mc, kept, every = mask_input(case)
    av, bv, a1, b1, G = mask_sets(case, dt)
    nb = W + 1
    plan = make_plan(tool, A, B, Mp, Mc, dt, W, masked=True, form=form)
    try:
        info = plan.info()
        assert info["kept_products"] == len(kept[0]) < info["products"] == len(every[0])
        if form != "auto":
            assert (info["rows"][DOT] > 0) == (form == "dot"), (form, info)
        gC = forward(tool, plan, dt, av[:nb], bv[:nb])
        gA, gB = backward(tool, plan, dt, G[:nb], a1[:nb], b1[:nb])
    finally:
        plan.close()
    for b in range(nb):
        rC, (rA, rB), dropped, clean = mask_refs(case, dt, b)
        what = f"{case} {form} {dt} W={W} set {b}"
        assert_nonfinite_reference(gC[b], rC, f"{what}, C ({dropped} non-finite products dropped beside {clean} finite entries)")
        assert_nonfinite_reference(gA[b], rA, f"{what}, dA")
        assert_nonfinite_reference(gB[b], rB, f"{what}, dB")
    print(f"{case} {form} {dt} W={W}: rows per class {info['rows']}")


# 4. sets do not poison each other
@all_plans
def test_nonfinite_sets_do_not_poison_each_other(tool, dt, W):
    """2 W + 1 sets, non-finite values in set 1 and in the last set only -- the short tail pass.  The other sets hold
    the finite bound, and their dA has the bits of the same call with every set finite (the header fixes dA's bits
    per set).  Then A shared by all sets (stride 0) and non-finite: every set shows it."""
    A, Cp, Ci, pqs = fb.square_case()
    nnz, nC, nb = A.nnz, len(Ci), 2 * W + 1
    hot = sorted({1, nb - 1})
    clean_a, clean_b, G = finite_sets(nnz, nb, 300, dt), finite_sets(nnz, nb, 700, dt), finite_sets(nC, nb, 1100, dt)
    av, bv = clean_a.copy(), clean_b.copy()
    for b in hot:
        av[b] = inject_nonfinite(av[b], 40 + b, rate=0.02, zeros=False)
        bv[b] = inject_nonfinite(bv[b], 60 + b, rate=0.02, zeros=False)
    shared = inject_nonfinite(clean_a[0], 77, rate=0.02)
    plan = make_plan(tool, A, A, Cp, Ci, dt, W)
    try:
        gC = forward(tool, plan, dt, av, bv)
        gA, gB = backward(tool, plan, dt, G, av, bv)
        fA, _ = backward(tool, plan, dt, G, clean_a, clean_b)
        sC = forward(tool, plan, dt, shared, clean_b)
        sA, sB = backward(tool, plan, dt, G, shared, clean_b)
    finally:
        plan.close()
    bits = np.uint64 if dt == "f64" else np.uint32
    for b in range(nb):
        what = f"{dt} W={W} set {b} of {nb}"
        if b in hot:
            rA, rB = grad_references(pqs, nnz, nnz, av[b], bv[b], G[b], dt)
            cls = assert_nonfinite_reference(gC[b], forward_reference(pqs, nC, av[b], bv[b], dt), f"{what}, C, non-finite")
            assert (cls != FINITE).any()
            assert_nonfinite_reference(gA[b], rA, f"{what}, dA, non-finite")
            assert_nonfinite_reference(gB[b], rB, f"{what}, dB, non-finite")
        else:
            refA, refB = grad_reference(pqs, nnz, nnz, av[b], bv[b], G[b], dt)
            fb.assert_set(gC[b], fb.reference(pqs, nC, av[b], bv[b], dt), dt, f"{what}, C beside non-finite sets")
            fb.assert_set(gA[b], refA, dt, f"{what}, dA beside non-finite sets")
            fb.assert_set(gB[b], refB, dt, f"{what}, dB beside non-finite sets")
            assert np.array_equal(np.ascontiguousarray(gA[b]).view(bits), np.ascontiguousarray(fA[b]).view(bits)), \
                f"{what}: dA's bits with every set finite"
        # A shared and non-finite: C and dB of every set show it (dA reads B and G only: finite)
        rA, rB = grad_references(pqs, nnz, nnz, shared, clean_b[b], G[b], dt)
        cls = assert_nonfinite_reference(sC[b], forward_reference(pqs, nC, shared, clean_b[b], dt), f"{what}, C, A shared")
        assert all((cls == c).any() for c in (POS_INF, NEG_INF, IS_NAN)), what
        assert (assert_nonfinite_reference(sB[b], rB, f"{what}, dB, A shared") != FINITE).any()
        assert (assert_nonfinite_reference(sA[b], rA, f"{what}, dA, A shared") == FINITE).all()


# 5. the carve-out: a zero cotangent times a non-finite value may give 0 or NaN
@functools.lru_cache(maxsize=None)
def carve_case(dt):
    """bin_zoo with non-finite values in A and B, and a cotangent that is zero at every second C entry a non-finite
    product lands in.  Per side: the reference over all products, the products the carve-out covers (zero cotangent,
    non-finite value), the entries they reach and the reference without them."""
    A, B, Cp, Ci, (p, q, s) = class_input("bin_zoo")
    av = inject_nonfinite(finite_values(A.nnz, 100, dt), 105, zeros=False)
    bv = inject_nonfinite(finite_values(B.nnz, 900, dt), 905, zeros=False)
    G = finite_values(len(Ci), 500, dt)
    hit = np.unique(s[~np.isfinite(av[p]) | ~np.isfinite(bv[q])])
    G[hit[::2]] = 0.0
    sides = []
    for idx, x, n in ((p, bv[q], A.nnz), (q, av[p], B.nnz)):
        carved = (G[s] == 0.0) & ~np.isfinite(x)
        reached = np.zeros(n, bool)
        reached[idx[carved]] = True
        assert 0 < reached.sum() < n // 10, "entries a carved product reaches: some, and fewer than one in ten"
        sides.append((nonfinite_reference(idx, x, G[s], n, unit(dt)), reached,
                      nonfinite_reference(idx[~carved], x[~carved], G[s][~carved], n, unit(dt))))
    return A, B, Cp, Ci, av, bv, G, sides


@all_plans
def test_carve_out_zero_cotangent(tool, dt, W):
    """include/mhspgemm.h, mhs_spgemm_values_grad: "A zero cotangent times a non-finite value may give 0 or NaN" --
    the direct classes skip a product whose staged cotangent is zero in every set.  Entries no such product reaches
    hold the contract; an entry one reaches is NaN, or holds the contract computed without those products."""
    A, B, Cp, Ci, av, bv, G, sides = carve_case(dt)
    nb = W + 1
    plan = make_plan(tool, A, B, Cp, Ci, dt, W)
    try:
        got = backward(tool, plan, dt, np.stack([G] * nb), np.stack([av] * nb), np.stack([bv] * nb))
    finally:
        plan.close()
    for g, (everything, reached, without), side in zip(got, sides, ("dA", "dB")):
        for b in range(nb):
            what = f"carve-out {dt} W={W} set {b}, {side}"
            assert_nonfinite_reference(g[b], everything, f"{what}, entries no carved product reaches", only=~reached)
            number = reached & ~np.isnan(g[b].astype(np.float64))
            assert_nonfinite_reference(g[b], without, f"{what}, reached entries that are not NaN", only=number)
            print(f"{what}: {reached.sum()} reached entries, {number.sum()} of them without the carved products")
