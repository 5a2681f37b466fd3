"""GPU tests of the values plans (forward and backward; plain and masked; FP64 and FP32; width 1, 2 and 4), of
mhs_transpose / AAT and of the driver on operands that repeat column indices within a row.

include/mhspgemm.h: "duplicates in A or B are summed" -- two products of one A entry land in one C slot, every
repeat of a B entry contributes to dAval and gets its own dBval, and mhs_transpose keeps "duplicates of A ... in
A's order".  The inputs are the repeat twins of tests/_dups.py.  Values and cotangents are integers of +-{1, 2, 3}:
every sum is exact in either type in any order while 9 * (products of an entry) < 2^24, which exact_sets asserts
on the host, so every output is compared with np.array_equal against sums of the expanded products taken in
float64; nothing here carries a tolerance.  Outputs start NaN-filled; entries no product reaches are exactly 0.
Mixed plans (float values summed in double) run as a third kind of plan on the same inputs, exact for the same reason.

Under min-plus, max-plus and max-min "every duplicate entry is a product of its own": repeats count in ties and share
their k in the witness.  The same twins run through the semiring plans' forward, subgradient and witness with the
checks of tests/test_gpu_subgrad.py and test_gpu_witness.py as they are, then once more on values in which every repeat
of a B entry copies the first of its run, where those sentences can be tested: all comparisons are np.array_equal.  The
smoothed min-plus and max-plus plans run on the twins too, held to the header's bounds by tests/test_gpu_smooth.py's
assert_forward and assert_grad."""
import functools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import mhspgemm
from oracle import oracle as orc
from _dups import is_legal, present, repeat_kinds, split_repeats, with_repeats
from _util import bin_zoo, csr_of, edge_val, edge_values, expand, random_csr, tiny_zoo
import test_gpu_values_batched as fb
from test_gpu_values_batched import (BLOCK_DIRECT, BLOCK_SEARCH, DOT, GLOBAL, TEAM, TYPES, WAVE_DIRECT, WAVE_SEARCH, WIDE,
                                     make_plan, nans, pattern_of, up)
from test_gpu_values_grad_batched import bits, call
import test_gpu_semiring as srf
import test_gpu_smooth as sm
import test_gpu_subgrad as sub
import test_gpu_witness as wit

pytestmark = pytest.mark.gpu

# (dt, W, accum): the FP64 and FP32 plans, and the mixed plans -- float values summed in double (accum "float64"), whose
# classes are those of the sum bytes 8 W.  Integer values make a mixed plan's double sums exact as well.
PLANS = [(dt, W, None) for dt in ("f64", "f32") for W in (1, 2, 4)] + [("f32", W, "float64") for W in (1, 2, 4)]
plans = pytest.mark.parametrize("dt,W,accum", PLANS, ids=[f"{'mixed' if a else d}-w{w}" for d, w, a in PLANS])
PRODUCT = (TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL)
NB_MOST = 5  # W + 1 sets for the widest plan


def integer_sets(n, seed):
    return np.stack([edge_values(n, seed + b) for b in range(NB_MOST)])


def repeat_pairs(X):
    """Index pairs (j, j + 1) of stored entries of one row with one column."""
    rows = np.repeat(np.arange(X.M), np.diff(X.ptr))
    eq = (X.col[1:] == X.col[:-1]) & (rows[1:] == rows[:-1])
    return np.nonzero(eq)[0]


@functools.lru_cache(maxsize=None)
def exact_sets(key):
    """A case's operands, pattern, kept products, NB_MOST integer sets of values and cotangents, and the exact
    outputs of every set: (A, B, Cp, Ci, pqs, av, bv, G, wantC, wantA, wantB).  Shared by the types and widths."""
    A, B, Cp, Ci = CASES[key]()
    assert is_legal((A.M, A.N, A.ptr, A.col, A.val)) and is_legal((B.M, B.N, B.ptr, B.col, B.val))
    p, q, s = pqs = expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)
    most = max(np.bincount(s, minlength=len(Ci)).max(initial=0), np.bincount(p, minlength=A.nnz).max(initial=0),
               np.bincount(q, minlength=B.nnz).max(initial=0))
    assert 9 * int(most) < 2 ** 24, "integers below 2^24: exact in float, in any order"
    av, bv, G = integer_sets(A.nnz, 50), integer_sets(B.nnz, 80), integer_sets(len(Ci), 110)
    wantC = np.stack([np.bincount(s, av[b][p] * bv[b][q], len(Ci)) for b in range(NB_MOST)])
    wantA = np.stack([np.bincount(p, bv[b][q] * G[b][s], A.nnz) for b in range(NB_MOST)])
    wantB = np.stack([np.bincount(q, av[b][p] * G[b][s], B.nnz) for b in range(NB_MOST)])
    return A, B, Cp, Ci, pqs, av, bv, G, wantC, wantA, wantB


def check_plan(tool, key, dt, W, **kw):
    """A plan of the case at (dt, W): the forward with nb = W + 1 sets (a full pass and a tail), the backward with both
    sides, with dA only and with dB only, all into NaN-filled outputs and all equal to the exact sums; then what
    the contract says of repeats: each repeat of an A entry has its own, equal dAval, each repeat of a B entry its
    own dBval, equal as the repeats of one row see the same A entries.  Returns (info(), the forward's values)."""
    A, B, Cp, Ci, pqs, av, bv, G, wantC, wantA, wantB = exact_sets(key)
    nb = W + 1
    plan = make_plan(tool, A, B, Cp, Ci, dt, W, **kw)
    try:
        info = plan.info()
        assert info["width"] == W and info["kept_products"] == len(pqs[0])
        dAv, dBv, dG = up(tool, av[:nb], dt), up(tool, bv[:nb], dt), up(tool, G[:nb], dt)
        out = nans(tool, (nb, len(Ci)), dt)
        plan.run_batched(dAv, dBv, out=out)
        torch.cuda.synchronize()
        gC = out.cpu().numpy()
        gA, gB = call(tool, plan, dt, dG, dAv, dBv, nb)
        onlyA, none = call(tool, plan, dt, dG, dAv, dBv, nb, need_B=False)
        assert none is None
        none, onlyB = call(tool, plan, dt, dG, dAv, dBv, nb, need_A=False)
        assert none is None
    finally:
        plan.close()
    what = f"{key} {dt} W={W}"
    for b in range(nb):
        for got, want, name in ((gC, wantC, "C"), (gA, wantA, "dA"), (gB, wantB, "dB"), (onlyA, wantA, "dA alone"),
                                (onlyB, wantB, "dB alone")):
            g = got[b].astype(np.float64)
            assert np.array_equal(g, want[b]), f"{what} set {b} {name}: {np.count_nonzero(g != want[b])} of {len(g)} entries differ"
        ja, jb = repeat_pairs(A), repeat_pairs(B)
        assert np.array_equal(gA[b][ja], gA[b][ja + 1]), f"{what} set {b}: the repeats of an A entry have equal gradients"
        assert np.array_equal(gB[b][jb], gB[b][jb + 1]), f"{what} set {b}: the repeats of a B entry have equal gradients"
    return info, gC


# ------------------------------------------------------------------ plain plans ---
def zoo_twin(zoo, seed):
    At, Bt = zoo()
    twin, counts = with_repeats(Bt, seed)
    assert present(counts) >= set("abcdefi"), counts
    A, B = csr_of((*At[:4], edge_values(len(At[3]), 1))), csr_of(twin)
    return (A, B) + pattern_of(A, B)


def global_rows(n):
    """edge_val's two rows of n entries over a wide span, past the block-search cap, with repeats in its B rows: the
    long rows take the remainder (kind i), the rows of one entry hold it 200 and 65 times."""
    At, Bt = edge_val(n, WIDE, n + 87, copies=2)
    twin, counts = with_repeats(Bt, 3, share=0.05, kinds="ei")
    assert counts["i"] > 100 and counts["e_single_200"] == 1 and counts["e_single_65"] == 1, counts
    A, B = csr_of(At), csr_of(twin)
    return (A, B) + pattern_of(A, B)


def wave_direct_rows():
    """Eight rows of 200 entries over 256 columns with about 1,300 products: the wave-direct class at every sum-byte
    size.  (At 32 sum bytes, FP64 width 4, that class spans at most 256 columns and neither zoo has such a row.)"""
    At, Bt = edge_val(200, 256, 1000)
    twin, counts = with_repeats(Bt, 4, kinds="ei")
    assert counts["i"] > 50 and counts["e_single_200"] == 1 and counts["e_single_65"] == 1, counts
    A, B = csr_of(At), csr_of(twin)
    return (A, B) + pattern_of(A, B)


CASES = {
    "wave_direct_rows": wave_direct_rows,
    "bin_zoo": lambda: zoo_twin(bin_zoo, 21),
    "tiny_zoo": lambda: zoo_twin(lambda: tiny_zoo(7), 22),
    "global_rows": lambda: global_rows(13313),      # past the block-search cap of sum bytes >= 8 (13,312)
    "global_rows_f32": lambda: global_rows(19969),  # ... and of the FP32 width-1 plan's 4 sum bytes (19,968)
}


def plain_inputs(dt, W, accum=None):
    """The inputs of a plan: the twins of bin_zoo, tiny_zoo and global_rows, and wave_direct_rows, without which
    the FP64 width-4 plans have no wave-direct row.  edge_val(13313, ...) is past every plan's block-search cap but
    the FP32 width-1 plan's, whose rows of the global class need 19,969 entries (tests/test_gpu_f64_bound.py's).
    A mixed plan (accum) classifies at 8 W sum bytes: it never has the 4 of that plan."""
    four_sum_bytes = (dt, W) == ("f32", 1) and accum is None
    return ["bin_zoo", "tiny_zoo", "global_rows_f32" if four_sum_bytes else "global_rows", "wave_direct_rows"]


def plan_keywords(accum):
    """make_plan's keywords of a PLANS entry: accum reaches ValuesPlan through them, on mixed plans only."""
    return {} if accum is None else {"accum": accum}


_PLAIN = {}


def plain(tool, key, dt, W, accum=None):
    if (key, dt, W, accum) not in _PLAIN:
        _PLAIN[key, dt, W, accum] = check_plan(tool, key, dt, W, **plan_keywords(accum))[0]
    return _PLAIN[key, dt, W, accum]


@plans
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["bin_zoo", "tiny_zoo", "global_rows", "wave_direct_rows"])
def test_repeats_plain_plan(tool, which, dt, W, accum):
    key = plain_inputs(dt, W, accum)[which]
    info = plain(tool, key, dt, W, accum)
    assert info["accum"] == accum and info["dtype"] == ("float64" if dt == "f64" else "float32"), info
    A, B = exact_sets(key)[:2]
    assert len(repeat_pairs(B)) > 0 and (which == 2 or len(repeat_pairs(A)) > 0), "repeats in B, and in A but for global_rows"
    if which == 3:
        assert info["rows"][WAVE_DIRECT] == A.M, info
    if which == 1:
        assert info["rows"][TEAM] > 0.5 * sum(info["rows"]), info
    if which == 2:
        assert info["rows"][GLOBAL] == 2, info


@plans
def test_repeats_plain_every_class_has_rows(tool, dt, W, accum):
    rows = np.sum([plain(tool, key, dt, W, accum)["rows"] for key in plain_inputs(dt, W, accum)], axis=0)
    for cls in PRODUCT:
        assert rows[cls] > 0, f"class {cls} has no rows at {dt} W={W} accum={accum}"
    assert rows[DOT] == 0


# ------------------------------------------------------------------ semiring plans ---
INPUT_IDS = ["bin_zoo", "tiny_zoo", "global_rows", "wave_direct_rows"]
DTYPES = {"float64": "f64", "float32": "f32"}


@functools.lru_cache(maxsize=None)
def semiring_input(key):
    """A case for the semiring plans: (A, B, Cp, Ci, kept products), then what the repeats of B are -- per stored B
    entry whether it is one of several copies and the position of the first of its run, the positions of the runs'
    first copies, and the kept products of A times B with every run collapsed to one entry (the same C pattern)."""
    A, B, Cp, Ci, pqs = exact_sets(key)[:5]
    p1, c1, mult, start = split_repeats((B.M, B.N, B.ptr, B.col, B.val))
    assert (mult > 1).any() and np.array_equal(B.col[start], c1)
    return (A, B, Cp, Ci, pqs, np.repeat(mult > 1, mult), np.repeat(start, mult), start,
            expand(A.ptr, A.col, p1, c1, Cp, Ci, B.N))


_HARD = {}


def hard_info(tool, key, dtype, sr):
    """info() of the semiring plan of a case, from the test that ran it where it has."""
    if (key, dtype, sr) not in _HARD:
        A, B, Cp, Ci = semiring_input(key)[:4]
        plan = mhspgemm.ValuesPlan(tool, *srf.on_device(tool, A, B, Cp, Ci), dtype=dtype, semiring=sr)
        try:
            _HARD[key, dtype, sr] = plan.info()
        finally:
            plan.close()
    return _HARD[key, dtype, sr]


@pytest.mark.parametrize("sr", srf.SEMIRINGS)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=INPUT_IDS)
def test_repeats_semiring_plan(tool, which, dtype, sr):
    key = plain_inputs(DTYPES[dtype], 1)[which]
    A, B, Cp, Ci, pqs, copied, first_copy, start, merged_pqs = semiring_input(key)
    nC = len(Ci)
    what = f"{key} {sr} {dtype}"
    plan = mhspgemm.ValuesPlan(tool, *srf.on_device(tool, A, B, Cp, Ci), dtype=dtype, semiring=sr)
    try:
        _HARD[key, dtype, sr] = info = plan.info()
        assert info["kept_products"] == len(pqs[0]) and info["semiring"] == sr and info["dtype"] == dtype
        if which == 2:
            assert info["rows"][GLOBAL] == 2, info
        if which == 3:
            assert info["rows"][WAVE_DIRECT] == A.M, info
        # the forward, the subgradient and the witness as any input's: both regimes of both
        sub.check_exact(tool, plan, A, B, nC, pqs, sr, dtype, 700)
        sub.check_general(tool, plan, A, B, nC, pqs, sr, dtype, 707, what)
        wit.check_exact(tool, plan, A, B, nC, pqs, sr, dtype, 700)
        wit.check_general(tool, plan, A, B, nC, pqs, sr, dtype, 707)
        # a second draw: every repeat of a B entry has the value of the first of its run.  (A B row that exact_values
        # saw without an infinity has none after the copying either: still no product is Inf - Inf.)
        av, bv = sub.exact_values(sr, A, B, 720)
        bv = bv[first_copy]
        cdev = sub.forward_values(tool, plan, nC, dtype, av, bv)
        c = cdev.cpu().numpy()
        assert np.array_equal(c, srf.reference(sr, pqs, av, bv, nC, dtype)) and not np.isnan(c).any(), f"{what}: the forward"
        win, T = sub.winners(sr, pqs, av, bv, c, dtype)
        p, q, s = pqs
        through = win & copied[q]  # the products won through a repeated B entry
        assert through.any(), "the case needs a winner that is a repeat"
        g = np.random.default_rng(721).integers(-2, 3, nC).astype(np.float64)
        G = np.where(T > 0, T * g, np.nan)
        _, gA, gB, ties = sub.call(tool, plan, A.nnz, B.nnz, nC, dtype, av, bv, G, cval=cdev)
        wA, wB = sub.exact_reference(sr, pqs, win, T, av, bv, G, A.nnz, B.nnz, dtype)
        assert np.array_equal(ties, T) and np.array_equal(gA, wA) and np.array_equal(gB, wB), what
        jb = repeat_pairs(B)
        won = np.bincount(q[win], minlength=B.nnz)
        assert np.array_equal(won[jb], won[jb + 1]), "the reference: both copies win or neither does"
        assert (won[jb] > 0).any() and np.array_equal(gB[jb], gB[jb + 1]), f"{what}: the repeats of a B entry get equal dB"
        assert np.all(ties[s[through]] >= 2), f"{what}: every duplicate is a product of its own, so a repeat that wins ties"
        # duplicates share their k: the witness is that of B with every run of repeats collapsed to one entry
        _, w = wit.call(tool, plan, nC, dtype, av, bv, cval=cdev)
        merged, _ = wit.witness_reference(sr, A, merged_pqs, av, bv[start], c, dtype)
        assert np.array_equal(w, merged), f"{what}: wit is the witness of the collapsed B"
        assert np.array_equal(w >= 0, ties >= 1)
    finally:
        plan.close()


@pytest.mark.parametrize("sr", srf.SEMIRINGS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_repeats_semiring_every_class_has_rows(tool, dtype, sr):
    rows = np.sum([hard_info(tool, key, dtype, sr)["rows"] for key in plain_inputs(DTYPES[dtype], 1)], axis=0)
    for cls in PRODUCT:
        assert rows[cls] > 0, f"class {cls} has no rows at {sr} {dtype}"
    assert rows[DOT] == 0


# ------------------------------------------------------------------ smoothed plans ---
@pytest.mark.parametrize("sr", sm.SEMIRINGS)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=INPUT_IDS)
def test_repeats_smooth_plan(tool, which, dtype, sr):
    """The log-sum-exp plans classify at twice the value's bytes, as a width-2 plan: global_rows(13313) is past the
    block-search cap at both sizes.  Global rows are held to the global bound, the others to the LDS classes'."""
    key = plain_inputs(DTYPES[dtype], 2)[which]
    assert key != "global_rows_f32"
    A, B, Cp, Ci, pqs = semiring_input(key)[:5]
    nC = len(Ci)
    what = f"{key} {sr} {dtype}"
    av, bv = sm.values(A.nnz, 731, dtype), sm.values(B.nnz, 1731, dtype)
    G = sm.values(nC, 733, dtype, -1.0, 1.0)
    is_global, nglobal = sm.global_entries(A, B, Cp, Ci, dtype)
    plan, info = sm.soft_plan(tool, *srf.on_device(tool, A, B, Cp, Ci), sr, dtype)
    try:
        assert info["rows"][GLOBAL] == nglobal and info["rows"][DOT] == 0 and info["kept_products"] == len(pqs[0]), info
        if which == 2:
            assert nglobal == 2 and is_global.all(), info
        got = sm.forward(tool, plan, av, bv, nC, dtype)
        sm.assert_forward(got, sm.soft_reference(sr, pqs, av, bv, nC, dtype), is_global, dtype, what)
        rA, rB = sm.grad_reference(sr, pqs, av, bv, got, G, A.nnz, B.nnz, dtype)
        gA, gB = sm.backward(tool, plan, G, got, av, bv, A.nnz, B.nnz, dtype)
        sm.assert_grad(gA, rA, G, dtype, f"{what} dA")
        sm.assert_grad(gB, rB, G, dtype, f"{what} dB")
        again, _ = sm.backward(tool, plan, G, got, av, bv, A.nnz, B.nnz, dtype)
        assert again.tobytes() == gA.tobytes(), f"{what}: dA has a fixed order, the same bits on two calls"
    finally:
        plan.close()


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_repeats_smooth_every_class_has_rows(tool, dtype):
    rows = np.zeros(8, np.int64)
    for key in plain_inputs(DTYPES[dtype], 2):
        A, B, Cp, Ci = semiring_input(key)[:4]
        plan, info = sm.soft_plan(tool, *srf.on_device(tool, A, B, Cp, Ci), "min_plus", dtype)
        plan.close()
        rows += info["rows"]
    for cls in PRODUCT:
        assert rows[cls] > 0, f"class {cls} has no rows at lse {dtype}"


# ------------------------------------------------------------------ masked plans ---
def twin_csr(X, seed):
    twin, counts = with_repeats((X.M, X.N, X.ptr, X.col, X.val), seed)
    assert present(counts) >= set("abcdfi"), counts
    return csr_of(twin)


def triangle_twin():
    """L * L on L's pattern (tests/test_gpu_values_batched.py's triangle), L with repeats: A and B are one matrix."""
    L, _, Mp, Mc = fb.triangle_case()
    T = twin_csr(L, 31)
    return T, T, Mp, Mc


def rect_twin():
    """The rect case there, A and B both with repeats, on its mask: half of the clean product's pattern."""
    A, B, Mp, Mc = fb.rect_mask_case()
    return twin_csr(A, 32), twin_csr(B, 33), Mp, Mc


CASES["triangle"] = triangle_twin
CASES["rect"] = rect_twin


@plans
@pytest.mark.parametrize("form", ["product", "dot", "auto"])
@pytest.mark.parametrize("case", ["triangle", "rect"])
def test_repeats_masked_forms(tool, case, form, dt, W, accum):
    A, B, Mp, Mc, pqs, av, bv = exact_sets(case)[:7]
    assert len(repeat_pairs(A)) > 0 and len(repeat_pairs(B)) > 0
    kw = dict(masked=True, form=form, **plan_keywords(accum))
    info, gC = check_plan(tool, case, dt, W, **kw)
    assert info["accum"] == accum, info
    assert 0 < info["kept_products"] < info["products"] == orc.flop(A.col, B.ptr), "the case needs products outside the mask"
    if form == "dot":
        assert info["rows"][DOT] > 0 and info["dot"] > 0, info
    if form == "product":
        assert info["rows"][DOT] == 0 and info["dot"] == 0, info
    if info["rows"][DOT] > 0:  # dot rows: two calls give the same bits, a batched set has the unbatched call's bits
        nb = W + 1
        dAv, dBv = up(tool, av[:nb], dt), up(tool, bv[:nb], dt)
        plan, plan1 = make_plan(tool, A, B, Mp, Mc, dt, W, **kw), None
        try:
            again = nans(tool, (nb, len(Mc)), dt)
            plan.run_batched(dAv, dBv, out=again)
            torch.cuda.synchronize()
            assert np.array_equal(bits(again.cpu().numpy()), bits(gC)), "two batched calls, the same bits"
            plan1 = make_plan(tool, A, B, Mp, Mc, dt, 1, **kw)
            assert plan1.info()["dot"] == info["dot"]
            for b in range(nb):
                o = nans(tool, (len(Mc),), dt)
                plan1.run(dAv[b], dBv[b], out=o)
                torch.cuda.synchronize()
                assert np.array_equal(bits(o.cpu().numpy()), bits(gC[b])), f"set {b}: the unbatched call's bits"
        finally:
            plan.close()
            if plan1 is not None:
                plan1.close()


# ------------------------------------------------------------------ transpose and AAT ---
def _csr(M, N, rows):
    ptr = np.zeros(M + 1, np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate(rows).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)
    # values all different, so the order of the repeats of an entry shows in the transpose
    return M, N, ptr.astype(np.int32), col, 1.0 + np.arange(len(col)) / 1024.0


def transpose_case(name):
    rng = np.random.default_rng(61)
    if name == "repeats":  # rectangular, every kind of repeat the matrix can hold, adjacent repeats with different values
        p, c, v = random_csr(700, 1900, 6, seed=2600)
        twin, counts = with_repeats((700, 1900, p, c, v), 41)
        assert present(counts) >= set("abcdefi"), counts
        return twin[:4] + (1.0 + np.arange(len(twin[3])) / 1024.0,)
    if name == "no_entries":
        return _csr(5, 7, [[]] * 5)
    if name == "empty_edge_columns":  # the first and the last hundred columns are empty
        return _csr(300, 1000, [np.sort(rng.integers(100, 900, int(rng.integers(0, 9)))) for _ in range(300)])
    if name == "one_column":  # N = 1: every entry is a repeat of (i, 0)
        return _csr(500, 1, [np.zeros(int(rng.integers(0, 4)), np.int64) for _ in range(500)])
    if name in ("n_1024", "n_1025"):  # the column sort's last key bit: N = 2^k, 2^k + 1, the last column used
        N = int(name[2:])
        rows = [np.sort(rng.integers(0, N, int(rng.integers(0, 9)))) for _ in range(400)]
        rows[7] = np.array([0, N - 1, N - 1])
        return _csr(400, N, rows)
    k = int(name.rsplit("_", 1)[1])  # nnz_256, nnz_2048: an exact multiple of 256 entries
    return _csr(k // 4, 333, [np.sort(rng.integers(0, 333, 4)) for _ in range(k // 4)])


TRANSPOSE_CASES = ["repeats", "no_entries", "empty_edge_columns", "one_column", "n_1024", "n_1025", "nnz_256", "nnz_2048"]


@pytest.mark.parametrize("name", TRANSPOSE_CASES)
def test_repeats_transpose_bit_exact(tool, name):
    """mhs_transpose against the oracle's transpose: ptr, col and val bit for bit -- the repeats of an entry stay
    repeated entries of the transpose, in A's order (all values differ, so their order shows)."""
    M, N, p, c, v = t = transpose_case(name)
    assert is_legal(t) and len(np.unique(v)) == len(v)
    if name in ("repeats", "one_column", "n_1024", "n_1025"):
        assert repeat_kinds(t)["repeated_entries"] > 0
    if name.startswith("nnz_"):
        assert len(c) % 256 == 0 and len(c) > 0
    if name == "empty_edge_columns":
        assert c.min() >= 100 and c.max() < 900
    A = mhspgemm.CSR(M, N, p, c, v)
    A.H2D(tool.device)
    try:
        T = mhspgemm.transpose(tool, A)
        try:
            tp, tc, tv = T.dev.to_host()
        finally:
            T.d_release_csr()
    finally:
        A.d_release_csr()
    oM, oN, op, oc, ov = orc.transpose(M, N, p, c, v)
    assert (T.M, T.N) == (N, M) == (oM, oN) and T.nnz == len(c)
    assert np.array_equal(tp, op) and np.array_equal(tc, oc)
    assert np.array_equal(np.asarray(tv).view(np.uint64), ov.view(np.uint64)), "the repeats' values keep A's order"


def test_repeats_aat(tool):
    """C = A * A^T, A rectangular with repeats and B = mhs_transpose(A) left on the device: exact against the oracle."""
    p, c, v = random_csr(900, 2500, 7, seed=2500)
    twin, counts = with_repeats((900, 2500, p, c, v), 43)
    assert present(counts) >= set("abcdefi"), counts
    A = csr_of(twin)
    oM, oN, op, oc, ov = orc.transpose(A.M, A.N, A.ptr, A.col, A.val)
    Cp, Ci, Cv = orc.spgemm(A.ptr, A.col, A.val, op, oc, ov, oN)
    _, _, s = expand(A.ptr, A.col, op, oc, Cp, Ci, oN)
    assert 9 * int(np.bincount(s).max()) < 2 ** 24 and repeat_kinds((oM, oN, op, oc, ov))["repeated_entries"] > 0
    A.H2D(tool.device)
    B = None
    try:
        B = mhspgemm.transpose(tool, A)
        C, tm = mhspgemm.spgemm(tool, A, B)
        try:
            gp, gc, gv = C.to_host()
        finally:
            C.release()
    finally:
        if B is not None:
            B.d_release_csr()
        A.d_release_csr()
    assert np.array_equal(gp, Cp) and np.array_equal(gc, Ci) and np.array_equal(gv, Cv)
    assert tm.nnzC == Cp[-1] > 0 and tm.flop == orc.flop(A.col, op)


# ------------------------------------------------------------------ the driver ---
CLI = Path(__file__).resolve().parent.parent / "mh-spgemm_amd" / "bin" / "spgemm"


def test_repeats_cli_check(tmp_path):
    """A .mtx with repeated lines (the reader keeps them and sorts each row) through every mode of the driver:
    --reuse, --masked, --grad, --f32, --batch with --check; the driver's own checks pass."""
    p, c, v = random_csr(400, 400, 6, seed=77)
    twin, counts = with_repeats((400, 400, p, c, v), 47)
    assert present(counts) >= set("abcdefi"), counts
    K, N, tp, tc, tv = twin
    rows = np.repeat(np.arange(K), np.diff(tp))
    order = np.random.default_rng(1).permutation(len(tc))  # (any line order: the reader sorts the rows)
    mtx = tmp_path / "repeats.mtx"
    with open(mtx, "w") as f:
        f.write(f"%%MatrixMarket matrix coordinate real general\n% repeated lines\n{K} {N} {len(tc)}\n")
        for j in order:
            f.write(f"{rows[j] + 1} {tc[j] + 1} {tv[j]:.1f}\n")
    R = mhspgemm.CSR()
    assert mhspgemm.readMtxFile(R, str(mtx)) == 0
    assert R.nnz == len(tc) and np.array_equal(R.ptr, tp) and np.array_equal(R.col, tc), "the reader keeps the repeats"
    assert len(split_repeats((K, N, R.ptr, R.col, R.val))[1]) < R.nnz
    r = subprocess.run([str(CLI), "--reuse", "2", "--masked", "2", "--grad", "2", "--f32", "--batch", "3", "--width", "2",
                        "--check", str(mtx)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    for tag in ("", "values ", "masked ", "grad ", "values f32 ", "masked f32 ", "grad f32 ", "batched ", "batched f32 ",
                "grad batched ", "grad batched f32 "):
        assert f"\n{tag}pass\n" in out, (tag, out)
    assert not re.search(r"error$", out, re.M), out
