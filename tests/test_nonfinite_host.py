"""CPU test of the non-finite contract's checker (tests/_util.py: inject_nonfinite, product_classes,
assert_nonfinite_contract) against the two references that form every product and nothing else: the oracle's
sequential product and the float64 ref_grad.

The contract (include/mhspgemm.h) is free of any order: an output entry is NaN if one of its kept products is NaN
(0 * Inf, anything times NaN) or products of both infinities occur, +Inf or -Inf if only that infinity occurs, and
otherwise finite within the rounding bound of its products.  (1) the classifier gives the class of every entry of
the oracle's C and of ref_grad's dA and dB, on the inputs the GPU tests of tests/test_gpu_nonfinite.py use, and
the references pass the whole check; (2) those inputs give what the GPU tests rely on: every class occurs and
more than half of the entries stay finite; (3) the checker fails on the slips it is there for: an explicit 0 * b
beside an Inf, a stored zero skipped, a non-finite product added to a neighbouring entry."""
import functools

import numpy as np
import pytest

from mhspgemm import synth
from oracle import oracle as orc
from _util import (FINITE, IS_NAN, NEG_INF, POS_INF, U64, assert_nonfinite_contract, bin_zoo, classes_of, csr_of, edge_val,
                   expand, group_zoo, inject_nonfinite, near_zoo, product_classes, ref_grad, run_zoo, tiny_zoo, wide_values)

EDGE_VALS = {"edge_val_team": (64, 100, 200), "edge_val_wave": (200, 1024, 1000), "edge_val_block": (3000, 19968, 4000)}
INPUTS = ["bin_zoo", "tiny_zoo", "run_zoo", "group_zoo", "near_zoo", "fem_5_5_13", "fem_5_4_9"] + list(EDGE_VALS)


@functools.lru_cache(maxsize=None)
def case(name):
    """Operands (B is A for the FEM grids), injected values, the product's pattern and its kept products."""
    if name.startswith("fem"):
        F = synth.fem_grid(5, 5, 13, 3, seed=5) if name == "fem_5_5_13" else synth.fem_grid(5, 4, 9, dof=3)
        A = B = F
    elif name in EDGE_VALS:
        A, B = (csr_of(t) for t in edge_val(*EDGE_VALS[name]))
    else:
        A, B = (csr_of(t) for t in {"bin_zoo": bin_zoo, "tiny_zoo": lambda: tiny_zoo(7), "run_zoo": lambda: run_zoo(5),
                                    "group_zoo": lambda: group_zoo(3), "near_zoo": near_zoo}[name]())
    if name in EDGE_VALS:  # (its own integer values, as the GPU test of the class edges keeps them)
        av, bv = inject_nonfinite(A.val, 5), inject_nonfinite(B.val, 6)
    else:
        av = inject_nonfinite(wide_values(A.nnz, 17), 5)
        bv = av if B is A else inject_nonfinite(wide_values(B.nnz, 1017), 6)
    Cp, Ci, Cv = orc.spgemm(A.ptr, A.col, av, B.ptr, B.col, bv, B.N)
    pqs = expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)
    assert len(pqs[0]) == orc.flop(A.col, B.ptr)
    return A, B, av, bv, Cp, Ci, Cv, pqs


def test_inject_nonfinite():
    v = np.arange(1.0, 3001.0)
    w = inject_nonfinite(v, 5)
    k = int(0.004 * 3000)
    changed = np.nonzero(~(w == v))[0]
    assert len(changed) == k == 12 and v[0] == 1.0, "a copy, k = max(least, int(rate * n)) distinct positions"
    assert np.array_equal(np.sort(changed), np.sort(np.random.default_rng(5).choice(3000, k, replace=False)))
    assert [int(np.count_nonzero(classes_of(w) == c)) for c in (POS_INF, NEG_INF, IS_NAN)] == [3, 3, 3]
    assert np.count_nonzero(w == 0.0) == 3
    w = inject_nonfinite(v[:100], 6, zeros=False)
    assert np.count_nonzero(w == 0.0) == 0 and np.count_nonzero(~np.isfinite(w)) == 6, "least = 6, no zeros"
    assert np.array_equal(inject_nonfinite(v, 5), inject_nonfinite(v, 5), equal_nan=True)


def test_product_classes_by_hand():
    inf, nan = np.inf, np.nan
    #        slot: 0 finite   1 +Inf     2 -Inf      3 Inf - Inf      4 0 * Inf  5 NaN     6 none  7 two -Inf
    idx = np.array([0, 0,     1, 1,      2,          3, 3,            4, 4,      5,        7, 7])
    x = np.array([1.0, -2.0,  inf, 3.0,  -inf,       inf, -inf,       0.0, 1.0,  nan,      -inf, 2.0])
    y = np.array([3.0, 4.0,   2.0, 5.0,  0.5,        1.0, 1.0,        inf, 1.0,  0.0,      1.0, -inf])
    assert product_classes(idx, x, y, 8).tolist() == [FINITE, POS_INF, NEG_INF, IS_NAN, IS_NAN, IS_NAN, FINITE, NEG_INF]
    assert product_classes(idx[:0], x[:0], y[:0], 3).tolist() == [FINITE] * 3
    assert classes_of([1.0, inf, -inf, nan, 0.0]).tolist() == [FINITE, POS_INF, NEG_INF, IS_NAN, FINITE]


# 1. the classifier is the references' own behaviour, and 2. the inputs give what the GPU tests rely on
@pytest.mark.parametrize("name", INPUTS)
def test_references_hold_the_contract(name):
    A, B, av, bv, Cp, Ci, Cv, (p, q, s) = case(name)
    nC = len(Ci)
    want = assert_nonfinite_contract(Cv, s, av[p], bv[q], nC, U64, f"{name}: the oracle's product")
    assert np.array_equal(want, classes_of(Cv))
    for c in (FINITE, POS_INF, NEG_INF, IS_NAN):
        assert (want == c).any(), f"class {c} does not occur in C"
    share = np.count_nonzero(want == FINITE) / nC
    print(f"{name}: finite share of C {share:.3f}")
    assert share > 0.5
    if name == "bin_zoo":
        rows = np.repeat(np.arange(A.M), np.diff(Cp))
        fin_rows = np.bincount(rows[want == FINITE], minlength=A.M) > 0
        bad_rows = np.bincount(rows[want != FINITE], minlength=A.M) > 0
        assert np.count_nonzero(fin_rows & bad_rows) > 50, "rows that hold both finite and non-finite entries"
    G = wide_values(nC, 2017) if name not in EDGE_VALS else np.where(np.arange(nC) % 2, 2.0, -3.0)
    wA, wB = ref_grad((p, q, s), av, bv, G, A.nnz, B.nnz)
    for got, idx, x, y, n, what in ((wA, p, bv[q], G[s], A.nnz, "dA"), (wB, q, av[p], G[s], B.nnz, "dB")):
        cls = assert_nonfinite_contract(got, idx, x, y, n, U64, f"{name}: ref_grad's {what}")
        assert np.array_equal(cls, classes_of(got))
        assert (cls == FINITE).any() and (cls != FINITE).any()
        assert name in EDGE_VALS or np.count_nonzero(cls == FINITE) > n // 2  # (edge_val: an A row of a few entries)


# 3. the checker fails on the slips it is there for
def slip_case():
    A, B, av, bv, Cp, Ci, Cv, (p, q, s) = case("tiny_zoo")
    with np.errstate(invalid="ignore"):
        w = av[p] * bv[q]
    return av, bv, Ci, Cv, p, q, s, w


def test_an_explicit_zero_product_is_caught():
    """Padding as 0 * b: a NaN where the contract has an infinity or a number."""
    av, bv, Ci, Cv, p, q, s, w = slip_case()
    cls = classes_of(Cv)
    for c in (POS_INF, NEG_INF, FINITE):
        bad = Cv.copy()
        bad[np.nonzero(cls == c)[0][0]] += 0.0 * np.inf if c != FINITE else np.nan
        with pytest.raises(AssertionError, match="in another class than their products'.*-> NaN"):
            assert_nonfinite_contract(bad, s, av[p], bv[q], len(Ci), U64, "C with one padded product")


def test_a_skipped_stored_zero_is_caught():
    """A product skipped because one factor is 0: a number where the contract has the NaN of 0 * Inf."""
    av, bv, Ci, Cv, p, q, s, w = slip_case()
    zero_inf = np.isnan(w) & ((av[p] == 0.0) | (bv[q] == 0.0))
    assert zero_inf.any(), "the case holds a stored zero against an infinity"
    keep = ~zero_inf
    with np.errstate(invalid="ignore"):
        got = np.bincount(s[keep], w[keep], len(Ci))
    assert np.count_nonzero(classes_of(got) != classes_of(Cv)) > 0
    with pytest.raises(AssertionError, match="in another class than their products'.*NaN -> "):
        assert_nonfinite_contract(got, s, av[p], bv[q], len(Ci), U64, "C with zero factors skipped")


def test_a_leak_into_a_neighbour_is_caught():
    """A non-finite product added to the entry next to its own, and a finite one (the bound catches that)."""
    av, bv, Ci, Cv, p, q, s, w = slip_case()
    cls = classes_of(Cv)
    at = np.nonzero((cls[:-1] != FINITE) & (cls[1:] == FINITE))[0][0]
    bad = Cv.copy()
    bad[at + 1] += Cv[at]
    with pytest.raises(AssertionError, match="in another class than their products'.*finite -> "):
        assert_nonfinite_contract(bad, s, av[p], bv[q], len(Ci), U64, "C with a leaked non-finite product")
    at = np.nonzero((cls[:-1] == FINITE) & (cls[1:] == FINITE) & (Cv[:-1] != 0))[0][0]
    bad = Cv.copy()
    bad[at + 1] += Cv[at]
    with pytest.raises(AssertionError, match="finite entries outside 1.01 m u S"):
        assert_nonfinite_contract(bad, s, av[p], bv[q], len(Ci), U64, "C with a leaked finite product")
    bad = Cv.copy()
    bad[np.nonzero(cls == IS_NAN)[0][0]] = 1.0
    with pytest.raises(AssertionError, match="NaN -> finite"):
        assert_nonfinite_contract(bad, s, av[p], bv[q], len(Ci), U64, "C with a NaN lost")
