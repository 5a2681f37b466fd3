"""CPU test of the FP64 rounding bound's checker (tests/_util.py: exact_forward, exact_grad, assert_f64_bound).

The bound of every FP64 value path is 1.01 * m * 2^-53 * S per entry (m kept products, S their absolute sum).
A test of that kind is worth something only if (1) the references themselves -- the oracle's product and the
float64 ref_grad -- stay inside it, so the tolerance can be met, and (2) the checker fails on the slips it is
there for: a value, a cotangent or a product that went through float32, a dropped product, a value written
where no product lands.  (3) records the gap the bound closes: the float32 slips all pass the older rule,
1e-6 of the same sum on absolute values.  bin_zoo and tiny_zoo(7), with the narrow values of new_values and
the wide ones of wide_values."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from _util import (assert_f64_bound, bin_zoo, csr_of, exact_forward, exact_grad, expand, new_values, ref_grad, seg_sum_ld,
                   tiny_zoo, wide_values)

ZOOS = ("bin_zoo", "tiny_zoo")
FAMILIES = ("narrow", "wide")


def f32(v):
    return np.asarray(v, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(zoo, family):
    """Operands, values of the family, the product's pattern, its kept products and the three exact references."""
    At, Bt = bin_zoo() if zoo == "bin_zoo" else tiny_zoo(7)
    A, B = csr_of(At), csr_of(Bt)
    Cp, Ci, _ = orc.spgemm(A.ptr, A.col, np.ones(A.nnz), B.ptr, B.col, np.ones(B.nnz), B.N)
    values = (lambda n, seed: new_values(n, seed, signed=True)) if family == "narrow" else wide_values
    av, bv, G = values(A.nnz, 3), values(B.nnz, 1003), values(len(Ci), 2003)
    pqs = expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)
    assert len(pqs[0]) == orc.flop(A.col, B.ptr)
    fwd = exact_forward(A, B, Cp, Ci, av, bv)
    gA, gB = exact_grad(pqs, av, bv, G, A.nnz, B.nnz)
    return A, B, Cp, Ci, av, bv, G, pqs, fwd, gA, gB


def old_rule(got, ref_ld, S):
    """The signed rule of assert_values / assert_grad: 1e-6 of the sum on absolute values."""
    return bool(np.all(np.abs(got - ref_ld.astype(np.float64)) <= 1e-6 * S.astype(np.float64) + 1e-300))


def product_of(A, B, av, bv):
    return orc.spgemm(A.ptr, A.col, av, B.ptr, B.col, bv, B.N)[2]


def test_seg_sum_keeps_long_double():
    # 1 + 2^-60 + 2^-60 needs 62 bits: a sum through float64 loses both small terms
    w = np.array([1.0, 2.0 ** -60, 2.0 ** -60, 3.0], np.longdouble)
    out = seg_sum_ld(np.array([2, 0, 2, 0]), w, 4)
    assert out.dtype == np.longdouble and out[1] == 0 and out[3] == 0
    assert out[2] - np.longdouble(1.0) == np.longdouble(2.0 ** -60)
    assert out[0] - np.longdouble(3.0) == np.longdouble(2.0 ** -60)
    assert seg_sum_ld(np.zeros(0, np.int64), np.zeros(0), 3).tolist() == [0, 0, 0]


def test_wide_values_are_wide_and_normal():
    v = wide_values(100_000, 5)
    a = np.abs(v)
    assert a.min() >= 2.0 ** -21 and a.max() < 2.0 ** 20 and (v < 0).any() and (v > 0).any()
    _, e = np.frexp(a)
    assert set(e.tolist()) == set(range(-20, 21)), "every binade of 2^[-20, 20] * [0.5, 1)"
    assert np.count_nonzero(f32(v) != v) > 0.99 * len(v), "mantissas past float32's 24 bits"


# 1. the references alone stay inside the bound
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("zoo", ZOOS)
def test_references_meet_the_bound(zoo, family):
    A, B, Cp, Ci, av, bv, G, pqs, fwd, gA, gB = case(zoo, family)
    assert fwd[1].min() >= 1, "the pattern is the product's own"
    assert zoo != "bin_zoo" or fwd[1].max() == 3000, "the row of 3000 repeated A entries: sums of 3000 products"
    assert_f64_bound(product_of(A, B, av, bv), *fwd, "the oracle's product")
    wA, wB = ref_grad(pqs, av, bv, G, A.nnz, B.nnz)
    assert_f64_bound(wA, *gA, "ref_grad's dA")
    assert_f64_bound(wB, *gB, "ref_grad's dB")
    assert (gA[1] == 0).any() or zoo == "bin_zoo"  # (tiny_zoo: A entries at empty B rows, m = 0)


# 2. the checker can fail, and 3. the float32 slips pass the older rule
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("zoo", ZOOS)
def test_aval_through_float32_is_caught(zoo, family):
    A, B, Cp, Ci, av, bv, G, pqs, fwd, gA, gB = case(zoo, family)
    got = product_of(A, B, f32(av), bv)
    with pytest.raises(AssertionError, match="outside 1.01 m 2\\^-53 S"):
        assert_f64_bound(got, *fwd, "C with Aval through float32")
    assert old_rule(got, fwd[0], fwd[2]), "the gap: the 1e-6 rule accepts it"
    _, dB = ref_grad(pqs, f32(av), bv, G, A.nnz, B.nnz)
    with pytest.raises(AssertionError, match="outside 1.01 m 2\\^-53 S"):
        assert_f64_bound(dB, *gB, "dB with Aval through float32")
    assert old_rule(dB, gB[0], gB[2])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("zoo", ZOOS)
def test_cotangent_through_float32_is_caught(zoo, family):
    A, B, Cp, Ci, av, bv, G, pqs, fwd, gA, gB = case(zoo, family)
    dA, dB = ref_grad(pqs, av, bv, f32(G), A.nnz, B.nnz)
    for got, ref, what in ((dA, gA, "dA"), (dB, gB, "dB")):
        with pytest.raises(AssertionError, match="outside 1.01 m 2\\^-53 S"):
            assert_f64_bound(got, *ref, f"{what} with G through float32")
        assert old_rule(got, ref[0], ref[2]), "the gap: the 1e-6 rule accepts it"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("zoo", ZOOS)
def test_products_through_float32_are_caught(zoo, family):
    A, B, Cp, Ci, av, bv, G, pqs, fwd, gA, gB = case(zoo, family)
    p, q, s = pqs
    got = np.bincount(s, f32(av[p] * bv[q]), len(Ci))  # float32 products, a float64 sum
    with pytest.raises(AssertionError, match="outside 1.01 m 2\\^-53 S"):
        assert_f64_bound(got, *fwd, "C of float32 products")
    assert old_rule(got, fwd[0], fwd[2]), "the gap: the 1e-6 rule accepts it"
    dA = np.bincount(p, f32(bv[q] * G[s]), A.nnz)
    with pytest.raises(AssertionError, match="outside 1.01 m 2\\^-53 S"):
        assert_f64_bound(dA, *gA, "dA of float32 products")
    assert old_rule(dA, gA[0], gA[2])


@pytest.mark.parametrize("zoo", ZOOS)
def test_one_dropped_product_is_caught(zoo):
    A, B, Cp, Ci, av, bv, G, pqs, fwd, gA, gB = case(zoo, "narrow")
    p, q, s = pqs
    slot = int(np.argmax(fwd[1]))  # the entry of the most products: one of them is the smallest share of its sum
    drop = int(np.nonzero(s == slot)[0][0])
    keep = np.ones(len(s), bool)
    keep[drop] = False
    got = np.bincount(s[keep], av[p[keep]] * bv[q[keep]], len(Ci))
    with pytest.raises(AssertionError, match="1 of .* entries outside"):
        assert_f64_bound(got, *fwd, "C less one product")


@pytest.mark.parametrize("zoo", ZOOS)
def test_value_at_an_unreached_entry_is_caught(zoo):
    A, B, Cp, Ci, av, bv, G, pqs, fwd, gA, gB = case(zoo, "narrow")
    # dB: B rows that no A entry points at hold entries with m = 0 in both zoos
    ref, m, S = gB
    assert (m == 0).any()
    _, got = ref_grad(pqs, av, bv, G, A.nnz, B.nnz)
    assert_f64_bound(got, ref, m, S, "dB")
    for stray in (5e-324, -1e-30, float("nan")):
        bad = got.copy()
        bad[np.nonzero(m == 0)[0][0]] = stray
        with pytest.raises(AssertionError, match="exactly 0.0|every entry is written"):
            assert_f64_bound(bad, ref, m, S, "dB with a stray value")
    with pytest.raises(AssertionError, match="shape"):
        assert_f64_bound(got[:-1], ref, m, S, "dB, one short")
