"""GPU tests of the semiring values plans (mhspgemm.ValuesPlan(semiring=...) over mhs_values_plan_create_semiring):
min-plus, max-plus and max-min on a kept pattern or a mask, in every row class, FP64 and FP32.

min and max are exact and do not depend on order, and the one rounding of a + b does not either, so every result is
bit-identical to a sequential evaluation: the checks are equalities (np.array_equal; numeric equality equates +0 and
-0, the one exemption of the contract).  The reference is numpy: _util.expand gives the kept products (A entry p, B
entry q, C slot s); an array of the identity is reduced with np.minimum.at / np.maximum.at over av[p] + bv[q] or
np.minimum(av[p], bv[q]) in the plan's dtype (FP32: the inputs rounded to float32 first, the add in float32).
Values are signed with magnitudes in [0.1, 1000]: no subnormals, no overflow.  Every output buffer starts as NaN."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mhspgemm
from mhspgemm import _lib
from oracle import oracle as orc
from _util import (GOLDEN, PRODUCT_CASES, assert_f64_bound, bin_zoo, csr_of, device_csr, exact_forward, expand, filled, keys,
                   load_golden, many_a_entries, random_csr, tiny_zoo)

pytestmark = pytest.mark.gpu

TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL, DOT = 1, 2, 3, 4, 5, 6, 7
SEMIRINGS = ("min_plus", "max_plus", "max_min")
IDENTITY = {"min_plus": np.inf, "max_plus": -np.inf, "max_min": -np.inf}
NP = {"float64": np.float64, "float32": np.float32}


def sr_values(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.1, 1000.0, n) * rng.choice([-1.0, 1.0], n)


def reference(sr, pqs, av, bv, nnzC, dtype="float64", skip=None):
    """The sequential reduce of the kept products pqs in `dtype`; skip: a mask over the products left out."""
    p, q, s = pqs
    if skip is not None:
        p, q, s = p[~skip], q[~skip], s[~skip]
    a, b = av.astype(NP[dtype]), bv.astype(NP[dtype])
    prod = np.minimum(a[p], b[q]) if sr == "max_min" else a[p] + b[q]
    assert prod.dtype == NP[dtype]
    out = np.full(nnzC, IDENTITY[sr], NP[dtype])
    (np.minimum if sr == "min_plus" else np.maximum).at(out, s, prod)
    return out


def dev(tool, v, dtype="float64"):
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=NP[dtype])).to(f"cuda:{tool.device}")
    torch.cuda.synchronize()
    return t


def nan_filled(tool, n, dtype="float64"):
    if dtype == "float64":
        return filled(tool, n)
    out = torch.full((n,), float("nan"), dtype=torch.float32, device=f"cuda:{tool.device}")
    torch.cuda.synchronize()
    return out


def run_plan(tool, A, B, C, sr, av, bv, dtype="float64", masked=False, form="auto", calls=1, between=None):
    """A plan of `sr` on device-resident A, B and the pattern C; `calls` calls into NaN-filled outputs, with
    between() -- other work on the plan's context -- ahead of every call after the first.
    Returns (the values of each call, info())."""
    plan = mhspgemm.ValuesPlan(tool, A, B, C, masked=masked, form=form, dtype=dtype, semiring=sr)
    try:
        assert plan.semiring == sr
        info = plan.info()
        dA, dB = dev(tool, av, dtype), dev(tool, bv, dtype)
        got = []
        for k in range(calls):
            if k and between is not None:
                between()
                assert plan.info() == info, "the plan after other work on its context"
            out = nan_filled(tool, C.nnz, dtype)
            assert plan.run(dA, dB, out=out) is None
            torch.cuda.synchronize()
            got.append(out.cpu().numpy())
    finally:
        plan.close()
    assert info["semiring"] == sr and info["width"] == 1 and info["dtype"] == dtype
    return got, info


def plus_times_info(tool, A, B, C, dtype="float64", masked=False, form="auto"):
    plan = mhspgemm.ValuesPlan(tool, A, B, C, masked=masked, form=form, dtype=dtype)
    try:
        return plan.info()
    finally:
        plan.close()


def same_classes(info, base):
    """info() of a semiring plan against the plus-times plan's on the same patterns and dtype: all but the name."""
    return {k: v for k, v in info.items() if k != "semiring"} == {k: v for k, v in base.items() if k != "semiring"}


@functools.lru_cache(maxsize=None)
def case(name):
    """Host operands, the product's pattern and the kept products of a golden case or a zoo, computed once."""
    if name in ("bin_zoo", "tiny_zoo"):
        At, Bt = bin_zoo() if name == "bin_zoo" else tiny_zoo(7)
        A, B = csr_of(At), csr_of(Bt)
    else:
        d, _, _, _ = load_golden(name)
        A = mhspgemm.CSR()
        assert mhspgemm.readMtxFile(A, str(GOLDEN / d["A"])) == 0
        B = A
        if d["B"]:
            B = mhspgemm.CSR()
            assert mhspgemm.readMtxFile(B, str(GOLDEN / d["B"])) == 0
    Cp, Ci, _ = orc.spgemm(A.ptr, A.col, A.val, B.ptr, B.col, B.val, B.N)
    pqs = expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)
    return A, B, Cp, Ci, pqs


def on_device(tool, A, B, Cp, Ci):
    dA = device_csr(tool, A.M, A.N, A.ptr, A.col, A.val)
    dB = dA if B is A else device_csr(tool, B.M, B.N, B.ptr, B.col, B.val)
    return dA, dB, device_csr(tool, A.M, B.N, Cp, Ci)


# 1. golden products: empty product, duplicates in A / B, rectangular, dense row and column, tile edges
@pytest.mark.parametrize("sr", SEMIRINGS)
@pytest.mark.parametrize("name", PRODUCT_CASES)
def test_semiring_golden_products(tool, name, sr):
    A, B, Cp, Ci, pqs = case(name)
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    av, bv = sr_values(A.nnz, 1), sr_values(B.nnz, 1001)
    if B is A:
        bv = av
    (got,), info = run_plan(tool, dA, dB, dC, sr, av, bv)
    assert np.array_equal(got, reference(sr, pqs, av, bv, len(Ci)))
    assert info["nnzC"] == len(Ci) and info["products"] == info["kept_products"] == len(pqs[0])
    if name == "duplicates":  # every duplicate is a product of its own, reduced by min / max: not summed
        plain = mhspgemm.ValuesPlan(tool, dA, dB, dC)
        try:
            out = filled(tool, dC.nnz)
            plain.run(dev(tool, av), dev(tool, bv), out=out)
            torch.cuda.synchronize()
        finally:
            plain.close()
        assert len(Ci) > 0 and not np.array_equal(got, out.cpu().numpy())


# 2. the zoos: every class between them, both types; classes are the plus-times plan's
@pytest.mark.parametrize("sr", SEMIRINGS)
@pytest.mark.parametrize("dtype", ("float64", "float32"))
@pytest.mark.parametrize("name", ("bin_zoo", "tiny_zoo"))
def test_semiring_zoos(tool, name, dtype, sr):
    A, B, Cp, Ci, pqs = case(name)
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    av, bv = sr_values(A.nnz, 3), sr_values(B.nnz, 1003)
    (got,), info = run_plan(tool, dA, dB, dC, sr, av, bv, dtype)
    assert got.dtype == NP[dtype] and np.array_equal(got, reference(sr, pqs, av, bv, len(Ci), dtype))
    assert same_classes(info, plus_times_info(tool, dA, dB, dC, dtype)), "classes do not depend on the semiring"
    if name == "bin_zoo":
        assert info["rows"][GLOBAL] >= 1, info  # (FP32 too: the 20,000-entry scattered rows are past a block's 19,968)


def test_semiring_every_class_has_rows(tool):
    rows = np.zeros(8, np.int64)
    for name in ("bin_zoo", "tiny_zoo"):
        A, B, Cp, Ci, _ = case(name)
        dA, dB, dC = on_device(tool, A, B, Cp, Ci)
        plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, semiring="min_plus")
        try:
            rows += plan.info()["rows"]
        finally:
            plan.close()
    for cls in (TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL):
        assert rows[cls] > 0, f"class {cls} has no rows in bin_zoo + tiny_zoo"
    assert rows[DOT] == 0


# 3. stage boundaries: wave rows whose A entries need more than one stage (64 entries a stage, 256 in a block)
@pytest.mark.parametrize("sr", SEMIRINGS)
def test_semiring_stage_boundaries(tool, sr):
    A, B, Cp, Ci, pqs = many_a_entries()
    assert sorted(np.diff(A.ptr)) == [65, 65, 100, 100, 150, 150, 257, 257, 300, 300, 700]
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    av, bv = sr_values(A.nnz, 9), sr_values(B.nnz, 1009)
    (got,), info = run_plan(tool, dA, dB, dC, sr, av, bv)
    assert info["rows"][WAVE_DIRECT] >= 5 and info["rows"][WAVE_SEARCH] >= 1 and info["rows"][BLOCK_DIRECT] >= 3, info
    assert np.array_equal(got, reference(sr, pqs, av, bv, len(Ci)))


# 4. C's pattern a strict superset of the product's: extra entries in some rows and one extra whole row
@functools.lru_cache(maxsize=None)
def superset_case():
    M, K, N, EMPTY = 600, 500, 8000, 7
    p, c, v = random_csr(M, K, 6, 5)
    rows = np.repeat(np.arange(M), np.diff(p))
    keep = rows != EMPTY  # A's row 7 emptied: its product row is empty
    p2 = np.zeros(M + 1, np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=M), out=p2[1:])
    A = mhspgemm.CSR(M, K, p2.astype(np.int32), c[keep], v[keep])
    Bp, Bc, Bv = random_csr(K, N, 9, 6)
    B = mhspgemm.CSR(K, N, Bp, Bc, Bv)
    Pp, Pi, _ = orc.spgemm(A.ptr, A.col, A.val, B.ptr, B.col, B.val, N)
    rng = np.random.default_rng(8)
    extra = np.concatenate([i * N + rng.choice(N, 3, replace=False) for i in range(0, M, 5)] +
                           [EMPTY * N + rng.choice(N, 40, replace=False)]).astype(np.int64)
    kP = keys(Pp, Pi, N)
    key = np.union1d(kP, extra)
    Cp = np.zeros(M + 1, np.int64)
    np.cumsum(np.bincount(key // N, minlength=M), out=Cp[1:])
    Cp, Ci = Cp.astype(np.int32), (key % N).astype(np.int32)
    is_extra = ~np.isin(key, kP)
    assert Pp[EMPTY + 1] == Pp[EMPTY] and Cp[EMPTY + 1] - Cp[EMPTY] == 40 and is_extra.sum() >= 300
    return A, B, Cp, Ci, expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, N), is_extra


@pytest.mark.parametrize("dtype", ("float64", "float32"))
def test_semiring_superset_pattern(tool, dtype):
    A, B, Cp, Ci, pqs, is_extra = superset_case()
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    av, bv = sr_values(A.nnz, 15), sr_values(B.nnz, 1015)
    for sr in SEMIRINGS:
        (got,), _ = run_plan(tool, dA, dB, dC, sr, av, bv, dtype)
        assert np.all(got[is_extra] == IDENTITY[sr]), "entries no product reaches get exactly the identity"
        assert np.isfinite(got[~is_extra]).all()
        assert np.array_equal(got, reference(sr, pqs, av, bv, len(Ci), dtype))


# 5. masked plans, every form, on three masks
def thinned_mask_with_strangers(Cp, Ci, N, seed=77):
    """Every second entry of the pattern, every 50th row emptied, and per row up to 2 columns the pattern lacks."""
    M = len(Cp) - 1
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(Cp))
    keep = (np.arange(len(Ci)) % 2 == 0) & (rows % 50 != 0)
    rng = np.random.default_rng(seed)
    srow = np.repeat(np.arange(M, dtype=np.int64), 2)
    srow = srow[srow % 50 != 0]
    skey = np.setdiff1d(srow * N + rng.integers(0, N, len(srow)), keys(Cp, Ci, N))  # strangers: not in the product
    key = np.union1d(rows[keep] * N + Ci[keep], skey)
    Mp = np.zeros(M + 1, np.int64)
    np.cumsum(np.bincount(key // N, minlength=M), out=Mp[1:])
    return Mp.astype(np.int32), (key % N).astype(np.int32)


@functools.lru_cache(maxsize=None)
def mask_case(name):
    """(A, B, mask ptr, mask col, kept products).  rect: a random rectangular pair, the mask a random subset of the
    product's pattern plus entries outside it; triangle: L*L on L of a few thousand rows; long_rows: mask rows of
    more than 64 entries (a dot row takes them 64 at a time and stages its A entries again) and A rows past 64."""
    if name == "rect":
        p, c, v = random_csr(1500, 1000, 7, 5)
        Bp, Bc, Bv = random_csr(1000, 20_000, 10, 6)
        A, B = mhspgemm.CSR(1500, 1000, p, c, v), mhspgemm.CSR(1000, 20_000, Bp, Bc, Bv)
        Cp, Ci, _ = orc.spgemm(p, c, v, Bp, Bc, Bv, B.N)
        Mp, Mc = thinned_mask_with_strangers(Cp, Ci, B.N)
    elif name == "triangle":
        n = 3000
        rng = np.random.default_rng(5)
        pairs = rng.integers(0, n, (24_000, 2))
        pairs = pairs[pairs[:, 0] != pairs[:, 1]]
        lower = np.unique(np.maximum(pairs[:, 0], pairs[:, 1]).astype(np.int64) * n + np.minimum(pairs[:, 0], pairs[:, 1]))
        ptr = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(lower // n, minlength=n), out=ptr[1:])
        A = B = mhspgemm.CSR(n, n, ptr.astype(np.int32), (lower % n).astype(np.int32), np.ones(len(lower)))
        Mp, Mc = A.ptr, A.col
    else:
        rng = np.random.default_rng(66)
        K, N = 400, 2500
        Bp, Bc, Bv = random_csr(K, N, 9, 67)
        arows = [np.sort(rng.choice(K, na, replace=False)) for na in (1, 63, 64, 65, 130, 200) * 4]
        mrows = [np.sort(rng.choice(N, nm, replace=False)) for nm in (300, 65, 64, 1, 129, 70) * 4]
        Ap = np.zeros(len(arows) + 1, np.int64)
        Ap[1:] = np.cumsum([len(r) for r in arows])
        Mp = np.zeros(len(mrows) + 1, np.int64)
        Mp[1:] = np.cumsum([len(r) for r in mrows])
        A = mhspgemm.CSR(len(arows), K, Ap.astype(np.int32), np.concatenate(arows).astype(np.int32), np.ones(int(Ap[-1])))
        B = mhspgemm.CSR(K, N, Bp, Bc, Bv)
        Mp, Mc = Mp.astype(np.int32), np.concatenate(mrows).astype(np.int32)
    return A, B, Mp, Mc, expand(A.ptr, A.col, B.ptr, B.col, Mp, Mc, B.N)


@pytest.mark.parametrize("form", ("product", "dot", "auto"))
@pytest.mark.parametrize("name", ("rect", "triangle", "long_rows"))
def test_semiring_masked(tool, name, form):
    A, B, Mp, Mc, pqs = mask_case(name)
    dA, dB, dC = on_device(tool, A, B, Mp, Mc)
    av, bv = sr_values(A.nnz, 21), sr_values(B.nnz, 1021)
    if B is A:
        bv = av
    reached = np.zeros(len(Mc), bool)
    reached[pqs[2]] = True
    assert reached.any() and not reached.all(), "the case needs mask entries no product reaches"
    assert len(pqs[0]) < orc.flop(A.col, B.ptr), "the case needs products outside the mask"
    base = plus_times_info(tool, dA, dB, dC, masked=True, form=form)
    assert base["kept_products"] == len(pqs[0])
    for sr in SEMIRINGS:
        (got,), info = run_plan(tool, dA, dB, dC, sr, av, bv, masked=True, form=form)
        assert np.array_equal(got, reference(sr, pqs, av, bv, len(Mc))), (sr, form)
        assert np.all(got[~reached] == IDENTITY[sr]) and np.isfinite(got[reached]).all()
        assert info["kept_products"] == base["kept_products"] and same_classes(info, base)
        if form == "dot":
            assert info["rows"][DOT] == np.count_nonzero((np.diff(Mp) > 0) & (np.diff(A.ptr) > 0)) > 0
            assert sum(info["rows"][1:7]) == np.count_nonzero((np.diff(Mp) > 0) & (np.diff(A.ptr) == 0))
        if form == "product":
            assert info["rows"][DOT] == 0


# 6. two calls give identical bytes (entries that are +0 or -0 apart: the sign of a zero is unspecified)
@pytest.mark.parametrize("sr", SEMIRINGS)
@pytest.mark.parametrize("name", ("bin_zoo", "tiny_zoo"))
def test_semiring_two_calls_same_bytes(tool, name, sr):
    A, B, Cp, Ci, _ = case(name)
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    (g1, g2), _ = run_plan(tool, dA, dB, dC, sr, sr_values(A.nnz, 4), sr_values(B.nnz, 1004), calls=2)
    nz = (g1 != 0) | (g2 != 0)
    assert g1[nz].tobytes() == g2[nz].tobytes() and not np.isnan(g1).any()


@functools.lru_cache(maxsize=None)
def small_pair():
    p, c, v = random_csr(800, 600, 6, 31)
    Bp, Bc, Bv = random_csr(600, 3000, 8, 32)
    A, B = mhspgemm.CSR(800, 600, p, c, v), mhspgemm.CSR(600, 3000, Bp, Bc, Bv)
    Cp, Ci, _ = orc.spgemm(p, c, v, Bp, Bc, Bv, B.N)
    return A, B, Cp, Ci, expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)


# 7. infinities are ordinary values: +Inf is "no edge" under min-plus
def test_semiring_min_plus_infinities(tool):
    A, B, Cp, Ci, pqs = small_pair()
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    av, bv = sr_values(A.nnz, 41), sr_values(B.nnz, 1041)
    bv[np.random.default_rng(42).random(B.nnz) < 0.1] = np.inf
    row = int(np.argmax(np.diff(A.ptr) >= 3))  # a row all of whose products are +Inf
    for k in A.col[A.ptr[row]:A.ptr[row + 1]]:
        bv[B.ptr[k]:B.ptr[k + 1]] = np.inf
    (got,), _ = run_plan(tool, dA, dB, dC, "min_plus", av, bv)
    want = reference("min_plus", pqs, av, bv, len(Ci))
    assert np.array_equal(got, want) and not np.isnan(got).any()
    assert Cp[row + 1] > Cp[row] and np.all(got[Cp[row]:Cp[row + 1]] == np.inf)
    assert np.isinf(want).sum() > Cp[row + 1] - Cp[row] and np.isfinite(want).sum() > 0.5 * len(want)


# 8. NaN containment: one A value NaN reaches only the entries it has a product in
@pytest.mark.parametrize("sr", SEMIRINGS)
def test_semiring_nan_containment(tool, sr):
    A, B, Cp, Ci, pqs = small_pair()
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    av, bv = sr_values(A.nnz, 51), sr_values(B.nnz, 1051)
    p0 = int(A.ptr[int(np.argmax(np.diff(A.ptr) >= 4))] + 1)
    av[p0] = np.nan
    uses = pqs[0] == p0
    touched = np.zeros(len(Ci), bool)
    touched[pqs[2][uses]] = True
    assert 0 < touched.sum() < 0.1 * len(Ci)
    rest = reference(sr, pqs, av, bv, len(Ci), skip=uses)  # the reduce of the other products
    (got,), _ = run_plan(tool, dA, dB, dC, sr, av, bv)
    assert np.array_equal(got[~touched], rest[~touched]), "a NaN product reaches no other entry"
    assert np.all(np.isnan(got[touched]) | (got[touched] == rest[touched])), "such an entry: NaN or its other products"


# 9. batched calls on a semiring plan: nb runs, padding between strided sets keeps its bytes, B shared by stride 0
def test_semiring_batched(tool):
    A, B, Cp, Ci, pqs = small_pair()
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    nb, pad = 3, 5
    avs = np.stack([sr_values(A.nnz, 60 + b) for b in range(nb)])
    bvs = np.stack([sr_values(B.nnz, 1060 + b) for b in range(nb)])

    def strided(v, n):  # [nb, n] at a row stride of n + pad, NaN between the sets
        buf = torch.full((nb, n + pad), float("nan"), dtype=torch.float64, device=f"cuda:{tool.device}")
        if v is not None:
            buf[:, :n] = torch.from_numpy(v).to(buf.device)
        torch.cuda.synchronize()
        return buf, buf[:, :n]

    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, semiring="min_plus")
    try:
        (_, Av), (_, Bv), (obuf, out) = strided(avs, A.nnz), strided(bvs, B.nnz), strided(None, len(Ci))
        assert Av.stride(0) == A.nnz + pad and out.stride(0) == len(Ci) + pad
        before = obuf.cpu().numpy().view(np.int64).copy()
        plan.run_batched(Av, Bv, out=out)
        torch.cuda.synchronize()
        after = obuf.cpu().numpy()
        for b in range(nb):
            assert np.array_equal(after[b, :len(Ci)], reference("min_plus", pqs, avs[b], bvs[b], len(Ci))), b
        assert np.array_equal(after.view(np.int64)[:, len(Ci):], before[:, len(Ci):]), "padding bytes are untouched"
        shared = dev(tool, bvs[0])  # one B for every set: stride 0
        (obuf, out) = strided(None, len(Ci))
        plan.run_batched(Av, shared, out=out)
        torch.cuda.synchronize()
        after = obuf.cpu().numpy()
        for b in range(nb):
            assert np.array_equal(after[b, :len(Ci)], reference("min_plus", pqs, avs[b], bvs[0], len(Ci))), b
        assert np.isnan(after[:, len(Ci):]).all()
    finally:
        plan.close()


# 10. mhs_values_plan_create_semiring with MHS_SR_PLUS_TIMES is mhs_values_plan_create_typed
def test_semiring_plus_times_is_the_typed_plan(tool):
    A, B, Cp, Ci, pqs = small_pair()
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    L = _lib.lib()
    ref = mhspgemm.ValuesPlan(tool, dA, dB, dC)
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC)
    try:
        L.mhs_values_plan_destroy(tool.ctx, plan.plan)  # the same object around a plan of the new entry point
        plan.plan = ctypes.c_void_p()
        a, b = dA.c_view(), dB.c_view()
        rc = L.mhs_values_plan_create_semiring(tool.ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(plan._c), 0, 0,
                                               _lib.MHS_F64, _lib.MHS_SR_PLUS_TIMES, ctypes.byref(plan.plan))
        assert rc == 0 and plan.plan.value
        assert plan.info() == ref.info() and plan.info()["semiring"] == "plus_times"
        av, bv = sr_values(A.nnz, 71), sr_values(B.nnz, 1071)
        out = filled(tool, len(Ci))
        plan.run(dev(tool, av), dev(tool, bv), out=out)
        torch.cuda.synchronize()
        assert_f64_bound(out.cpu().numpy(), *exact_forward(A, B, Cp, Ci, av, bv), "create_semiring(PLUS_TIMES), C")
        G = dev(tool, sr_values(len(Ci), 72))
        gA, gB = plan.grad(G, dev(tool, av), dev(tool, bv))
        rA, rB = ref.grad(G, dev(tool, av), dev(tool, bv))
        torch.cuda.synchronize()
        assert torch.equal(gA, rA), "dA has a fixed order: the bits of the typed plan's"
        assert torch.allclose(gB, rB, rtol=1e-9, atol=0.0) and not torch.isnan(gB).any()
    finally:
        plan.close()
        ref.close()


# 11. refusals: no backward on a plan of another semiring, the type and the width stay fixed
def test_semiring_refusals(tool):
    A, B, Cp, Ci, _ = small_pair()
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    av, bv, G = dev(tool, sr_values(A.nnz, 81)), dev(tool, sr_values(B.nnz, 1081)), dev(tool, sr_values(len(Ci), 82))
    refused = (mhspgemm.MHSpGEMMError, ValueError)
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, semiring="max_min")
    try:
        oA, oB = filled(tool, A.nnz), filled(tool, B.nnz)
        with pytest.raises(refused, match="max_min"):
            plan.grad(G, av, bv, out_A=oA, out_B=oB)
        oA3, oB3 = (torch.full((3, n), float("nan"), dtype=torch.float64, device=G.device) for n in (A.nnz, B.nnz))
        with pytest.raises(refused, match="max_min"):
            plan.grad_batched(G.expand(3, -1).contiguous(), av, bv, out_A=oA3, out_B=oB3)
        ra, rb = av.clone().requires_grad_(True), bv.clone().requires_grad_(True)
        with pytest.raises(refused, match="max_min"):
            plan.apply(ra, rb)
        with pytest.raises(refused, match="max_min"):
            plan.apply_batched(ra.expand(2, -1).contiguous(), rb)
        torch.cuda.synchronize()
        for t in (oA, oB, oA3, oB3):
            assert torch.isnan(t).all(), "a refused backward writes nothing"
        # the library's own refusals, on the four entry points, name the semiring
        L = _lib.lib()
        pad = G.data_ptr()
        assert L.mhs_spgemm_values_grad(tool.ctx, plan.plan, pad, pad, pad, oA.data_ptr(), oB.data_ptr(), None) == 3
        assert b"max_min" in L.mhs_last_error(tool.ctx)
        assert L.mhs_spgemm_values_grad_batched(tool.ctx, plan.plan, 1, pad, 0, pad, 0, pad, len(Ci), oA.data_ptr(), A.nnz,
                                                oB.data_ptr(), B.nnz, None) == 3
        assert b"max_min" in L.mhs_last_error(tool.ctx)
        # an _f32 call on an FP64 semiring plan
        out32 = nan_filled(tool, len(Ci), "float32")
        assert L.mhs_spgemm_values_f32(tool.ctx, plan.plan, pad, pad, out32.data_ptr(), None) == 3
        msg = L.mhs_last_error(tool.ctx)
        assert b"FP64" in msg and b"FP32" in msg
        torch.cuda.synchronize()
        assert torch.isnan(out32).all() and torch.isnan(oA).all() and torch.isnan(oB).all()
    finally:
        plan.close()
    with pytest.raises(ValueError, match="width"):
        mhspgemm.ValuesPlan(tool, dA, dB, dC, width=2, semiring="min_plus")
    # ... and the library's: a semiring that is none
    p = ctypes.c_void_p()
    a, b, c = dA.c_view(), dB.c_view(), dC.c_view()
    for bad in (-1, 4):
        assert L.mhs_values_plan_create_semiring(tool.ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), 0, 0,
                                                 _lib.MHS_F64, bad, ctypes.byref(p)) == 3 and not p.value
        assert b"semiring" in L.mhs_last_error(tool.ctx)


# 12. unsynchronised use: MHS_OPT_SYNC 0 on a torch stream, two calls queued back to back, read after one synchronise
def test_semiring_stream_ordered(tool):
    A, B, Cp, Ci, pqs = small_pair()
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    vals = [(sr_values(A.nnz, 91 + i), sr_values(B.nnz, 1091 + i)) for i in range(2)]
    plans = [mhspgemm.ValuesPlan(tool, dA, dB, dC, semiring=sr) for sr in ("min_plus", "max_min")]
    ins = [(dev(tool, a), dev(tool, b)) for a, b in vals]
    outs = [filled(tool, len(Ci)) for _ in plans]
    stream = torch.cuda.Stream(device=tool.device)
    tool.set_option(_lib.MHS_OPT_SYNC, 0)
    tool.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            for plan, (a, b), out in zip(plans, ins, outs):
                assert plan.run(a, b, out=out) is None
        torch.cuda.synchronize()
        got = [out.cpu().numpy() for out in outs]
    finally:
        tool.set_option(_lib.MHS_OPT_SYNC, 1)
        tool.set_stream(None)
        for plan in plans:
            plan.close()
    for sr, (a, b), g in zip(("min_plus", "max_min"), vals, got):
        assert np.array_equal(g, reference(sr, pqs, a, b, len(Ci))), sr
