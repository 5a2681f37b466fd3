"""GPU tests of the soft semiring plans (mhspgemm.ValuesPlan(semiring="min_plus" | "max_plus", smooth="lse") over
mhs_values_plan_create_smooth): the log-sum-exp forward through the existing hot calls, in every row class, and its
gradient (ValuesPlan.softgrad over mhs_spgemm_values_softgrad), FP64 and FP32.

The reference is numpy in long double (FP32 plans: double) on the products v = a[p] + b[q] formed in the plan's dtype
over _util.expand's kept products (A entry p, B entry q, C slot s).  The bounds are the header's (include/mhspgemm.h),
with u = 2^-53 or 2^-24, E the exact result on the v, m the kept products of the entry, V = max |v|:
  team, wave, block and dot rows   |got - E| <= 1.01 u (|E| + 2 m + 2 c_exp + 2 c_log ln m)
  global rows                      |got - E| <= 1.01 m u (V + ln m + 2 c_exp + 2 c_log + 1)
  softgrad, an output entry of m' terms w = G[s] exp(-+(v - Cval[s])) exact on the Cval handed in, S = sum |w|,
  D = max |v - Cval[s]|            |got - exact| <= 1.01 (m' + D + 2 c_exp + 1) u S  (+ m' 2^-126 max |G| in FP32)
c_exp and c_log are the device library's worst observed errors in ulps, rounded up, plus 1
(tools/ulp_probe.hip, profiles/smooth/ulp_probe.txt): 2 and 2 in FP64, 2 and 4 in FP32.  No entry is left out of a
bound check; entries whose exact result is not finite are compared for equality.  Values are uniform in [-8, 8]
unless noted; every output buffer starts as NaN."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mhspgemm
from mhspgemm import _lib
from oracle import oracle as orc
from _util import (GOLDEN, PRODUCT_CASES, bin_zoo, csr_of, device_csr, edge_val, expand, load_golden, many_a_entries, random_csr,
                   tiny_zoo)
from test_gpu_values_batched import rect_mask_case, triangle_case, val_class

pytestmark = pytest.mark.gpu

TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL, DOT = 1, 2, 3, 4, 5, 6, 7
WIDE = 1_000_000
SEMIRINGS = ("min_plus", "max_plus")
DTYPES = ("float64", "float32")
SIGN = {"min_plus": -1.0, "max_plus": 1.0}
IDENTITY = {"min_plus": np.inf, "max_plus": -np.inf}
NP = {"float64": np.float64, "float32": np.float32}
HI = {"float64": np.longdouble, "float32": np.float64}  # the reference's type
U = {"float64": 2.0 ** -53, "float32": 2.0 ** -24}
VB = {"float64": 8, "float32": 4}
C_EXP = {"float64": 2, "float32": 2}  # profiles/smooth/ulp_probe.txt: worst 0.8750 and 1.0000 ulp
C_LOG = {"float64": 2, "float32": 4}  # ... 0.6392 and 2.3315 ulp (log and log1p)
both = pytest.mark.parametrize("sr", SEMIRINGS)
types = pytest.mark.parametrize("dtype", DTYPES)


# ------------------------------------------------------------------ values, uploads, references ---
def values(n, seed, dtype="float64", lo=-8.0, hi=8.0):
    """n values uniform in [lo, hi), as the plan's type holds them."""
    return np.random.default_rng(seed).uniform(lo, hi, n).astype(NP[dtype])


def dev(tool, v, dtype):
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=NP[dtype])).to(f"cuda:{tool.device}")
    torch.cuda.synchronize()
    return t


def nans(tool, n, dtype):
    out = torch.full((n,), float("nan"), dtype=getattr(torch, dtype), device=f"cuda:{tool.device}")
    torch.cuda.synchronize()
    return out


def seg(ufunc, idx, w, n, init):
    """out[k] = ufunc over w[idx == k] in w's type, `init` where there is none."""
    out = np.full(n, init, w.dtype)
    if len(idx):
        order = np.argsort(idx, kind="stable")
        slots, starts = np.unique(np.asarray(idx)[order], return_index=True)
        out[slots] = ufunc.reduceat(w[order], starts)
    return out


def soft_reference(sr, pqs, av, bv, nC, dtype):
    """(E, m, V): per entry the exact soft result on the products formed in the plan's dtype, their count, max |v|."""
    p, q, s = pqs
    H = HI[dtype]
    v = av.astype(NP[dtype])[p] + bv.astype(NP[dtype])[q]
    assert v.dtype == NP[dtype]
    vs = (SIGN[sr] * v).astype(H)
    M = seg(np.maximum, s, vs, nC, H(-np.inf))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = np.where(np.isfinite(M[s]), np.exp(vs - M[s]), H(0))
        ssum = seg(np.add, s, t.astype(H), nC, H(0))
        E = H(SIGN[sr]) * np.where(np.isfinite(M), M + np.log(ssum), M)
    return E, np.bincount(s, minlength=nC).astype(np.int64), seg(np.maximum, s, np.abs(v).astype(H), nC, H(0))


def assert_forward(got, ref, is_global, dtype, what):
    """Every entry of got against the reference: equal where the exact result is not finite, else within its class's bound."""
    E, m, V = ref
    H, u, ce, cl = HI[dtype], U[dtype], C_EXP[dtype], C_LOG[dtype]
    assert got.dtype == NP[dtype] and got.shape == E.shape, what
    assert not np.isnan(got).any(), f"{what}: every entry is written"
    fin = np.isfinite(E)
    assert np.array_equal(got[~fin].astype(H), E[~fin]), f"{what}: the identity and the infinities are exact"
    lnm = np.log(np.maximum(m, 1)).astype(H)
    lds = H(1.01 * u) * (np.abs(E) + 2 * m + 2 * ce + 2 * cl * lnm)
    glob = H(1.01 * u) * m * (V + lnm + 2 * ce + 2 * cl + 1)
    bound = np.where(is_global, glob, lds)
    err = np.abs(np.where(fin, got.astype(H), H(0)) - np.where(fin, E, H(0)))
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=fin)
    for name, sel in (("LDS-class", fin & ~is_global), ("global-class", fin & is_global)):
        if sel.any():
            print(f"soft forward, {what}, {name} rows: worst err / bound {float(ratio[sel].max()):.3f} over {sel.sum()} entries, "
                  f"max m {m[sel].max()}")
    bad = fin & (err > bound)
    assert not bad.any(), f"{what}: {bad.sum()} entries outside the bound (worst err / bound {float(ratio.max(initial=0)):.3e})"


def grad_reference(sr, pqs, av, bv, cval, G, nnzA, nnzB, dtype):
    """The exact terms of the gradient on the Cval handed in, and per output entry of dA and of dB the tuple
    (exact sum, m', S, D)."""
    p, q, s = pqs
    H = HI[dtype]
    v = av.astype(NP[dtype])[p] + bv.astype(NP[dtype])[q]
    c = cval.astype(NP[dtype])[s]
    with np.errstate(invalid="ignore", over="ignore"):
        d = H(SIGN[sr]) * (v.astype(H) - c.astype(H))
        ok = np.isfinite(c)
        w = np.where(ok, G.astype(NP[dtype])[s].astype(H) * np.exp(np.where(ok, d, H(0))), H(0))
        D = np.where(ok, np.abs(d), H(0))
    return [(seg(np.add, i, w, n, H(0)), np.bincount(i, minlength=n).astype(np.int64), seg(np.add, i, np.abs(w), n, H(0)),
             seg(np.maximum, i, D, n, H(0))) for i, n in ((p, nnzA), (q, nnzB))]


def assert_grad(got, ref, G, dtype, what):
    exact, m, S, D = ref
    H, u, ce = HI[dtype], U[dtype], C_EXP[dtype]
    assert got.dtype == NP[dtype] and got.shape == exact.shape, what
    assert not np.isnan(got).any(), f"{what}: every entry is written"
    assert np.all(got[m == 0] == 0.0), f"{what}: entries no product reaches are exactly 0"
    bound = H(1.01 * u) * (m + D + 2 * ce + 1) * S
    if dtype == "float32":
        finite_g = np.abs(G[np.isfinite(G)])
        bound = bound + m * 2.0 ** -126 * (finite_g.max() if len(finite_g) else 0.0)
    err = np.abs(got.astype(H) - exact)
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    print(f"softgrad, {what}: worst err / bound {float(ratio.max(initial=0)):.3f} over {len(got)} entries, max m' {m.max(initial=0)}")
    bad = err > bound
    assert not bad.any(), f"{what}: {bad.sum()} entries outside the bound (worst err / bound {float(ratio.max(initial=0)):.3e})"


# ------------------------------------------------------------------ plans and cases ---
def soft_plan(tool, dA, dB, dC, sr, dtype, **kw):
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, dtype=dtype, semiring=sr, smooth="lse", **kw)
    info = plan.info()
    assert plan.smooth == "lse" and plan.semiring == sr
    assert info["smooth"] == "lse" and info["semiring"] == sr and info["width"] == 1 and info["dtype"] == dtype, info
    return plan, info


def forward(tool, plan, av, bv, nC, dtype):
    out = nans(tool, nC, dtype)
    assert plan.run(dev(tool, av, dtype), dev(tool, bv, dtype), out=out) is None
    torch.cuda.synchronize()
    return out.cpu().numpy()


def backward(tool, plan, G, cval, av, bv, nnzA, nnzB, dtype, need_A=True, need_B=True):
    oA, oB = nans(tool, nnzA, dtype), nans(tool, nnzB, dtype)
    dA, dB = plan.softgrad(dev(tool, G, dtype), dev(tool, cval, dtype), dev(tool, av, dtype), dev(tool, bv, dtype),
                           need_A=need_A, need_B=need_B, out_A=oA, out_B=oB)
    torch.cuda.synchronize()
    assert (dA is oA if need_A else dA is None) and (dB is oB if need_B else dB is None)
    return oA.cpu().numpy(), oB.cpu().numpy()


def width2_rows(tool, dA, dB, dC, dtype, **kw):
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, dtype=dtype, width=2, **kw)
    try:
        return plan.info()["rows"]
    finally:
        plan.close()


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
    return with_pattern(A, B)


def with_pattern(A, B):
    Cp, Ci, _ = orc.spgemm(A.ptr, A.col, np.ones(A.nnz), B.ptr, B.col, np.ones(B.nnz), B.N)
    return A, B, Cp, Ci, expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)


def on_device(tool, A, B, Cp, Ci):
    dA = device_csr(tool, A.M, A.N, A.ptr, A.col, A.val)
    dB = dA if B is A else device_csr(tool, B.M, B.N, B.ptr, B.col, B.val)
    return dA, dB, device_csr(tool, A.M, B.N, Cp, Ci)


def global_entries(A, B, Cp, Ci, dtype):
    """Per C entry whether its row is of the global class of a plan that classifies at twice the value's bytes."""
    n = np.diff(Cp).astype(np.int64)
    products = np.add.reduceat(np.append(np.diff(B.ptr)[A.col], 0), A.ptr[:-1].astype(np.int64)) * (np.diff(A.ptr) > 0)
    rows = np.zeros(len(n), bool)
    for i in np.nonzero(n > 0)[0]:
        span = int(Ci[Cp[i + 1] - 1]) - int(Ci[Cp[i]]) + 1
        rows[i] = val_class(int(n[i]), span, int(products[i]), 2 * VB[dtype]) == GLOBAL
    return np.repeat(rows, n), int(rows.sum())


def pair_values(A, B, seed, dtype):
    av = values(A.nnz, seed, dtype)
    return av, (av if B is A else values(B.nnz, seed + 1000, dtype))


# ------------------------------------------------------------------ 1. goldens ---
@types
@both
@pytest.mark.parametrize("name", PRODUCT_CASES)
def test_smooth_golden_products(tool, name, sr, dtype):
    A, B, Cp, Ci, pqs = case(name)
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    av, bv = pair_values(A, B, 1, dtype)
    plan, info = soft_plan(tool, dA, dB, dC, sr, dtype)
    try:
        assert info["rows"][GLOBAL] == 0 and info["nnzC"] == len(Ci) and info["products"] == info["kept_products"] == len(pqs[0])
        got = forward(tool, plan, av, bv, len(Ci), dtype)
        assert_forward(got, soft_reference(sr, pqs, av, bv, len(Ci), dtype), np.zeros(len(Ci), bool), dtype, f"{name} {sr}")
        if name == "duplicates":  # every duplicate is a product of its own: on equal values, log(m) from the hard plan
            one = np.ones(max(A.nnz, B.nnz), NP[dtype])
            m = np.bincount(pqs[2], minlength=len(Ci))
            assert (m >= 2).any()
            soft = forward(tool, plan, 1.5 * one[:A.nnz], 2.25 * one[:B.nnz], len(Ci), dtype)
            hard_plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, dtype=dtype, semiring=sr)
            try:
                hard = forward(tool, hard_plan, 1.5 * one[:A.nnz], 2.25 * one[:B.nnz], len(Ci), dtype)
            finally:
                hard_plan.close()
            assert np.all(hard == 3.75)
            want = 3.75 + SIGN[sr] * np.log(m.astype(HI[dtype]))
            assert np.all(np.abs(soft - want) <= 1.01 * U[dtype] * (np.abs(want) + 2 * m + 2 * C_EXP[dtype] + 2 * C_LOG[dtype] * np.log(m)))
            assert np.all(np.abs(soft[m == 2] - hard[m == 2]) > 0.69)
    finally:
        plan.close()


# ------------------------------------------------------------------ 2. every class ---
@types
@both
@pytest.mark.parametrize("name", ("bin_zoo", "tiny_zoo"))
def test_smooth_every_class(tool, name, sr, dtype):
    A, B, Cp, Ci, pqs = case(name)
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    av, bv = pair_values(A, B, 3, dtype)
    G = values(len(Ci), 5, dtype, -1.0, 1.0)
    is_global, nglobal = global_entries(A, B, Cp, Ci, dtype)
    plan, info = soft_plan(tool, dA, dB, dC, sr, dtype)
    try:
        assert info["rows"] == width2_rows(tool, dA, dB, dC, dtype), "the rows per class of the width-2 plus-times plan"
        assert info["rows"][GLOBAL] == nglobal and info["rows"][DOT] == 0
        if name == "bin_zoo":
            assert nglobal >= 1 and is_global.any()
        got = forward(tool, plan, av, bv, len(Ci), dtype)
        assert_forward(got, soft_reference(sr, pqs, av, bv, len(Ci), dtype), is_global, dtype, f"{name} {sr} {dtype}")
        rA, rB = grad_reference(sr, pqs, av, bv, got, G, A.nnz, B.nnz, dtype)
        gA, gB = backward(tool, plan, G, got, av, bv, A.nnz, B.nnz, dtype)
        assert_grad(gA, rA, G, dtype, f"{name} {sr} {dtype} dA")
        assert_grad(gB, rB, G, dtype, f"{name} {sr} {dtype} dB")
        onlyA, untouchedB = backward(tool, plan, G, got, av, bv, A.nnz, B.nnz, dtype, need_B=False)
        untouchedA, onlyB = backward(tool, plan, G, got, av, bv, A.nnz, B.nnz, dtype, need_A=False)
        assert np.isnan(untouchedA).all() and np.isnan(untouchedB).all(), "a side not asked for is not touched"
        assert onlyA.tobytes() == gA.tobytes(), "dA has a fixed order: the same bits on every call"
        assert_grad(onlyB, rB, G, dtype, f"{name} {sr} {dtype} dB alone")
    finally:
        plan.close()


def test_smooth_every_class_has_rows(tool):
    for dtype in DTYPES:
        rows = np.zeros(8, np.int64)
        for name in ("bin_zoo", "tiny_zoo"):
            A, B, Cp, Ci, _ = case(name)
            plan, info = soft_plan(tool, *on_device(tool, A, B, Cp, Ci), "min_plus", dtype)
            plan.close()
            rows += info["rows"]
        for cls in (TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL):
            assert rows[cls] > 0, f"class {cls} has no rows in bin_zoo + tiny_zoo ({dtype})"


# A rows of 65, 257 and 700 entries (_util.many_a_entries): the staged walk of the forward and of the
# gradient refills its stage inside a row -- past 64 entries in a wave class, past 256 in a block class -- and leaves
# lane groups idle in the last step
@types
@both
def test_smooth_stage_boundaries(tool, sr, dtype):
    A, B, Cp, Ci, pqs = many_a_entries()
    nA = np.diff(A.ptr)
    assert {65, 257, 700} <= set(nA.tolist())
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    av, bv = pair_values(A, B, 121, dtype)
    G = values(len(Ci), 123, dtype, -1.0, 1.0)
    # the class of every row at the plan's two planes, and through it the rows whose stage is refilled
    products = np.add.reduceat(np.append(np.diff(B.ptr)[A.col], 0), A.ptr[:-1].astype(np.int64))
    cls = np.array([val_class(int(Cp[i + 1] - Cp[i]), int(Ci[Cp[i + 1] - 1]) - int(Ci[Cp[i]]) + 1, int(products[i]), 2 * VB[dtype])
                    for i in range(A.M)])
    plan, info = soft_plan(tool, dA, dB, dC, sr, dtype)
    try:
        assert list(info["rows"]) == np.bincount(cls, minlength=len(info["rows"])).tolist(), info
        assert (np.isin(cls, (WAVE_DIRECT, WAVE_SEARCH)) & (nA > 64)).any(), "a wave row that refills its stage"
        assert (np.isin(cls, (BLOCK_DIRECT, BLOCK_SEARCH)) & (nA > 256)).any(), "a block row that refills its stage"
        got = forward(tool, plan, av, bv, len(Ci), dtype)
        assert_forward(got, soft_reference(sr, pqs, av, bv, len(Ci), dtype), np.repeat(cls == GLOBAL, np.diff(Cp)), dtype, f"stage {sr} {dtype}")
        rA, rB = grad_reference(sr, pqs, av, bv, got, G, A.nnz, B.nnz, dtype)
        gA, gB = backward(tool, plan, G, got, av, bv, A.nnz, B.nnz, dtype)
        assert_grad(gA, rA, G, dtype, f"stage {sr} {dtype} dA")
        assert_grad(gB, rB, G, dtype, f"stage {sr} {dtype} dB")
    finally:
        plan.close()


# ------------------------------------------------------------------ 3. class edges ---
# (at, above): edge_val's (n, span, products), then the classes of the two sides, at the sum bytes 2 x vb
EDGES = {
    16: {"wave_direct_span": ((200, 512, 1000), (200, 513, 1000), (WAVE_DIRECT, BLOCK_DIRECT)),
         "wave_search_n": ((408, WIDE, 2000), (409, WIDE, 2000), (WAVE_SEARCH, BLOCK_SEARCH)),
         "block_direct_span": ((3000, 9984, 4000), (3000, 9985, 4000), (BLOCK_DIRECT, BLOCK_SEARCH)),
         "block_search_n": ((7986, WIDE, 8000), (7987, WIDE, 8000), (BLOCK_SEARCH, GLOBAL))},
    8: {"wave_direct_span": ((200, 1024, 1000), (200, 1025, 1000), (WAVE_DIRECT, BLOCK_DIRECT)),
        "wave_search_n": ((682, WIDE, 2000), (683, WIDE, 2000), (WAVE_SEARCH, BLOCK_SEARCH)),
        "block_direct_span": ((3000, 19968, 4000), (3000, 19969, 4000), (BLOCK_DIRECT, BLOCK_SEARCH)),
        "block_search_n": ((13312, WIDE, 13400), (13313, WIDE, 13400), (BLOCK_SEARCH, GLOBAL))},
}


@functools.lru_cache(maxsize=None)
def edge_rows_of(n, span, products):
    A, B = (csr_of(t) for t in edge_val(n, span, products))
    return with_pattern(A, B)


@types
@both
@pytest.mark.parametrize("side", [0, 1], ids=["at", "above"])
@pytest.mark.parametrize("name", list(EDGES[16]))
def test_smooth_class_edges(tool, name, side, sr, dtype):
    sb = 2 * VB[dtype]
    edge = EDGES[sb][name]
    n, span, products = edge[side]
    A, B, Cp, Ci, pqs = edge_rows_of(n, span, products)
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    av, bv = pair_values(A, B, 50, dtype)
    G = values(len(Ci), 52, dtype, -1.0, 1.0)
    plan, info = soft_plan(tool, dA, dB, dC, sr, dtype)
    try:
        classes = [c for c in range(8) if info["rows"][c]]
        assert sum(info["rows"]) == A.M and classes == [edge[2][side]] == [val_class(n, span, products, sb)], info
        got = forward(tool, plan, av, bv, len(Ci), dtype)
        is_global = np.full(len(Ci), classes == [GLOBAL])
        assert_forward(got, soft_reference(sr, pqs, av, bv, len(Ci), dtype), is_global, dtype, f"{name} {sr} {dtype}")
        rA, rB = grad_reference(sr, pqs, av, bv, got, G, A.nnz, B.nnz, dtype)
        gA, gB = backward(tool, plan, G, got, av, bv, A.nnz, B.nnz, dtype)
        assert_grad(gA, rA, G, dtype, f"{name} {sr} {dtype} dA")
        assert_grad(gB, rB, G, dtype, f"{name} {sr} {dtype} dB")
    finally:
        plan.close()


# ------------------------------------------------------------------ 4. masked plans ---
@functools.lru_cache(maxsize=None)
def mask_input(which):
    A, B, Mp, Mc = triangle_case() if which == "triangle" else rect_mask_case()
    return A, B, Mp, Mc, expand(A.ptr, A.col, B.ptr, B.col, Mp, Mc, B.N)


@types
@both
@pytest.mark.parametrize("form", ["product", "dot", "auto"])
@pytest.mark.parametrize("which", ["triangle", "rect"])
def test_smooth_masked(tool, which, form, sr, dtype):
    A, B, Mp, Mc, pqs = mask_input(which)
    dA, dB, dC = on_device(tool, A, B, Mp, Mc)
    av, bv = pair_values(A, B, 21, dtype)
    reached = np.zeros(len(Mc), bool)
    reached[pqs[2]] = True
    # (the rectangular mask is a subset of the product's pattern: the triangle is the case with unreached entries)
    assert reached.any() and (which == "rect" or not reached.all()), "the triangle needs mask entries no product reaches"
    assert len(pqs[0]) < orc.flop(A.col, B.ptr), "the case needs products outside the mask"
    G = values(len(Mc), 23, dtype, -1.0, 1.0)
    G[~reached] = np.nan  # an unreached entry passes no gradient: its cotangent is never used
    plan, info = soft_plan(tool, dA, dB, dC, sr, dtype, masked=True, form=form)
    try:
        assert info["rows"] == width2_rows(tool, dA, dB, dC, dtype, masked=True, form=form)
        assert info["kept_products"] == len(pqs[0])
        if form == "dot":
            assert info["rows"][DOT] == np.count_nonzero((np.diff(Mp) > 0) & (np.diff(A.ptr) > 0)) > 0
        if form == "product":
            assert info["rows"][DOT] == 0
        got = forward(tool, plan, av, bv, len(Mc), dtype)
        # (a global-class row of a masked plan has no products: its entries are the identity, compared for equality)
        assert_forward(got, soft_reference(sr, pqs, av, bv, len(Mc), dtype), np.zeros(len(Mc), bool), dtype, f"{which} {form} {sr}")
        assert np.all(got[~reached] == IDENTITY[sr]) and np.isfinite(got[reached]).all()
        if form == "dot":
            again = forward(tool, plan, av, bv, len(Mc), dtype)
            assert again.tobytes() == got.tobytes(), "dot rows: the same bits on every call"
        rA, rB = grad_reference(sr, pqs, av, bv, got, G, A.nnz, B.nnz, dtype)
        gA, gB = backward(tool, plan, G, got, av, bv, A.nnz, B.nnz, dtype)
        assert_grad(gA, rA, G, dtype, f"{which} {form} {sr} dA")
        assert_grad(gB, rB, G, dtype, f"{which} {form} {sr} dB")
    finally:
        plan.close()


# ------------------------------------------------------------------ 5. exact anchors ---
@functools.lru_cache(maxsize=None)
def small_pair():
    p, c, v = random_csr(800, 600, 6, 31)
    Bp, Bc, Bv = random_csr(600, 3000, 8, 32)
    return with_pattern(mhspgemm.CSR(800, 600, p, c, v), mhspgemm.CSR(600, 3000, Bp, Bc, Bv))


@functools.lru_cache(maxsize=None)
def permutation_pair():
    """A random, B a permutation matrix: every C entry has one product."""
    p, c, v = random_csr(700, 500, 6, 41)
    perm = np.random.default_rng(42).permutation(500).astype(np.int32)
    A = mhspgemm.CSR(700, 500, p, c, v)
    B = mhspgemm.CSR(500, 500, np.arange(501, dtype=np.int32), perm, np.ones(500))
    return with_pattern(A, B)


@types
@both
def test_smooth_one_product_per_entry_is_exact(tool, sr, dtype):
    A, B, Cp, Ci, (p, q, s) = permutation_pair()
    assert len(s) == len(Ci) == A.nnz and np.array_equal(np.sort(s), np.arange(len(Ci)))
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    av, bv = pair_values(A, B, 61, dtype)
    G = values(len(Ci), 63, dtype, -1.0, 1.0)
    plan, _ = soft_plan(tool, dA, dB, dC, sr, dtype)
    try:
        got = forward(tool, plan, av, bv, len(Ci), dtype)
        want = np.empty(len(Ci), NP[dtype])
        want[s] = av[p] + bv[q]
        assert got.tobytes() == want.tobytes(), "one product: the forward is that product, bit for bit"
        gA, gB = backward(tool, plan, G, got, av, bv, A.nnz, B.nnz, dtype)
        wantA, wantB = np.zeros(A.nnz, NP[dtype]), np.zeros(B.nnz, NP[dtype])
        wantA[p] = G[s]
        np.add.at(wantB, q, G[s])  # (a B entry gathers the cotangents of its column's entries: summed in any order)
        assert np.array_equal(gA, wantA), "one product: its weight is 1, dA is the gathered G"
        m = np.bincount(q, minlength=B.nnz)
        assert np.all(np.abs(gB.astype(np.float64) - wantB) <= 1.01 * U[dtype] * m * np.bincount(q, np.abs(G[s]), B.nnz))
        assert np.array_equal(gB[m == 1], wantB[m == 1])
    finally:
        plan.close()


@types
@both
def test_smooth_wide_gaps_are_the_hard_plan(tool, sr, dtype):
    A, B, Cp, Ci, pqs = small_pair()
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    rng = np.random.default_rng(71)
    av = (1024.0 * rng.integers(-4000, 4001, A.nnz)).astype(NP[dtype])  # multiples of 1024 below 2^23 in magnitude
    bv = (1024.0 * rng.integers(-4000, 4001, B.nnz)).astype(NP[dtype])
    assert max(np.abs(av).max(), np.abs(bv).max()) < 2 ** 23
    p, q, s = pqs
    H = HI[dtype]
    vs = (SIGN[sr] * (av[p].astype(np.float64) + bv[q])).astype(H)  # (integers below 2^24: exact in either type)
    M = seg(np.maximum, s, vs, len(Ci), H(-np.inf))
    ties = np.bincount(s, vs == M[s], len(Ci)).astype(np.int64)
    assert (ties == 1).sum() > 0.9 * len(Ci) and (ties >= 1).all()
    plan, _ = soft_plan(tool, dA, dB, dC, sr, dtype)
    hard = mhspgemm.ValuesPlan(tool, dA, dB, dC, dtype=dtype, semiring=sr)
    try:
        got = forward(tool, plan, av, bv, len(Ci), dtype)
        want = forward(tool, hard, av, bv, len(Ci), dtype)
    finally:
        plan.close()
        hard.close()
    one = ties == 1
    assert got[one].tobytes() == want[one].tobytes(), "a unique extreme product: the hard plan's bits (the others underflow to 0)"
    E = H(SIGN[sr]) * (M + np.log(ties.astype(H)))
    m = np.bincount(s, minlength=len(Ci))
    bound = H(1.01 * U[dtype]) * (np.abs(E) + 2 * m + 2 * C_EXP[dtype] + 2 * C_LOG[dtype] * np.log(m))
    assert np.all(np.abs(got.astype(H) - E) <= bound), "elsewhere: M +- log(ties)"


# ------------------------------------------------------------------ 6. non-finite values ---
def tiny_case():
    """A 4 x 3 times 3 x 2: row i of C has the products of A's row i with B's rows; every C entry has 3 products."""
    A = mhspgemm.CSR(4, 3, np.arange(0, 13, 3, dtype=np.int32), np.tile(np.arange(3, dtype=np.int32), 4), np.ones(12))
    B = mhspgemm.CSR(3, 2, np.arange(0, 7, 2, dtype=np.int32), np.tile(np.arange(2, dtype=np.int32), 3), np.ones(6))
    return with_pattern(A, B)


@types
@both
def test_smooth_nonfinite(tool, sr, dtype):
    A, B, Cp, Ci, pqs = tiny_case()
    assert len(Ci) == 8 and np.all(np.bincount(pqs[2]) == 3)
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    ident, opp = IDENTITY[sr], -IDENTITY[sr]
    av, bv = values(A.nnz, 81, dtype), values(B.nnz, 82, dtype)
    av[0:3] = ident   # row 0: every product is "no edge"        -> the identity
    av[3] = ident     # row 1: an identity operand beside finite -> ignored
    av[6] = opp       # row 2: the opposite infinity             -> that infinity
    av[9] = np.nan    # row 3: a NaN operand                     -> NaN, or the rest
    plan, _ = soft_plan(tool, dA, dB, dC, sr, dtype)
    try:
        got = forward(tool, plan, av, bv, len(Ci), dtype)
        assert np.all(got[0:2] == ident) and np.all(got[4:6] == opp)
        skip = pqs[0] == 9
        rest = soft_reference(sr, tuple(x[~skip] for x in pqs), av, bv, len(Ci), dtype)
        assert np.all(np.isnan(got[6:8]) | (np.abs(got[6:8] - rest[0][6:8]) <= 1e-5 * (1 + np.abs(rest[0][6:8])))), "NaN, or the rest"
        clean = av.copy()
        clean[9] = 0.0
        want = soft_reference(sr, pqs, clean, bv, len(Ci), dtype)
        with_nan = got.copy()
        with_nan[6:8] = want[0][6:8].astype(NP[dtype])  # (row 3 was judged above; its neighbours are judged here)
        assert_forward(with_nan, want, np.zeros(8, bool), dtype, f"nonfinite {sr} {dtype}")
        assert np.isfinite(got[2:4]).all(), "an identity operand beside finite ones is ignored"
        # softgrad with non-finite Cval entries: exactly 0 from there, the bound elsewhere
        cval = got.copy()
        cval[6:8] = np.nan
        G = values(len(Ci), 83, dtype, -1.0, 1.0)
        fa, fb = values(A.nnz, 84, dtype), values(B.nnz, 85, dtype)  # finite operands: the weights of rows 0, 2, 3 are 0 by Cval alone
        fwd = forward(tool, plan, fa, fb, len(Ci), dtype)
        cval[2:4] = fwd[2:4]
        rA, rB = grad_reference(sr, pqs, fa, fb, cval, G, A.nnz, B.nnz, dtype)
        gA, gB = backward(tool, plan, G, cval, fa, fb, A.nnz, B.nnz, dtype)
        assert np.all(gA[0:3] == 0) and np.all(gA[6:12] == 0) and np.all(gA[3:6] != 0), "a non-finite Cval passes exactly 0"
        assert_grad(gA, rA, G, dtype, f"nonfinite {sr} {dtype} dA")
        assert_grad(gB, rB, G, dtype, f"nonfinite {sr} {dtype} dB")
    finally:
        plan.close()


# ------------------------------------------------------------------ 7. stream order ---
def test_smooth_stream_ordered(tool):
    A, B, Cp, Ci, pqs = small_pair()
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    dtype, sr = "float64", "min_plus"
    av, bv = pair_values(A, B, 91, dtype)
    G = values(len(Ci), 93, dtype, -1.0, 1.0)
    plan, _ = soft_plan(tool, dA, dB, dC, sr, dtype)
    ta, tb, tg = dev(tool, av, dtype), dev(tool, bv, dtype), dev(tool, G, dtype)
    out, oA, oB = nans(tool, len(Ci), dtype), nans(tool, A.nnz, dtype), nans(tool, B.nnz, dtype)
    stream = torch.cuda.Stream(device=tool.device)
    tool.set_option(_lib.MHS_OPT_SYNC, 0)
    tool.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            assert plan.run(ta, tb, out=out) is None
            plan.softgrad(tg, out, ta, tb, out_A=oA, out_B=oB)  # reads the forward's result, queued behind it
        torch.cuda.synchronize()
        got, gA, gB = out.cpu().numpy(), oA.cpu().numpy(), oB.cpu().numpy()
    finally:
        tool.set_option(_lib.MHS_OPT_SYNC, 1)
        tool.set_stream(None)
        plan.close()
    assert_forward(got, soft_reference(sr, pqs, av, bv, len(Ci), dtype), np.zeros(len(Ci), bool), dtype, "stream ordered")
    rA, rB = grad_reference(sr, pqs, av, bv, got, G, A.nnz, B.nnz, dtype)
    assert_grad(gA, rA, G, dtype, "stream ordered dA")
    assert_grad(gB, rB, G, dtype, "stream ordered dB")


# ------------------------------------------------------------------ 8. autograd ---
@types
@both
def test_smooth_autograd_against_logsumexp(tool, sr, dtype):
    p, c, v = random_csr(40, 30, 4, 101)
    Bp, Bc, Bv = random_csr(30, 50, 5, 102)
    A, B, Cp, Ci, pqs = with_pattern(mhspgemm.CSR(40, 30, p, c, v), mhspgemm.CSR(30, 50, Bp, Bc, Bv))
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    av, bv = pair_values(A, B, 103, dtype)
    G = values(len(Ci), 105, dtype, -1.0, 1.0)
    plan, _ = soft_plan(tool, dA, dB, dC, sr, dtype)
    try:
        ta, tb = dev(tool, av, dtype).requires_grad_(True), dev(tool, bv, dtype).requires_grad_(True)
        out = plan.apply_soft(ta, tb)
        out.backward(dev(tool, G, dtype))
        torch.cuda.synchronize()
        got, gA, gB = out.detach().cpu().numpy(), ta.grad.cpu().numpy(), tb.grad.cpu().numpy()
    finally:
        plan.close()
    # torch: a dense [M, K, N] tensor of the products, -+Inf where there is none, in double on the CPU
    sg = SIGN[sr]
    ha = torch.tensor(av.astype(np.float64), requires_grad=True)
    hb = torch.tensor(bv.astype(np.float64), requires_grad=True)
    Ad = torch.full((A.M, A.N), -sg * np.inf, dtype=torch.float64)
    Bd = torch.full((B.M, B.N), -sg * np.inf, dtype=torch.float64)
    ar = np.repeat(np.arange(A.M), np.diff(A.ptr))
    br = np.repeat(np.arange(B.M), np.diff(B.ptr))
    Ad = Ad.index_put((torch.tensor(ar), torch.tensor(A.col.astype(np.int64))), ha)
    Bd = Bd.index_put((torch.tensor(br), torch.tensor(B.col.astype(np.int64))), hb)
    cr = np.repeat(np.arange(A.M), np.diff(Cp))
    dense = Ad[:, :, None] + Bd[None, :, :]  # [M, K, N]; its fibres over k at C's entries (each has a product: no NaN below)
    want = sg * torch.logsumexp(sg * dense[torch.tensor(cr), :, torch.tensor(Ci.astype(np.int64))], dim=1)
    want.backward(torch.tensor(G.astype(np.float64)))
    m = np.bincount(pqs[2], minlength=len(Ci))
    E = want.detach().numpy()
    slack = 40 * U["float64"] * (np.abs(E) + m)  # (torch's own double evaluation, on products that are not rounded to the dtype)
    rnd = U[dtype] * 2 * 16.0 if dtype == "float32" else 0.0  # (its products are exact sums: ours round once, |v| <= 16)
    bound = 1.01 * U[dtype] * (np.abs(E) + 2 * m + 2 * C_EXP[dtype] + 2 * C_LOG[dtype] * np.log(m)) + slack + rnd
    assert np.all(np.abs(got - E) <= bound)
    rA, rB = grad_reference(sr, pqs, av, bv, got, G, A.nnz, B.nnz, dtype)
    assert_grad(gA, rA, G, dtype, f"autograd {sr} {dtype} dA")
    assert_grad(gB, rB, G, dtype, f"autograd {sr} {dtype} dB")
    # and the gradients agree with torch's, which differentiates its own forward: to the forward's error times the mass
    for g, h, idx in ((gA, ha.grad.numpy(), pqs[0]), (gB, hb.grad.numpy(), pqs[1])):
        S = np.bincount(idx, np.abs(G[pqs[2]]), len(g))
        assert np.all(np.abs(g - h) <= (64 * U[dtype] * 40 + 1e-12) * S + 1e-300)


# ------------------------------------------------------------------ 9. refusals ---
def test_smooth_refusals(tool):
    A, B, Cp, Ci, _ = small_pair()
    dA, dB, dC = on_device(tool, A, B, Cp, Ci)
    L = _lib.lib()
    dtype = "float64"
    av, bv, G = dev(tool, values(A.nnz, 111), dtype), dev(tool, values(B.nnz, 112), dtype), dev(tool, values(len(Ci), 113), dtype)
    refused = (mhspgemm.MHSpGEMMError, ValueError)
    a, b, c = dA.c_view(), dB.c_view(), dC.c_view()
    ra, rb, rc = ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)
    # creation: the semiring and smooth arguments, before any HIP call
    p = ctypes.c_void_p()
    for semiring, smooth, word in ((0, 1, b"plus_times"), (3, 1, b"max_min"), (4, 1, b"semiring"), (-1, 1, b"semiring"),
                                   (1, 2, b"smooth"), (2, -1, b"smooth"), (4, 0, b"semiring")):
        assert L.mhs_values_plan_create_smooth(tool.ctx, ra, rb, rc, 0, 0, _lib.MHS_F64, semiring, smooth, ctypes.byref(p)) == 3
        assert not p.value and word in L.mhs_last_error(tool.ctx), (semiring, smooth, L.mhs_last_error(tool.ctx))
    assert L.mhs_values_plan_create_semiring(tool.ctx, ra, rb, rc, 0, 0, _lib.MHS_F64, 4, ctypes.byref(p)) == 3 and not p.value
    # MHS_SMOOTH_NONE is mhs_values_plan_create_semiring
    assert L.mhs_values_plan_create_smooth(tool.ctx, ra, rb, rc, 0, 0, _lib.MHS_F64, 3, 0, ctypes.byref(p)) == 0 and p.value
    sm, srv = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.mhs_values_plan_smooth(p, ctypes.byref(sm)) == 0 and sm.value == _lib.MHS_SMOOTH_NONE
    assert L.mhs_values_plan_semiring(p, ctypes.byref(srv)) == 0 and srv.value == 3
    L.mhs_values_plan_destroy(tool.ctx, p)

    # mhs_values_plan_smooth is NONE on plain, masked, mixed and hard-semiring plans; softgrad refuses them and points on
    others = [({}, b"mhs_spgemm_values_grad"), ({"masked": True}, b"mhs_spgemm_values_grad"),
              ({"dtype": "float32", "accum": "float64"}, b"mhs_spgemm_values_grad"),
              ({"semiring": "min_plus"}, b"mhs_spgemm_values_subgrad"), ({"semiring": "max_min"}, b"mhs_spgemm_values_subgrad")]
    for kw, points_at in others:
        plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, **kw)
        try:
            assert plan.smooth is None and plan.info()["smooth"] is None
            assert L.mhs_values_plan_smooth(plan.plan, ctypes.byref(sm)) == 0 and sm.value == _lib.MHS_SMOOTH_NONE
            f32 = kw.get("dtype") == "float32"
            t = "float32" if f32 else "float64"
            oA, oB = nans(tool, A.nnz, t), nans(tool, B.nnz, t)
            call = L.mhs_spgemm_values_softgrad_f32 if f32 else L.mhs_spgemm_values_softgrad
            pad = G.data_ptr()
            assert call(tool.ctx, plan.plan, pad, pad, pad, pad, oA.data_ptr(), oB.data_ptr(), None) == 3
            msg = L.mhs_last_error(tool.ctx)
            assert b"not smoothed" in msg and points_at in msg, msg
            with pytest.raises(refused, match="not smoothed"):
                plan.softgrad(G, G, av, bv, out_A=oA, out_B=oB)
            with pytest.raises(refused, match="not smoothed"):
                plan.apply_soft(av, bv)
            torch.cuda.synchronize()
            assert torch.isnan(oA).all() and torch.isnan(oB).all(), "a refused call writes nothing"
        finally:
            plan.close()

    plan, _ = soft_plan(tool, dA, dB, dC, "max_plus", dtype)
    try:
        oA, oB, oC = nans(tool, A.nnz, dtype), nans(tool, B.nnz, dtype), nans(tool, len(Ci), dtype)
        ties = torch.full((len(Ci),), -7, dtype=torch.int32, device=G.device)
        # the subgradient and the witness: weights, not winners, no witness -- and where to go
        for call in (lambda: plan.subgrad(G, G, av, bv, out_A=oA, out_B=oB, ties=ties), lambda: plan.apply_subgrad(av, bv),
                     lambda: plan.witness(G, av, bv, out=ties), lambda: plan.run_arg(av, bv)):
            with pytest.raises(refused, match="mhs_spgemm_values_softgrad"):
                call()
        pad = G.data_ptr()
        assert L.mhs_spgemm_values_subgrad(tool.ctx, plan.plan, pad, pad, pad, pad, ties.data_ptr(), oA.data_ptr(), oB.data_ptr(), None) == 3
        msg = L.mhs_last_error(tool.ctx)
        assert b"weights, not winners" in msg and b"mhs_spgemm_values_softgrad" in msg, msg
        assert L.mhs_spgemm_values_witness(tool.ctx, plan.plan, pad, pad, pad, ties.data_ptr(), None) == 3
        msg = L.mhs_last_error(tool.ctx)
        assert b"no witness" in msg and b"mhs_spgemm_values_softgrad" in msg, msg
        # the four plus-times backward entry points refuse by semiring and now name the soft gradient
        with pytest.raises(refused, match="max_plus"):
            plan.grad(G, av, bv, out_A=oA, out_B=oB)
        assert L.mhs_spgemm_values_grad(tool.ctx, plan.plan, pad, pad, pad, oA.data_ptr(), oB.data_ptr(), None) == 3
        msg = L.mhs_last_error(tool.ctx)
        assert b"max_plus" in msg and b"mhs_spgemm_values_softgrad" in msg, msg
        assert L.mhs_spgemm_values_grad_batched(tool.ctx, plan.plan, 1, pad, 0, pad, 0, pad, len(Ci), oA.data_ptr(), A.nnz,
                                                oB.data_ptr(), B.nnz, None) == 3
        assert b"mhs_spgemm_values_softgrad" in L.mhs_last_error(tool.ctx)
        # a call of the wrong type, NULL arguments, no output
        o32 = nans(tool, len(Ci), "float32")
        assert L.mhs_spgemm_values_softgrad_f32(tool.ctx, plan.plan, pad, pad, pad, pad, oA.data_ptr(), oB.data_ptr(), None) == 3
        msg = L.mhs_last_error(tool.ctx)
        assert b"FP64" in msg and b"FP32" in msg
        assert L.mhs_spgemm_values_f32(tool.ctx, plan.plan, pad, pad, o32.data_ptr(), None) == 3
        for args in ((None, pad, pad, pad), (pad, None, pad, pad), (pad, pad, None, pad), (pad, pad, pad, None)):
            assert L.mhs_spgemm_values_softgrad(tool.ctx, plan.plan, *args, oA.data_ptr(), oB.data_ptr(), None) == 3
            assert b"null" in L.mhs_last_error(tool.ctx)
        assert L.mhs_spgemm_values_softgrad(tool.ctx, plan.plan, pad, pad, pad, pad, None, None, None) == 3
        assert b"no output" in L.mhs_last_error(tool.ctx)
        assert L.mhs_spgemm_values_softgrad(tool.ctx, None, pad, pad, pad, pad, oA.data_ptr(), oB.data_ptr(), None) == 3
        assert L.mhs_spgemm_values_softgrad(None, plan.plan, pad, pad, pad, pad, oA.data_ptr(), oB.data_ptr(), None) == 3
        with pytest.raises(ValueError, match="need_A or need_B"):
            plan.softgrad(G, G, av, bv, need_A=False, need_B=False)
        torch.cuda.synchronize()
        for t in (oA, oB, oC, o32):
            assert torch.isnan(t).all(), "a refused call writes nothing"
        assert torch.all(ties == -7)
    finally:
        plan.close()
    if torch.cuda.device_count() > 1:  # a plan of another device
        other = mhspgemm.Tool(1)
        try:
            plan, _ = soft_plan(tool, dA, dB, dC, "max_plus", dtype)
            try:
                pad = G.data_ptr()
                assert L.mhs_spgemm_values_softgrad(other.ctx, plan.plan, pad, pad, pad, pad, pad, None, None) == 3
                assert b"another device" in L.mhs_last_error(other.ctx)
            finally:
                plan.close()
        finally:
            other.close()


# ------------------------------------------------------------------ 10. poison ---
def test_smooth_under_poison(tool, monkeypatch):
    """A context created with MHS_POISON=0xA5 (the switch is read when the context is made): plan memory starts as
    0xA5 bytes, and the forward and the gradient on bin_zoo are what they are without it."""
    A, B, Cp, Ci, pqs = case("bin_zoo")
    dtype, sr = "float64", "min_plus"
    av, bv = pair_values(A, B, 3, dtype)
    G = values(len(Ci), 5, dtype, -1.0, 1.0)
    is_global, _ = global_entries(A, B, Cp, Ci, dtype)
    ref = soft_reference(sr, pqs, av, bv, len(Ci), dtype)
    results = []
    for poison in (None, "0xA5"):
        if poison is None:
            monkeypatch.delenv("MHS_POISON", raising=False)
        else:
            monkeypatch.setenv("MHS_POISON", poison)
        t2 = mhspgemm.Tool(tool.device)
        monkeypatch.delenv("MHS_POISON", raising=False)
        try:
            plan, info = soft_plan(t2, *on_device(t2, A, B, Cp, Ci), sr, dtype)
            try:
                assert (t2.stat("poison_fills") > 0) == (poison is not None)
                got = forward(t2, plan, av, bv, len(Ci), dtype)
                assert_forward(got, ref, is_global, dtype, f"MHS_POISON={poison}")
                rA, rB = grad_reference(sr, pqs, av, bv, got, G, A.nnz, B.nnz, dtype)
                gA, gB = backward(t2, plan, G, got, av, bv, A.nnz, B.nnz, dtype)
                assert_grad(gA, rA, G, dtype, f"MHS_POISON={poison} dA")
                assert_grad(gB, rB, G, dtype, f"MHS_POISON={poison} dB")
                results.append((info["rows"], got))
            finally:
                plan.close()
        finally:
            t2.close()
    assert results[0][0] == results[1][0], "the classes do not depend on the switch"
    fin = np.isfinite(results[0][1])
    assert np.array_equal(fin, np.isfinite(results[1][1])) and np.array_equal(results[0][1][~fin], results[1][1][~fin])
