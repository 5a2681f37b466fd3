"""GPU tests of the semiring subgradient (mhspgemm.ValuesPlan.subgrad / apply_subgrad over mhs_spgemm_values_subgrad):
the backward of min-plus, max-plus and max-min plans in every row class, FP64 and FP32, on kept patterns and masks.

The reference is numpy over _util.expand's kept products (A entry p, B entry q, C slot s), on the shapes the forward's
tests (test_gpu_semiring.py) already prove reach every code path -- their cached cases are shared.  A product is a
winner of s when mul(a, b) == Cval[s] in the plan's type and Cval[s] is not the identity; T[s] counts them; each
carries G[s] / T[s], to both operands under the _plus semirings, to the smaller one under max-min (half each when
equal).  Two regimes, both run on one plan per case:

exact    values are integers in [-3, 3] with a few +-Inf operands (placed so that no product is Inf - Inf), so ties are
         frequent and every mul is exact.  G = T * g with g small integers, NaN where T == 0 -- which proves it is
         not read there.  Every weight is then a small integer or half of one and every sum exact: ties, dA and dB are
         held to the reference by np.array_equal, and the gradient mass to that of G.
general  values are the forward tests' sr_values (signed, magnitudes in [0.1, 1000]), G random.  ties must be exact; a
         gradient entry summed from m winning terms whose absolute values sum to S must lie within
         1.01 * (m + 1) * u * S of a long-double reference, u = 2^-53 or 2^-24: m - 1 roundings of the sum in any
         order, one of the division, and the 1.01 of _util.assert_f64_bound.  Nothing in it is measured.
Every output buffer starts as NaN."""
import functools

import numpy as np
import pytest
import torch

import mhspgemm
from mhspgemm import _lib
from oracle import oracle as orc
from _util import expand, filled, seg_sum_ld
import test_gpu_semiring as fwd

pytestmark = pytest.mark.gpu

TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL, DOT = 1, 2, 3, 4, 5, 6, 7
SEMIRINGS = fwd.SEMIRINGS
IDENTITY = fwd.IDENTITY
NP = fwd.NP
U = {"float64": 2.0 ** -53, "float32": 2.0 ** -24}
DTYPES = ("float64", "float32")


# ------------------------------------------------------------------ the reference ---
def winners(sr, pqs, av, bv, cval, dtype):
    """(win, T): per kept product whether it wins its C entry, and the winners per entry.  av, bv, cval in `dtype`."""
    p, q, s = pqs
    a, b = av.astype(NP[dtype])[p], bv.astype(NP[dtype])[q]
    with np.errstate(invalid="ignore"):
        prod = np.minimum(a, b) if sr == "max_min" else a + b
        if sr == "max_min":  # (np.minimum hands a NaN of either side on, as the kernels' mul)
            assert np.array_equal(np.isnan(prod), np.isnan(a) | np.isnan(b))
    assert prod.dtype == NP[dtype] and cval.dtype == NP[dtype]
    c = cval[s]
    win = (prod == c) & (c != IDENTITY[sr])
    return win, np.bincount(s[win], minlength=len(cval)).astype(np.int64)


def shares(sr, pqs, win, av, bv, dtype):
    """The winning products and the fraction of their weight that goes to the A entry and to the B entry."""
    p, q, s = (x[win] for x in pqs)
    if sr != "max_min":
        one = np.ones(len(p))
        return p, q, s, one, one
    a, b = av.astype(NP[dtype])[p], bv.astype(NP[dtype])[q]
    return p, q, s, np.where(a < b, 1.0, np.where(a == b, 0.5, 0.0)), np.where(b < a, 1.0, np.where(a == b, 0.5, 0.0))


def exact_reference(sr, pqs, win, T, av, bv, G, nnzA, nnzB, dtype):
    """dA and dB where every weight and sum is exact (the exact regime): plain float64 sums, cast to the plan's type."""
    p, q, s, fa, fb = shares(sr, pqs, win, av, bv, dtype)
    w = G[s] / T[s]
    return (np.bincount(p, w * fa, nnzA).astype(NP[dtype]), np.bincount(q, w * fb, nnzB).astype(NP[dtype]))


def bound_reference(sr, pqs, win, T, av, bv, G, nnzA, nnzB, dtype):
    """Per side (ref, m, S): the long-double sum of the exact weights, the winning terms and their absolute sum."""
    p, q, s, fa, fb = shares(sr, pqs, win, av, bv, dtype)
    w = G.astype(NP[dtype])[s].astype(np.longdouble) / T[s].astype(np.longdouble)
    out = []
    for idx, f, n in ((p, fa, nnzA), (q, fb, nnzB)):
        on = f > 0
        t = w[on] * f[on].astype(np.longdouble)
        out.append((seg_sum_ld(idx[on], t, n), np.bincount(idx[on], minlength=n), seg_sum_ld(idx[on], np.abs(t), n)))
    return out


def assert_bound(got, ref, m, S, dtype, what):
    assert got.dtype == NP[dtype] and got.shape == ref.shape, what
    assert not np.isnan(got).any(), f"{what}: every entry is written"
    assert np.all(got[m == 0] == 0), f"{what}: entries no winner reaches are exactly 0"
    err = np.abs(got.astype(np.longdouble) - ref)
    bound = np.longdouble(1.01 * U[dtype]) * (m + 1).astype(np.longdouble) * S
    ratio = np.zeros(len(got), np.longdouble)
    np.divide(err, bound, out=ratio, where=bound > 0)
    worst = float(ratio.max(initial=0.0))
    print(f"subgrad bound, {what}: worst err / bound {worst:.3f} over {len(got)} entries, max m {m.max(initial=0)}")
    assert not (err > bound).any(), f"{what}: {(err > bound).sum()} entries outside 1.01 (m + 1) u S (worst {worst:.3e})"


# -------------------------------------------------------------------- the values ---
def exact_values(sr, A, B, seed):
    """Integers in [-3, 3]; about 2 % of both operands the identity of add (no edge), and some A entries the opposite
    infinity where their B row is all finite: no product is Inf - Inf, so the forward is bit-identical everywhere."""
    rng = np.random.default_rng(seed)
    av = rng.integers(-3, 4, A.nnz).astype(np.float64)
    bv = rng.integers(-3, 4, B.nnz).astype(np.float64)
    ident = IDENTITY[sr]
    av[rng.random(A.nnz) < 0.02] = ident
    bv[rng.random(B.nnz) < 0.02] = ident
    if sr == "max_min":  # min of any two values is a value: both infinities anywhere
        av[rng.random(A.nnz) < 0.01] = -ident
        bv[rng.random(B.nnz) < 0.01] = -ident
        return av, bv
    inf_row = np.zeros(B.M, bool)
    inf_row[np.repeat(np.arange(B.M), np.diff(B.ptr))[np.isinf(bv)]] = True
    cand = np.nonzero(~inf_row[A.col] & np.isfinite(av))[0]
    if len(cand):
        av[rng.choice(cand, max(1, len(cand) // 200), replace=False)] = -ident
    return av, bv


def call(tool, plan, nA, nB, nC, dtype, av, bv, G, cval=None, **kw):
    """One forward (unless cval is given) and one subgradient call into NaN-filled buffers; numpy results."""
    dA, dB, dG = fwd.dev(tool, av, dtype), fwd.dev(tool, bv, dtype), fwd.dev(tool, G, dtype)
    if cval is None:
        cval = fwd.nan_filled(tool, nC, dtype)
        plan.run(dA, dB, out=cval)
    oA, oB = fwd.nan_filled(tool, nA, dtype), fwd.nan_filled(tool, nB, dtype)
    ties = torch.full((nC,), -1, dtype=torch.int32, device=dG.device)
    gA, gB, gT = plan.subgrad(dG, cval, dA, dB, out_A=oA, out_B=oB, ties=ties, **kw)
    torch.cuda.synchronize()
    assert gT is ties and (gA is None or gA is oA) and (gB is None or gB is oB)
    return cval.cpu().numpy(), oA.cpu().numpy(), oB.cpu().numpy(), ties.cpu().numpy().astype(np.int64)


def forward_values(tool, plan, nC, dtype, av, bv):
    cval = fwd.nan_filled(tool, nC, dtype)
    plan.run(fwd.dev(tool, av, dtype), fwd.dev(tool, bv, dtype), out=cval)
    torch.cuda.synchronize()
    return cval


def check_exact(tool, plan, A, B, nC, pqs, sr, dtype, seed):
    av, bv = exact_values(sr, A, B, seed)
    cdev = forward_values(tool, plan, nC, dtype, av, bv)
    c = cdev.cpu().numpy()
    assert np.array_equal(c, fwd.reference(sr, pqs, av, bv, nC, dtype)), "the forward is bit-identical (no NaN product)"
    win, T = winners(sr, pqs, av, bv, c, dtype)
    reached = np.zeros(nC, bool)
    reached[pqs[2]] = True
    assert np.all(T[reached & (c != IDENTITY[sr])] >= 1), "a reached entry that is not the identity has a winner"
    g = np.random.default_rng(seed + 1).integers(-2, 3, nC).astype(np.float64)
    G = np.where(T > 0, T * g, np.nan)  # NaN where nothing wins: it must not be read
    _, gA, gB, ties = call(tool, plan, A.nnz, B.nnz, nC, dtype, av, bv, G, cval=cdev)
    assert np.array_equal(ties, T), "ties"
    assert np.all(ties[c == IDENTITY[sr]] == 0), "an entry equal to the identity has no winners"
    wA, wB = exact_reference(sr, pqs, win, T, av, bv, G, A.nnz, B.nnz, dtype)
    assert gA.dtype == NP[dtype] and np.array_equal(gA, wA), "dA"
    assert np.array_equal(gB, wB), "dB"
    mass = G[T > 0].sum()
    sA, sB = gA.astype(np.float64).sum(), gB.astype(np.float64).sum()
    assert abs(mass) < 2 ** 50 and np.abs(gA).sum() < 2 ** 50, "the sums below are exact in float64"
    if sr == "max_min":
        assert sA + sB == mass, "the gradient mass of an entry is G"
    else:
        assert sA == mass and sB == mass, "both operands get every entry's G"
    return T


def check_general(tool, plan, A, B, nC, pqs, sr, dtype, seed, what):
    av, bv, G = fwd.sr_values(A.nnz, seed), fwd.sr_values(B.nnz, seed + 1000), fwd.sr_values(nC, seed + 2000)
    c, gA, gB, ties = call(tool, plan, A.nnz, B.nnz, nC, dtype, av, bv, G)
    assert np.array_equal(c, fwd.reference(sr, pqs, av, bv, nC, dtype))
    win, T = winners(sr, pqs, av, bv, c, dtype)
    assert np.array_equal(ties, T), "ties"
    (rA, mA, SA), (rB, mB, SB) = bound_reference(sr, pqs, win, T, av, bv, G, A.nnz, B.nnz, dtype)
    assert_bound(gA, rA, mA, SA, dtype, f"{what}, dA")
    assert_bound(gB, rB, mB, SB, dtype, f"{what}, dB")
    _, gA2, _, ties2 = call(tool, plan, A.nnz, B.nnz, nC, dtype, av, bv, G)
    assert gA2.tobytes() == gA.tobytes() and np.array_equal(ties2, ties), "dA has a fixed order: two calls, the same bits"


def check_case(tool, A, B, Cp, Ci, pqs, sr, dtype, seed, masked=False, form="auto"):
    """Both regimes on one plan of `sr` and `dtype`; returns info()."""
    dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, masked=masked, form=form, dtype=dtype, semiring=sr)
    try:
        info = plan.info()
        check_exact(tool, plan, A, B, len(Ci), pqs, sr, dtype, seed)
        check_general(tool, plan, A, B, len(Ci), pqs, sr, dtype, seed + 7, f"{sr} {dtype}")
    finally:
        plan.close()
    assert info["semiring"] == sr and info["dtype"] == dtype and info["width"] == 1
    return info


# 1. the zoos: every class between them
@pytest.mark.parametrize("sr", SEMIRINGS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("bin_zoo", "tiny_zoo"))
def test_subgrad_zoos(tool, name, dtype, sr):
    A, B, Cp, Ci, pqs = fwd.case(name)
    info = check_case(tool, A, B, Cp, Ci, pqs, sr, dtype, 100)
    dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
    assert fwd.same_classes(info, fwd.plus_times_info(tool, dA, dB, dC, dtype)), "info() is the plus-times plan's"
    if name == "bin_zoo":
        assert info["rows"][GLOBAL] >= 1, info


def test_subgrad_every_class_has_rows(tool):
    rows = np.zeros(8, np.int64)
    for name in ("bin_zoo", "tiny_zoo"):
        A, B, Cp, Ci, _ = fwd.case(name)
        dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
        plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, semiring="max_plus")
        try:
            rows += plan.info()["rows"]
        finally:
            plan.close()
    for cls in (TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL):
        assert rows[cls] > 0, f"class {cls} has no rows in bin_zoo + tiny_zoo"


# 2. stage boundaries: A rows of 65, 257 and 700 entries among them
@pytest.mark.parametrize("sr", SEMIRINGS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_subgrad_stage_boundaries(tool, dtype, sr):
    A, B, Cp, Ci, pqs = fwd.many_a_entries()
    assert {65, 257, 700} <= set(np.diff(A.ptr).tolist())
    info = check_case(tool, A, B, Cp, Ci, pqs, sr, dtype, 200)
    assert info["rows"][WAVE_DIRECT] >= 1 and info["rows"][BLOCK_DIRECT] + info["rows"][BLOCK_SEARCH] >= 1, info


# 3. golden cases: duplicates in A and B (each a product of its own), a rectangular pair, an empty product
@pytest.mark.parametrize("sr", SEMIRINGS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("duplicates", "rect_AB", "empty_product"))
def test_subgrad_golden(tool, name, dtype, sr):
    A, B, Cp, Ci, pqs = fwd.case(name)
    if name == "empty_product":
        assert len(pqs[0]) == 0
    if name == "duplicates":
        assert any(len(np.unique(X.col[X.ptr[i]:X.ptr[i + 1]])) < X.ptr[i + 1] - X.ptr[i] for X in (A, B) for i in range(X.M))
    check_case(tool, A, B, Cp, Ci, pqs, sr, dtype, 300)


# 4. C's pattern a strict superset of the product's, with one product-empty row
@pytest.mark.parametrize("dtype", DTYPES)
def test_subgrad_superset_pattern(tool, dtype):
    A, B, Cp, Ci, pqs, is_extra = fwd.superset_case()
    for sr in SEMIRINGS:
        dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
        plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, dtype=dtype, semiring=sr)
        try:
            T = check_exact(tool, plan, A, B, len(Ci), pqs, sr, dtype, 400)
            assert np.all(T[is_extra] == 0) and T[~is_extra].sum() > 0
            check_general(tool, plan, A, B, len(Ci), pqs, sr, dtype, 407, f"superset {sr} {dtype}")
        finally:
            plan.close()


# 5. masked plans, every form: a thinned mask with stranger columns, and L*L on L with n = 3000
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ("product", "dot", "auto"))
@pytest.mark.parametrize("name", ("rect", "triangle"))
def test_subgrad_masked(tool, name, form, dtype):
    A, B, Mp, Mc, pqs = fwd.mask_case(name)
    assert len(pqs[0]) < orc.flop(A.col, B.ptr), "the case needs products outside the mask"
    if name == "triangle":
        assert A.M == 3000 and B is A
    for sr in SEMIRINGS:
        info = check_case(tool, A, B, Mp, Mc, pqs, sr, dtype, 500, masked=True, form=form)
        assert info["kept_products"] == len(pqs[0])
        if form == "dot":
            assert info["rows"][DOT] > 0
        if form == "product":
            assert info["rows"][DOT] == 0


# 6. an independent oracle: CPU torch autograd of amin / amax over the dense products, on a tiny case with ties
@functools.lru_cache(maxsize=None)
def tiny_case():
    M, K, N = 37, 29, 40
    rng = np.random.default_rng(61)

    def pattern(R, Cn, density):
        keep = rng.random((R, Cn)) < density
        ptr = np.zeros(R + 1, np.int64)
        np.cumsum(keep.sum(1), out=ptr[1:])
        return ptr.astype(np.int32), np.nonzero(keep)[1].astype(np.int32)

    Ap, Ac = pattern(M, K, 0.3)
    Bp, Bc = pattern(K, N, 0.3)
    A = mhspgemm.CSR(M, K, Ap, Ac, np.ones(len(Ac)))
    B = mhspgemm.CSR(K, N, Bp, Bc, np.ones(len(Bc)))
    Cp, Ci, _ = orc.spgemm(A.ptr, A.col, A.val, B.ptr, B.col, B.val, N)
    return A, B, Cp, Ci, expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, N)


@pytest.mark.parametrize("sr", SEMIRINGS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_subgrad_against_torch_autograd(tool, dtype, sr):
    A, B, Cp, Ci, pqs = tiny_case()
    assert max(A.M, A.N, B.N) <= 40 and len(Ci) > 100
    rng = np.random.default_rng(62)
    small = np.array([-1.5, -0.5, 0.25, 1.0, 2.0])  # a small set: sums and minima collide
    av, bv, G = rng.choice(small, A.nnz), rng.choice(small, B.nnz), fwd.sr_values(len(Ci), 63)
    tdt = getattr(torch, dtype)
    # the library's side
    dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, dtype=dtype, semiring=sr)
    try:
        ta = fwd.dev(tool, av, dtype).requires_grad_(True)
        tb = fwd.dev(tool, bv, dtype).requires_grad_(True)
        out = plan.apply_subgrad(ta, tb)
        out.backward(fwd.dev(tool, G, dtype))
        torch.cuda.synchronize()
        c, gA, gB = out.detach().cpu().numpy(), ta.grad.cpu().numpy(), tb.grad.cpu().numpy()
    finally:
        plan.close()
    # torch's side, dense on the CPU: missing entries at the identity's infinity
    miss = float(IDENTITY[sr])
    ca = torch.tensor(av, dtype=tdt, requires_grad=True)
    cb = torch.tensor(bv, dtype=tdt, requires_grad=True)
    rowsA = torch.from_numpy(np.repeat(np.arange(A.M), np.diff(A.ptr)))
    rowsB = torch.from_numpy(np.repeat(np.arange(B.M), np.diff(B.ptr)))
    Ad = torch.full((A.M, A.N), miss, dtype=tdt).index_put((rowsA, torch.from_numpy(A.col.astype(np.int64))), ca)
    Bd = torch.full((B.M, B.N), miss, dtype=tdt).index_put((rowsB, torch.from_numpy(B.col.astype(np.int64))), cb)
    if sr == "max_min":
        dense = torch.minimum(Ad[:, :, None], Bd[None]).amax(1)
    else:
        P = Ad[:, :, None] + Bd[None]
        dense = P.amin(1) if sr == "min_plus" else P.amax(1)
    rowsC = torch.from_numpy(np.repeat(np.arange(A.M), np.diff(Cp)))
    want = dense[rowsC, torch.from_numpy(Ci.astype(np.int64))]
    want.backward(torch.tensor(G, dtype=tdt))
    assert np.array_equal(c, want.detach().numpy()), "the forward"
    win, T = winners(sr, pqs, av, bv, c, dtype)
    assert (T > 1).sum() > 10, "the case needs ties"
    (_, mA, SA), (_, mB, SB) = bound_reference(sr, pqs, win, T, av, bv, G, A.nnz, B.nnz, dtype)
    assert_bound(gA, ca.grad.numpy().astype(np.longdouble), mA, SA, dtype, f"torch {sr} {dtype}, dA")
    assert_bound(gB, cb.grad.numpy().astype(np.longdouble), mB, SB, dtype, f"torch {sr} {dtype}, dB")


# 7. one-sided calls write only their side
@pytest.mark.parametrize("dtype", DTYPES)
def test_subgrad_one_sided(tool, dtype):
    A, B, Cp, Ci, pqs = fwd.small_pair()
    dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, dtype=dtype, semiring="max_min")
    try:
        av, bv, G = fwd.sr_values(A.nnz, 71), fwd.sr_values(B.nnz, 1071), fwd.sr_values(len(Ci), 2071)
        c, gA, gB, ties = call(tool, plan, A.nnz, B.nnz, len(Ci), dtype, av, bv, G)
        _, oA, xB, tA = call(tool, plan, A.nnz, B.nnz, len(Ci), dtype, av, bv, G, need_B=False)
        _, xA, oB, tB = call(tool, plan, A.nnz, B.nnz, len(Ci), dtype, av, bv, G, need_A=False)
        assert np.isnan(xB).all() and np.isnan(xA).all(), "the side not asked for keeps its bytes"
        assert oA.tobytes() == gA.tobytes() and np.array_equal(tA, ties) and np.array_equal(tB, ties)
        win, T = winners("max_min", pqs, av, bv, c, dtype)
        (_, _, _), (rB, mB, SB) = bound_reference("max_min", pqs, win, T, av, bv, G, A.nnz, B.nnz, dtype)
        assert_bound(oB, rB, mB, SB, dtype, f"dB alone {dtype}")
        assert (gA != 0).any() and (gB != 0).any() and np.array_equal(ties, T)
        with pytest.raises(ValueError, match="need_A or need_B"):
            plan.subgrad(fwd.dev(tool, G, dtype), fwd.dev(tool, c, dtype), fwd.dev(tool, av, dtype), fwd.dev(tool, bv, dtype),
                         need_A=False, need_B=False)
    finally:
        plan.close()


# 8. refusals: a plus_times plan has a gradient; the wrong type; missing arrays; the four backward entry points keep refusing
def test_subgrad_refusals(tool):
    A, B, Cp, Ci, _ = fwd.small_pair()
    dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
    av, bv, G = fwd.dev(tool, fwd.sr_values(A.nnz, 81)), fwd.dev(tool, fwd.sr_values(B.nnz, 1081)), fwd.dev(tool, fwd.sr_values(len(Ci), 82))
    L = _lib.lib()
    refused = (mhspgemm.MHSpGEMMError, ValueError)
    plain = mhspgemm.ValuesPlan(tool, dA, dB, dC)
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, semiring="min_plus")
    try:
        oA, oB = filled(tool, A.nnz), filled(tool, B.nnz)
        ties = torch.full((len(Ci),), -1, dtype=torch.int32, device=G.device)
        with pytest.raises(refused, match="plus_times") as e:
            plain.subgrad(G, G, av, bv, out_A=oA, out_B=oB, ties=ties)
        assert "mhs_spgemm_values_grad" in str(e.value)
        with pytest.raises(refused, match="plus_times"):
            plain.apply_subgrad(av.clone().requires_grad_(True), bv)
        x, t = G.data_ptr(), ties.data_ptr()
        assert L.mhs_spgemm_values_subgrad(tool.ctx, plain.plan, x, x, x, x, t, oA.data_ptr(), oB.data_ptr(), None) == 3
        msg = L.mhs_last_error(tool.ctx)
        assert b"plus_times" in msg and b"mhs_spgemm_values_grad" in msg
        # on the semiring plan: the wrong type, a needed array NULL, both outputs NULL, a NULL plan
        assert L.mhs_spgemm_values_subgrad_f32(tool.ctx, plan.plan, x, x, x, x, t, oA.data_ptr(), oB.data_ptr(), None) == 3
        msg = L.mhs_last_error(tool.ctx)
        assert b"FP64" in msg and b"FP32" in msg
        for hole in range(5):
            args = [x, x, x, x, t]
            args[hole] = None
            assert L.mhs_spgemm_values_subgrad(tool.ctx, plan.plan, *args, oA.data_ptr(), oB.data_ptr(), None) == 3, hole
        assert L.mhs_spgemm_values_subgrad(tool.ctx, plan.plan, x, x, x, x, t, None, None, None) == 3
        assert b"no output" in L.mhs_last_error(tool.ctx)
        assert L.mhs_spgemm_values_subgrad(tool.ctx, None, x, x, x, x, t, oA.data_ptr(), oB.data_ptr(), None) == 3
        # the existing backward keeps refusing the semiring plan
        with pytest.raises(refused, match="min_plus"):
            plan.grad(G, av, bv, out_A=oA, out_B=oB)
        with pytest.raises(refused, match="min_plus"):
            plan.apply(av.clone().requires_grad_(True), bv)
        torch.cuda.synchronize()
        assert torch.isnan(oA).all() and torch.isnan(oB).all() and (ties == -1).all(), "a refused call writes nothing"
    finally:
        plan.close()
        plain.close()


# 9. unsynchronised use: MHS_OPT_SYNC 0 on a torch stream, forward and subgradient queued back to back
def test_subgrad_stream_ordered(tool):
    A, B, Cp, Ci, pqs = fwd.small_pair()
    dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
    sr, dtype, nC = "max_plus", "float64", len(Ci)
    av, bv, G = fwd.sr_values(A.nnz, 91), fwd.sr_values(B.nnz, 1091), fwd.sr_values(nC, 2091)
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, semiring=sr)
    ta, tb, tg = fwd.dev(tool, av), fwd.dev(tool, bv), fwd.dev(tool, G)
    cval, oA, oB = filled(tool, nC), filled(tool, A.nnz), filled(tool, B.nnz)
    ties = torch.full((nC,), -1, dtype=torch.int32, device=tg.device)
    stream = torch.cuda.Stream(device=tool.device)
    tool.set_option(_lib.MHS_OPT_SYNC, 0)
    tool.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            assert plan.run(ta, tb, out=cval) is None
            plan.subgrad(tg, cval, ta, tb, out_A=oA, out_B=oB, ties=ties)
        torch.cuda.synchronize()
        c, gA, gB, t = cval.cpu().numpy(), oA.cpu().numpy(), oB.cpu().numpy(), ties.cpu().numpy().astype(np.int64)
    finally:
        tool.set_option(_lib.MHS_OPT_SYNC, 1)
        tool.set_stream(None)
        plan.close()
    assert np.array_equal(c, fwd.reference(sr, pqs, av, bv, nC))
    win, T = winners(sr, pqs, av, bv, c, dtype)
    assert np.array_equal(t, T)
    (rA, mA, SA), (rB, mB, SB) = bound_reference(sr, pqs, win, T, av, bv, G, A.nnz, B.nnz, dtype)
    assert_bound(gA, rA, mA, SA, dtype, "stream-ordered, dA")
    assert_bound(gB, rB, mB, SB, dtype, "stream-ordered, dB")
