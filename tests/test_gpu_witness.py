"""GPU tests of the semiring witness (mhspgemm.ValuesPlan.witness / run_arg over mhs_spgemm_values_witness): the arg of
min-plus, max-plus and max-min plans in every row class, FP64 and FP32, on kept patterns and masks.

The reference is numpy over _util.expand's kept products (A entry p, B entry q, C slot s), on the shapes the forward's
and the subgradient's tests (test_gpu_semiring.py, test_gpu_subgrad.py) already prove reach every code path -- their
cached cases and the subgradient's winner rule (test_gpu_subgrad.winners) are shared.  wit[s] is the smallest
A.col[p] among the winners of s and -1 where s has none.  The result is a minimum of integers: every comparison is
np.array_equal and nothing has a tolerance.  Two regimes, both run on one plan per case:

exact    the subgradient's exact_values: integers in [-3, 3] with a few +-Inf operands, so ties are frequent -- a case
         is asserted to have entries with winners of different k, or it says nothing about "smallest".
general  the forward tests' sr_values (signed, magnitudes in [0.1, 1000]): ties are rare.
Every wit buffer starts as 12345: an entry the call leaves alone shows."""
import numpy as np
import pytest
import torch

import mhspgemm
from mhspgemm import _lib
from oracle import oracle as orc
import test_gpu_semiring as fwd
import test_gpu_subgrad as sub

pytestmark = pytest.mark.gpu

TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL, DOT = 1, 2, 3, 4, 5, 6, 7
SEMIRINGS = fwd.SEMIRINGS
IDENTITY = fwd.IDENTITY
NP = fwd.NP
DTYPES = ("float64", "float32")
JUNK = 12345


# ------------------------------------------------------------------ the reference ---
def witness_reference(sr, A, pqs, av, bv, cval, dtype):
    """(ref, spread): per C entry the smallest A.col[p] among its winners (-1: none), and whether its winners have
    more than one k."""
    win, T = sub.winners(sr, pqs, av, bv, cval, dtype)
    k = A.col[pqs[0][win]].astype(np.int64)
    s = pqs[2][win]
    lo = np.full(len(cval), np.iinfo(np.int64).max, np.int64)
    hi = np.full(len(cval), -1, np.int64)
    np.minimum.at(lo, s, k)
    np.maximum.at(hi, s, k)
    ref = np.full(len(cval), -1, np.int64)
    ref[T > 0] = lo[T > 0]
    return ref.astype(np.int32), (T > 0) & (hi > lo)


def junk(tool, n):
    t = torch.full((n,), JUNK, dtype=torch.int32, device=f"cuda:{tool.device}")
    torch.cuda.synchronize()
    return t


def call(tool, plan, nC, dtype, av, bv, cval=None):
    """One forward (unless cval is given) and one witness call into a junk-filled buffer; numpy results."""
    dA, dB = fwd.dev(tool, av, dtype), fwd.dev(tool, bv, dtype)
    if cval is None:
        cval = fwd.nan_filled(tool, nC, dtype)
        plan.run(dA, dB, out=cval)
    wit = junk(tool, nC)
    got = plan.witness(cval, dA, dB, out=wit)
    torch.cuda.synchronize()
    assert got is wit
    w = wit.cpu().numpy()
    assert w.dtype == np.int32
    return cval.cpu().numpy(), w


def check_exact(tool, plan, A, B, nC, pqs, sr, dtype, seed):
    """The exact regime; returns the entries whose winners have more than one k."""
    av, bv = sub.exact_values(sr, A, B, seed)
    c, w = call(tool, plan, nC, dtype, av, bv)
    assert np.array_equal(c, fwd.reference(sr, pqs, av, bv, nC, dtype)), "the forward is bit-identical (no NaN product)"
    ref, spread = witness_reference(sr, A, pqs, av, bv, c, dtype)
    assert np.array_equal(w, ref), "wit"
    assert np.all(w[c == IDENTITY[sr]] == -1), "an entry equal to the identity has no witness"
    return int(spread.sum())


def check_general(tool, plan, A, B, nC, pqs, sr, dtype, seed):
    av, bv = fwd.sr_values(A.nnz, seed), fwd.sr_values(B.nnz, seed + 1000)
    c, w = call(tool, plan, nC, dtype, av, bv)
    assert np.array_equal(c, fwd.reference(sr, pqs, av, bv, nC, dtype))
    ref, _ = witness_reference(sr, A, pqs, av, bv, c, dtype)
    assert np.array_equal(w, ref), "wit"
    reached = np.zeros(nC, bool)
    reached[pqs[2]] = True
    assert np.array_equal(w >= 0, reached), "finite values: exactly the reached entries have a witness"


def check_case(tool, A, B, Cp, Ci, pqs, sr, dtype, seed, masked=False, form="auto"):
    """Both regimes on one plan of `sr` and `dtype`; returns (info(), the exact regime's entries with several k)."""
    dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, masked=masked, form=form, dtype=dtype, semiring=sr)
    try:
        info = plan.info()
        spread = check_exact(tool, plan, A, B, len(Ci), pqs, sr, dtype, seed)
        check_general(tool, plan, A, B, len(Ci), pqs, sr, dtype, seed + 7)
    finally:
        plan.close()
    assert info["semiring"] == sr and info["dtype"] == dtype and info["width"] == 1
    return info, spread


# 1. the zoos: every class between them
@pytest.mark.parametrize("sr", SEMIRINGS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("bin_zoo", "tiny_zoo"))
def test_witness_zoos(tool, name, dtype, sr):
    A, B, Cp, Ci, pqs = fwd.case(name)
    info, spread = check_case(tool, A, B, Cp, Ci, pqs, sr, dtype, 100)
    assert spread > 0, "the case needs entries whose winners have different k"
    if name == "bin_zoo":
        assert info["rows"][GLOBAL] >= 1, info


def test_witness_every_class_has_rows(tool):
    rows = np.zeros(8, np.int64)
    for name in ("bin_zoo", "tiny_zoo"):
        A, B, Cp, Ci, _ = fwd.case(name)
        dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
        plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, semiring="max_min")
        try:
            assert hasattr(plan, "witness")
            rows += plan.info()["rows"]
        finally:
            plan.close()
    for cls in (TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL):
        assert rows[cls] > 0, f"class {cls} has no rows in bin_zoo + tiny_zoo"


# 2. stage boundaries: A rows of 65, 257 and 700 entries among them -- the stage is filled again inside a row, and a
# wrong entry index would give a neighbour's column
@pytest.mark.parametrize("sr", SEMIRINGS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_witness_stage_boundaries(tool, dtype, sr):
    A, B, Cp, Ci, pqs = fwd.many_a_entries()
    assert {65, 257, 700} <= set(np.diff(A.ptr).tolist())
    info, spread = check_case(tool, A, B, Cp, Ci, pqs, sr, dtype, 200)
    assert spread > 0, "the case needs entries whose winners have different k"
    assert info["rows"][WAVE_DIRECT] >= 1 and info["rows"][BLOCK_DIRECT] + info["rows"][BLOCK_SEARCH] >= 1, info


# 3. golden cases: duplicates in A and B (they share their k), a rectangular pair, an empty product
@pytest.mark.parametrize("sr", SEMIRINGS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("duplicates", "rect_AB", "empty_product"))
def test_witness_golden(tool, name, dtype, sr):
    A, B, Cp, Ci, pqs = fwd.case(name)
    if name == "duplicates":
        assert any(len(np.unique(X.col[X.ptr[i]:X.ptr[i + 1]])) < X.ptr[i + 1] - X.ptr[i] for X in (A, B) for i in range(X.M))
    check_case(tool, A, B, Cp, Ci, pqs, sr, dtype, 300)
    if name == "empty_product":
        assert len(pqs[0]) == 0
        dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
        plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, dtype=dtype, semiring=sr)
        try:
            _, w = call(tool, plan, len(Ci), dtype, fwd.sr_values(A.nnz, 301), fwd.sr_values(B.nnz, 1301))
        finally:
            plan.close()
        assert np.array_equal(w, np.full(len(Ci), -1, np.int32)), "no product: every entry is -1"


# 4. C's pattern a strict superset of the product's, with one product-empty row
@pytest.mark.parametrize("dtype", DTYPES)
def test_witness_superset_pattern(tool, dtype):
    A, B, Cp, Ci, pqs, is_extra = fwd.superset_case()
    EMPTY = 7
    assert A.ptr[EMPTY + 1] == A.ptr[EMPTY] and Cp[EMPTY + 1] > Cp[EMPTY]
    for sr in SEMIRINGS:
        dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
        plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, dtype=dtype, semiring=sr)
        try:
            check_exact(tool, plan, A, B, len(Ci), pqs, sr, dtype, 400)
            check_general(tool, plan, A, B, len(Ci), pqs, sr, dtype, 407)
            _, w = call(tool, plan, len(Ci), dtype, fwd.sr_values(A.nnz, 407), fwd.sr_values(B.nnz, 1407))
        finally:
            plan.close()
        assert np.all(w[is_extra] == -1) and np.all(w[~is_extra] >= 0)
        assert np.all(w[Cp[EMPTY]:Cp[EMPTY + 1]] == -1), "the product-empty row"


# 5. masked plans, every form: a thinned mask with stranger columns, and L*L on L with n = 3000
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ("product", "dot", "auto"))
@pytest.mark.parametrize("name", ("rect", "triangle"))
def test_witness_masked(tool, name, form, dtype):
    A, B, Mp, Mc, pqs = fwd.mask_case(name)
    assert len(pqs[0]) < orc.flop(A.col, B.ptr), "the case needs products outside the mask"
    if name == "triangle":
        assert A.M == 3000 and B is A
    for sr in SEMIRINGS:
        info, spread = check_case(tool, A, B, Mp, Mc, pqs, sr, dtype, 500, masked=True, form=form)
        assert spread > 0, "the case needs entries whose winners have different k"
        assert info["kept_products"] == len(pqs[0])
        if form == "dot":
            assert info["rows"][DOT] > 0
        if form == "product":
            assert info["rows"][DOT] == 0


# 6. consistency with the subgradient: an entry has a witness exactly where it has winners
@pytest.mark.parametrize("sr,name", (("min_plus", "bin_zoo"), ("max_plus", "tiny_zoo"), ("max_min", "bin_zoo")))
def test_witness_consistent_with_ties(tool, sr, name):
    A, B, Cp, Ci, pqs = fwd.case(name)
    nC, dtype = len(Ci), "float64"
    dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, semiring=sr)
    try:
        av, bv = sub.exact_values(sr, A, B, 600)
        cdev = sub.forward_values(tool, plan, nC, dtype, av, bv)
        _, _, _, ties = sub.call(tool, plan, A.nnz, B.nnz, nC, dtype, av, bv, np.ones(nC), cval=cdev)
        _, w = call(tool, plan, nC, dtype, av, bv, cval=cdev)
    finally:
        plan.close()
    assert np.array_equal(w >= 0, ties >= 1)
    assert (ties == 0).any() and (ties >= 2).any(), "the case needs entries without winners and entries with ties"


# 7. an independent oracle: argmin / argmax over the dense [M, K, N] products, which shares nothing with expand or
# winners; np.argmin and np.argmax return the first occurrence, the smallest k
@pytest.mark.parametrize("sr", SEMIRINGS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_witness_against_dense_arg(tool, dtype, sr):
    A, B, Cp, Ci, _ = sub.tiny_case()
    assert max(A.M, A.N, B.N) <= 40 and len(Ci) > 100
    rng = np.random.default_rng(72)
    av, bv = rng.integers(-3, 4, A.nnz).astype(np.float64), rng.integers(-3, 4, B.nnz).astype(np.float64)
    dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, dtype=dtype, semiring=sr)
    try:
        c, w = call(tool, plan, len(Ci), dtype, av, bv)
    finally:
        plan.close()
    miss = NP[dtype](IDENTITY[sr])
    Ad, Bd = np.full((A.M, A.N), miss, NP[dtype]), np.full((B.M, B.N), miss, NP[dtype])
    Ad[np.repeat(np.arange(A.M), np.diff(A.ptr)), A.col] = av
    Bd[np.repeat(np.arange(B.M), np.diff(B.ptr)), B.col] = bv
    P = np.minimum(Ad[:, :, None], Bd[None]) if sr == "max_min" else Ad[:, :, None] + Bd[None]
    assert P.dtype == NP[dtype] and P.shape == (A.M, A.N, B.N)
    arg = P.argmin(1) if sr == "min_plus" else P.argmax(1)
    val = P.min(1) if sr == "min_plus" else P.max(1)
    arg = np.where(val == miss, -1, arg).astype(np.int32)
    rows = np.repeat(np.arange(A.M), np.diff(Cp))
    assert np.array_equal(c, val[rows, Ci]), "the forward"
    assert np.array_equal(w, arg[rows, Ci]), "wit"
    several = (P == val[:, None, :]).sum(1)[rows, Ci]
    assert (several[w >= 0] > 1).sum() > 10, "the case needs ties"


# 8. the witness is usable: through wit[s] = k there is an A entry (i, k) and a B entry (k, j) whose mul is Cval[s]
@pytest.mark.parametrize("sr", SEMIRINGS)
@pytest.mark.parametrize("name", ("duplicates", "small_pair"))
def test_witness_is_usable(tool, name, sr):
    A, B, Cp, Ci, pqs = fwd.small_pair() if name == "small_pair" else fwd.case(name)
    dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, semiring=sr)
    try:
        av, bv = sub.exact_values(sr, A, B, 800)
        c, w = call(tool, plan, len(Ci), "float64", av, bv)
    finally:
        plan.close()
    assert (w >= 0).any()
    rows = np.repeat(np.arange(A.M), np.diff(Cp))
    for s in np.nonzero(w >= 0)[0]:
        i, j, k = rows[s], Ci[s], w[s]
        a = av[A.ptr[i]:A.ptr[i + 1]][A.col[A.ptr[i]:A.ptr[i + 1]] == k]
        b = bv[B.ptr[k]:B.ptr[k + 1]][B.col[B.ptr[k]:B.ptr[k + 1]] == j]
        assert len(a) and len(b), (s, i, j, k)
        prod = np.minimum(a[:, None], b[None]) if sr == "max_min" else a[:, None] + b[None]
        assert (prod == c[s]).any(), (s, i, j, k)


# 9. identity, NaN, determinism
def test_witness_all_identity_row(tool):
    A, B, Cp, Ci, pqs = fwd.small_pair()
    dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
    av, bv = fwd.sr_values(A.nnz, 41), fwd.sr_values(B.nnz, 1041)
    row = int(np.argmax(np.diff(A.ptr) >= 3))  # a row all of whose products are +Inf: "no path"
    for k in A.col[A.ptr[row]:A.ptr[row + 1]]:
        bv[B.ptr[k]:B.ptr[k + 1]] = np.inf
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, semiring="min_plus")
    try:
        c, w = call(tool, plan, len(Ci), "float64", av, bv)
    finally:
        plan.close()
    assert Cp[row + 1] > Cp[row] and np.all(c[Cp[row]:Cp[row + 1]] == np.inf)
    assert np.all(w[Cp[row]:Cp[row + 1]] == -1), "an entry whose products are all the identity has no witness"
    ref, _ = witness_reference("min_plus", A, pqs, av, bv, c, "float64")
    assert np.array_equal(w, ref) and (w >= 0).sum() > 0.5 * len(w)


@pytest.mark.parametrize("sr", SEMIRINGS)
def test_witness_nan_containment(tool, sr):
    A, B, Cp, Ci, pqs = fwd.small_pair()
    dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
    av, bv = fwd.sr_values(A.nnz, 51), fwd.sr_values(B.nnz, 1051)
    p0 = int(A.ptr[int(np.argmax(np.diff(A.ptr) >= 4))] + 1)
    clean = av.copy()
    av[p0] = np.nan
    uses = pqs[0] == p0
    touched = np.zeros(len(Ci), bool)
    touched[pqs[2][uses]] = True
    assert 0 < touched.sum() < 0.1 * len(Ci)
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, semiring=sr)
    try:
        c, w = call(tool, plan, len(Ci), "float64", av, bv)
    finally:
        plan.close()
    # the reference without that entry's products: the rest of the products, with the entry's value finite again
    rest = tuple(x[~uses] for x in pqs)
    crest = fwd.reference(sr, pqs, clean, bv, len(Ci), skip=uses)
    ref, _ = witness_reference(sr, A, rest, clean, bv, crest, "float64")
    assert np.array_equal(c[~touched], crest[~touched])
    assert np.array_equal(w[~touched], ref[~touched]), "a NaN product reaches no other entry's witness"
    # a touched entry: -1, or the k of a winner that is not a NaN product
    p, q, s = rest
    prod = np.minimum(clean[p], bv[q]) if sr == "max_min" else clean[p] + bv[q]
    good = np.zeros(len(Ci), bool)
    good[s[(prod == c[s]) & (A.col[p] == w[s])]] = True
    assert np.all((w[touched] == -1) | good[touched])
    assert np.all(w[np.isnan(c)] == -1), "a NaN entry has no witness"


@pytest.mark.parametrize("dtype", DTYPES)
def test_witness_two_calls_same_bytes(tool, dtype):
    for name, sr in (("bin_zoo", "max_plus"), ("tiny_zoo", "max_min")):
        A, B, Cp, Ci, pqs = fwd.case(name)
        dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
        plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, dtype=dtype, semiring=sr)
        try:
            av, bv = sub.exact_values(sr, A, B, 900)
            cdev = sub.forward_values(tool, plan, len(Ci), dtype, av, bv)
            _, w1 = call(tool, plan, len(Ci), dtype, av, bv, cval=cdev)
            _, w2 = call(tool, plan, len(Ci), dtype, av, bv, cval=cdev)
        finally:
            plan.close()
        assert w1.tobytes() == w2.tobytes() and (w1 >= 0).any() and not (w1 == JUNK).any()


# 10. refusals: a sum has no witness; the wrong type; missing arrays; a closed plan
def test_witness_refusals(tool):
    A, B, Cp, Ci, _ = fwd.small_pair()
    dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
    av, bv, cv = fwd.dev(tool, fwd.sr_values(A.nnz, 81)), fwd.dev(tool, fwd.sr_values(B.nnz, 1081)), fwd.dev(tool, fwd.sr_values(len(Ci), 82))
    L = _lib.lib()
    refused = (mhspgemm.MHSpGEMMError, ValueError)
    plain = mhspgemm.ValuesPlan(tool, dA, dB, dC)
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, semiring="min_plus")
    plan32 = mhspgemm.ValuesPlan(tool, dA, dB, dC, dtype="float32", semiring="min_plus")
    closed = mhspgemm.ValuesPlan(tool, dA, dB, dC, semiring="max_min")
    closed.close()
    try:
        wit = junk(tool, len(Ci))
        with pytest.raises(refused, match="plus_times") as e:
            plain.witness(cv, av, bv, out=wit)
        assert "no witness" in str(e.value)
        with pytest.raises(refused, match="plus_times"):
            plain.run_arg(av, bv)
        x, t = cv.data_ptr(), wit.data_ptr()
        assert L.mhs_spgemm_values_witness(tool.ctx, plain.plan, x, x, x, t, None) == 3
        msg = L.mhs_last_error(tool.ctx)
        assert b"plus_times" in msg and b"no witness" in msg
        # the wrong type, in both directions
        assert L.mhs_spgemm_values_witness_f32(tool.ctx, plan.plan, x, x, x, t, None) == 3
        msg = L.mhs_last_error(tool.ctx)
        assert b"FP64" in msg and b"FP32" in msg
        assert L.mhs_spgemm_values_witness(tool.ctx, plan32.plan, x, x, x, t, None) == 3
        msg = L.mhs_last_error(tool.ctx)
        assert b"FP64" in msg and b"FP32" in msg
        with pytest.raises(refused, match="float32"):
            plan32.witness(cv, av, bv, out=wit)
        with pytest.raises(refused, match="float64"):
            plan.witness(cv.float(), av, bv, out=wit)
        # each array NULL, a NULL plan
        for hole in range(4):
            args = [x, x, x, t]
            args[hole] = None
            assert L.mhs_spgemm_values_witness(tool.ctx, plan.plan, *args, None) == 3, hole
            assert b"null" in L.mhs_last_error(tool.ctx)
        assert L.mhs_spgemm_values_witness(tool.ctx, None, x, x, x, t, None) == 3
        # a closed plan, and an output of the wrong kind
        with pytest.raises(mhspgemm.MHSpGEMMError, match="closed"):
            closed.witness(cv, av, bv, out=wit)
        with pytest.raises(ValueError, match="int32"):
            plan.witness(cv, av, bv, out=cv)
        torch.cuda.synchronize()
        assert (wit == JUNK).all(), "a refused call writes nothing"
    finally:
        plan.close()
        plan32.close()
        plain.close()


# 11. unsynchronised use: MHS_OPT_SYNC 0 on a torch stream, forward and witness queued back to back by run_arg
def test_witness_stream_ordered(tool):
    A, B, Cp, Ci, pqs = fwd.small_pair()
    dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
    sr, dtype, nC = "max_plus", "float64", len(Ci)
    av, bv = sub.exact_values(sr, A, B, 91)
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, semiring=sr)
    ta, tb, ta2 = fwd.dev(tool, av), fwd.dev(tool, bv), fwd.dev(tool, av + 1.0)
    stream = torch.cuda.Stream(device=tool.device)
    tool.set_option(_lib.MHS_OPT_SYNC, 0)
    try:
        with torch.cuda.stream(stream):
            cval, wit = plan.run_arg(ta, tb)
            cval2, wit2 = plan.run_arg(ta2, tb)  # queued behind, nothing waited for in between
        torch.cuda.synchronize()
        c, w, c2, w2 = cval.cpu().numpy(), wit.cpu().numpy(), cval2.cpu().numpy(), wit2.cpu().numpy()
    finally:
        tool.set_option(_lib.MHS_OPT_SYNC, 1)
        tool.set_stream(None)
        plan.close()
    assert np.array_equal(c, fwd.reference(sr, pqs, av, bv, nC))
    ref, spread = witness_reference(sr, A, pqs, av, bv, c, dtype)
    assert np.array_equal(w, ref) and spread.any()
    assert np.array_equal(c2, fwd.reference(sr, pqs, av + 1.0, bv, nC))
    assert np.array_equal(w2, witness_reference(sr, A, pqs, av + 1.0, bv, c2, dtype)[0])


# 12. run_arg: the forward's bits and the witness of the two separate calls
@pytest.mark.parametrize("dtype", DTYPES)
def test_witness_run_arg(tool, dtype):
    A, B, Cp, Ci, pqs = fwd.small_pair()
    dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
    sr, nC = "max_min", len(Ci)
    av, bv = sub.exact_values(sr, A, B, 95)
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, dtype=dtype, semiring=sr)
    try:
        c, w = call(tool, plan, nC, dtype, av, bv)
        cval, wit = plan.run_arg(fwd.dev(tool, av, dtype), fwd.dev(tool, bv, dtype))
        torch.cuda.synchronize()
        assert cval.dtype == plan.dtype and wit.dtype == torch.int32 and cval.numel() == wit.numel() == nC
        c2 = cval.cpu().numpy()
        nz = (c != 0) | (c2 != 0)  # (the sign of a zero result is unspecified)
        assert c2[nz].tobytes() == c[nz].tobytes() and np.array_equal(c2, c) and np.array_equal(wit.cpu().numpy(), w)
        w_timed, ms = plan.witness(cval, fwd.dev(tool, av, dtype), fwd.dev(tool, bv, dtype), timed=True)
        assert ms > 0 and np.array_equal(w_timed.cpu().numpy(), w)
    finally:
        plan.close()
    assert np.array_equal(w, witness_reference(sr, A, pqs, av, bv, c, dtype)[0])
