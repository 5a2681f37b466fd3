"""GPU tests of the batched values backward (mhspgemm.ValuesPlan.grad_batched / .apply_batched over
mhs_spgemm_values_grad_batched / _f32): W cotangent sets in one walk of the patterns, on plans of every width.

Every set has the contract of the unbatched backward, and the references are per set: tests/_util.py's exact_grad
over expand's kept products.  FP64 plans: assert_f64_bound, |got - ref| <= 1.01 m 2^-53 S against long-double sums
for an entry of m kept products with absolute sum S.  FP32 plans: the contract of tests/test_gpu_values_f32.py on
float32-rounded inputs, |got - ref| <= 1.01 m 2^-24 S against the FP64 sum.  Inputs have magnitude in [0.1, 1):
nothing is subnormal.  Entries with m = 0 must be exactly 0.  Every output starts NaN-filled, padding between the
sets included: every segment entry must be written and the padding must keep the sentinel's bits.  Rows on the class
edges carry integer values and cotangents of +-{1, 2, 3}, exact in either type in any order while every sum stays
below 2^24, and are compared with np.array_equal.  dA has a fixed order: its bits are held equal across two calls,
for a set inside a batch and alone, and against mhs_spgemm_values_grad on a width-1 plan of the same type.  Nothing
here is a measured tolerance.  Inputs, value sets and helpers of the forward's batched tests are shared by import."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mhspgemm
from mhspgemm import _lib
import test_gpu_values_batched as fb
from test_gpu_values_batched import (BLOCK_DIRECT, BLOCK_SEARCH, DOT, GLOBAL, TEAM, TYPES, WAVE_DIRECT, WAVE_SEARCH, assert_set,
                                     make_plan, nans, plans, rounded, set_values, up)
from _util import device_csr, edge_values, exact_grad, expand, new_values

pytestmark = pytest.mark.gpu

PAD = 7
NB1 = fb.NB1  # 5: W = 2 runs passes of 2, 2, 1 and W = 4 passes of 4, 1
PRODUCT = (TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32)


def grad_reference(pqs, nA, nB, av, bv, G, dt):
    """The (ref, m, S) triples of dA and of dB of one set: long double for FP64 plans (exact_grad), float64 for
    FP32 ones."""
    if dt == "f64":
        return exact_grad(pqs, av, bv, G, nA, nB)
    p, q, s = pqs

    def triple(idx, w, n):
        return np.bincount(idx, w, n), np.bincount(idx, minlength=n).astype(np.int64), np.bincount(idx, np.abs(w), n)

    return triple(p, bv[q] * G[s], nA), triple(q, av[p] * G[s], nB)


def call(tool, plan, dt, dG, dAv, dBv, nb, **kw):
    """One grad_batched call into NaN-filled outputs whose row stride is nnz + PAD: the two gradients as host arrays
    [nb, nnz], after the padding has been held to the sentinel's bits."""
    outs, views = {}, {}
    for side, nnz, need in (("A", plan.nnzA, kw.get("need_A", True)), ("B", plan.nnzB, kw.get("need_B", True))):
        if need:
            outs[side] = nans(tool, (nb, nnz + PAD), dt)
            views[side] = outs[side][:, :nnz]
    r = plan.grad_batched(dG, dAv, dBv, out_A=views.get("A"), out_B=views.get("B"), **kw)
    torch.cuda.synchronize()
    assert (r[0] is views.get("A")) and (r[1] is views.get("B"))
    got = []
    sentinel = bits(np.full(1, np.nan, TYPES[dt][1]))[0]
    for side, nnz in (("A", plan.nnzA), ("B", plan.nnzB)):
        if side not in outs:
            got.append(None)
            continue
        full = outs[side].cpu().numpy()
        assert np.all(bits(full[:, nnz:]) == sentinel), f"d{side}: the padding between the sets keeps its bytes"
        got.append(np.ascontiguousarray(full[:, :nnz]))
    return got


def assert_sets(gA, gB, refs, dt, what):
    for b, (refA, refB) in enumerate(refs):
        if gA is not None:
            assert_set(gA[b], refA, dt, f"{what} set {b} dA")
        if gB is not None:
            assert_set(gB[b], refB, dt, f"{what} set {b} dB")


def unbatched(tool, plan1, dG, dAv, dBv, b):
    """Set b through mhs_spgemm_values_grad on the width-1 plan."""
    pick = lambda t: t if t.dim() == 1 else t[b]  # noqa: E731
    dA, dB = plan1.grad(dG[b].contiguous(), pick(dAv).contiguous(), pick(dBv).contiguous())
    torch.cuda.synchronize()
    return dA.cpu().numpy(), dB.cpu().numpy()


# ------------------------------------------------------------------ 1. every class, every set, dA's bits ---
@functools.lru_cache(maxsize=None)
def product_grad_sets(name, dt):
    """The NB1 value and cotangent sets of an input and each set's references: shared by the widths, never changed."""
    A, B, Cp, Ci, pqs = fb.product_input(name)
    av, bv, _ = fb.product_sets(name, dt)
    G = set_values(len(Ci), NB1, 500, dt)
    return av, bv, G, [grad_reference(pqs, A.nnz, B.nnz, av[b], bv[b], G[b], dt) for b in range(NB1)]


_DONE = {}


def every_set(tool, name, dt, W):
    if (name, dt, W) not in _DONE:
        A, B, Cp, Ci, _ = fb.product_input(name)
        av, bv, G, refs = product_grad_sets(name, dt)
        plan, plan1 = make_plan(tool, A, B, Cp, Ci, dt, W), make_plan(tool, A, B, Cp, Ci, dt, 1)
        try:
            info = plan.info()
            assert info["width"] == W
            dG, dAv, dBv = up(tool, G, dt), up(tool, av, dt), up(tool, bv, dt)
            gA, gB = call(tool, plan, dt, dG, dAv, dBv, NB1)
            gA2, _ = call(tool, plan, dt, dG, dAv, dBv, NB1)
            last = NB1 - 1  # (the tail pass's set inside the batch; alone it is set 0 of a pass)
            aloneA, aloneB = call(tool, plan, dt, dG[last:], dAv[last:], dBv[last:], 1)
            one = [unbatched(tool, plan1, dG, dAv, dBv, b) for b in range(NB1)]
        finally:
            plan.close()
            plan1.close()
        what = f"{name} {dt} W={W}"
        assert_sets(gA, gB, refs, dt, what)
        assert_sets(aloneA, aloneB, refs[last:], dt, what + " nb=1")
        assert np.array_equal(bits(gA), bits(gA2)), f"{what}: dA has the same bits on every call"
        assert np.array_equal(bits(gA[last]), bits(aloneA[0])), f"{what}: a set's dA inside the batch and alone"
        for b in range(NB1):
            assert np.array_equal(bits(gA[b]), bits(one[b][0])), f"{what} set {b}: dA has the width-1 plan's unbatched bits"
            assert_set(one[b][1], refs[b][1], dt, f"{what} set {b} unbatched dB")
        _DONE[name, dt, W] = info
    return _DONE[name, dt, W]


@plans
@pytest.mark.parametrize("name", fb.INPUTS)
def test_grad_batched_every_class_every_set(tool, name, dt, W):
    info = every_set(tool, name, dt, W)
    if name == "global_rows":
        assert info["rows"][GLOBAL] == 2, info
    if name == "tiny_zoo":
        assert info["rows"][TEAM] > 0.5 * sum(info["rows"])


@plans
def test_grad_batched_every_class_has_rows(tool, dt, W):
    rows = np.sum([every_set(tool, name, dt, W)["rows"] for name in fb.INPUTS], axis=0)
    for cls in PRODUCT:
        assert rows[cls] > 0, f"class {cls} has no rows at {dt} W={W}"
    assert rows[DOT] == 0


# ------------------------------------------------------------------ 2. class edges, exact ---
def integer_sets(n, nb, seed):
    return np.stack([edge_values(n, seed + b) for b in range(nb)])


def integer_grads(pqs, nA, nB, av, bv, G):
    p, q, s = pqs
    wA, wB = np.bincount(p, bv[q] * G[s], nA), np.bincount(q, av[p] * G[s], nB)  # integers: exact in float64
    absA, absB = np.bincount(p, np.abs(bv[q] * G[s]), nA), np.bincount(q, np.abs(av[p] * G[s]), nB)
    assert max(absA.max(initial=0), absB.max(initial=0)) < 2 ** 24
    return wA, wB


@plans
@pytest.mark.parametrize("side", [0, 1], ids=["at", "above"])
@pytest.mark.parametrize("name", fb.EDGE_NAMES)
def test_grad_batched_class_edges_exact(tool, name, side, dt, W):
    sb = W * TYPES[dt][2]
    edge = fb.TEAM_EDGES[name] if name in fb.TEAM_EDGES else fb.BYTE_EDGES[sb][name]
    n, span, products = edge[side]
    A, B, Cp, Ci, pqs = fb.edge_rows_of(n, span, products)
    nb = W + 1
    av, bv, G = integer_sets(A.nnz, nb, 50), integer_sets(B.nnz, nb, 80), integer_sets(len(Ci), nb, 110)
    plan = make_plan(tool, A, B, Cp, Ci, dt, W)
    try:
        info = plan.info()
        classes = [c for c in range(8) if info["rows"][c]]
        assert classes == [edge[2][side]] == [fb.val_class(n, span, products, sb)], (classes, info)
        gA, gB = call(tool, plan, dt, up(tool, G, dt), up(tool, av, dt), up(tool, bv, dt), nb)
    finally:
        plan.close()
    for b in range(nb):
        wA, wB = integer_grads(pqs, A.nnz, B.nnz, av[b], bv[b], G[b])
        assert np.array_equal(gA[b].astype(np.float64), wA), f"set {b} dA"
        assert np.array_equal(gB[b].astype(np.float64), wB), f"set {b} dB"


# ------------------------------------------------------------------ 3. reduction placement ---
# The shapes of tests/test_gpu_values_grad.py::test_grad_group_reduction_placement -- B rows one below, at and one
# above the group widths (8 and 16 lanes) and the width-1 piece loop (128) -- with B rows around the piece loop of
# the wide walks, val_pieces(W) x 16 = 64 (W = 2) and 32 (W = 4), and A rows around the stage's capacity: 63, 64, 65
# and 130 entries in a wave (its stage holds 64, wide or not), 255, 256, 257 in a block (256), which leave lane
# groups idle in the last step; in a narrow column window (direct classes) and a wide one (searched).
B_LENS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
# A rows as {B-row length: count}.  The narrow window's rows are direct at every width (span 200 <= 256); the wide
# window's are searched, so their C rows must fit the narrowest searched slices (FP64 W = 4: 226 entries a wave,
# 4,436 a block): a wave row has at most 220 products, a block row 1,931.
WAVE_NARROW = {1: 40, 15: 3, 16: 3, 17: 3, 31: 2, 32: 2, 33: 2, 63: 2, 64: 2, 65: 2, 127: 1, 129: 1}  # 63 entries, 1,016 products
WAVE_WIDE = {1: 55, 15: 2, 16: 2, 17: 2, 31: 1, 33: 1}                                                # 63 entries, 215 products
WAVE_WIDE_130 = {1: 124, 15: 2, 16: 2, 17: 2}                                                         # 130 entries, 220 products
BLOCK_NARROW = {1: 60, 15: 20, 16: 20, 17: 20, 31: 20, 32: 20, 33: 20, 63: 15, 64: 15, 65: 15, 127: 10, 128: 10, 129: 10}  # 255, 9,660
BLOCK_WIDE = {1: 201, 15: 10, 16: 10, 17: 10, 31: 5, 32: 5, 33: 5, 63: 2, 64: 2, 65: 2, 127: 1, 128: 1, 129: 1}            # 255, 1,929


@functools.lru_cache(maxsize=None)
def reduction_case():
    rng = np.random.default_rng(43)
    per, N, narrow = 210, 200_000, 200
    half = per * len(B_LENS)
    brows = []
    for k in range(2 * half):
        ln = B_LENS[k % len(B_LENS)]
        brows.append(np.sort(rng.choice(narrow if k < half else N, ln, replace=False)))
    Bp = np.zeros(2 * half + 1, np.int64)
    Bp[1:] = np.cumsum([len(r) for r in brows])
    Bc = np.concatenate(brows).astype(np.int32)

    def arow(base, mix):
        ks = []
        for ln, cnt in mix.items():
            pool = base + np.arange(B_LENS.index(ln), half, len(B_LENS))
            ks.extend(rng.choice(pool, cnt, replace=False).tolist())
        return sorted(ks)

    arows = []
    for base, wave, wave130, block in ((0, WAVE_NARROW, {**WAVE_NARROW, 1: 107}, BLOCK_NARROW),
                                       (half, WAVE_WIDE, WAVE_WIDE_130, BLOCK_WIDE)):
        for extra in (0, 1, 2):  # 63, 64, 65 entries, then 130: waves
            arows.append(arow(base, {**wave, 1: wave[1] + extra}))
        arows.append(arow(base, wave130))
        for extra in (0, 1, 2):  # 255, 256, 257 entries: blocks
            arows.append(arow(base, {**block, 1: block[1] + extra}))
        for mix in ({1: 1, 15: 1, 17: 1}, {16: 2, 1: 3}, {33: 1}, {31: 1, 1: 2}, {32: 1}):  # teams
            arows.append(arow(base, mix))
    Ap = np.zeros(len(arows) + 1, np.int64)
    Ap[1:] = np.cumsum([len(r) for r in arows])
    Ac = np.array([k for r in arows for k in r], np.int32)
    A = mhspgemm.CSR(len(arows), 2 * half, Ap.astype(np.int32), Ac, np.ones(len(Ac)))
    B = mhspgemm.CSR(2 * half, N, Bp.astype(np.int32), Bc, np.ones(len(Bc)))
    Cp, Ci = fb.pattern_of(A, B)
    return A, B, Cp, Ci, expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)


@functools.lru_cache(maxsize=None)
def reduction_sets(dt):
    A, B, Cp, Ci, pqs = reduction_case()
    av, bv, G = set_values(A.nnz, NB1, 210, dt), set_values(B.nnz, NB1, 220, dt), set_values(len(Ci), NB1, 230, dt)
    return av, bv, G, [grad_reference(pqs, A.nnz, B.nnz, av[b], bv[b], G[b], dt) for b in range(NB1)]


@plans
def test_grad_batched_group_reduction_placement(tool, dt, W):
    A, B, Cp, Ci, _ = reduction_case()
    assert {63, 64, 65, 130, 255, 256, 257} <= set(np.diff(A.ptr).tolist()) and set(np.diff(B.ptr).tolist()) == set(B_LENS)
    av, bv, G, refs = reduction_sets(dt)
    plan, plan1 = make_plan(tool, A, B, Cp, Ci, dt, W), make_plan(tool, A, B, Cp, Ci, dt, 1)
    try:
        rows = plan.info()["rows"]
        assert rows[WAVE_DIRECT] == 4 and rows[WAVE_SEARCH] == 4 and rows[BLOCK_DIRECT] == 3 and rows[BLOCK_SEARCH] == 3, rows
        assert rows[TEAM] == 10, rows
        dG, dAv, dBv = up(tool, G, dt), up(tool, av, dt), up(tool, bv, dt)
        gA, gB = call(tool, plan, dt, dG, dAv, dBv, NB1)
        one = [unbatched(tool, plan1, dG, dAv, dBv, b)[0] for b in range(NB1)]
    finally:
        plan.close()
        plan1.close()
    assert_sets(gA, gB, refs, dt, f"reduction {dt} W={W}")
    for b in range(NB1):
        assert np.array_equal(bits(gA[b]), bits(one[b])), f"set {b}: dA has the width-1 plan's unbatched bits"


# ------------------------------------------------------------------ 4. masked plans ---
@functools.lru_cache(maxsize=None)
def mask_grad_sets(case, dt, nb):
    A, B, Mp, Mc, pqs = fb.mask_input(case)
    av, bv, _ = fb.mask_sets(case, dt, nb)
    G = set_values(len(Mc), nb, 600, dt)
    return av, bv, G, [grad_reference(pqs, A.nnz, B.nnz, av[b], bv[b], G[b], dt) for b in range(nb)]


@plans
@pytest.mark.parametrize("form", ["product", "dot", "auto"])
@pytest.mark.parametrize("case", ["triangle", "rect"])
def test_grad_batched_masked_forms(tool, case, form, dt, W):
    A, B, Mp, Mc, (p, q, s) = fb.mask_input(case)
    nb = W + 1
    av, bv, G, refs = mask_grad_sets(case, dt, nb)
    plan = make_plan(tool, A, B, Mp, Mc, dt, W, masked=True, form=form)
    plan1 = None
    try:
        info = plan.info()
        assert info["kept_products"] == len(p) and 0 < info["kept_products"] < info["products"], "products outside the mask"
        if form != "auto":
            assert (info["dot"] > 0) == (form == "dot"), (form, info)
        dG, dAv, dBv = up(tool, G, dt), up(tool, av, dt), up(tool, bv, dt)
        gA, gB = call(tool, plan, dt, dG, dAv, dBv, nb)
        gA2, _ = call(tool, plan, dt, dG, dAv, dBv, nb)
        plan1 = make_plan(tool, A, B, Mp, Mc, dt, 1, masked=True, form=form)
        one = [unbatched(tool, plan1, dG, dAv, dBv, b)[0] for b in range(nb)]
    finally:
        plan.close()
        if plan1 is not None:
            plan1.close()
    assert_sets(gA, gB, refs, dt, f"{case} {form} {dt} W={W}")  # (m counts kept products only: dropped ones reach neither side)
    assert np.array_equal(bits(gA), bits(gA2)), "two calls, the same dA bits"
    for b in range(nb):
        assert np.array_equal(bits(gA[b]), bits(one[b])), f"set {b}: dA has the width-1 plan's unbatched bits"


# ------------------------------------------------------------------ 5. sets do not mix; strides; shared operands ---
@plans
def test_grad_batched_sets_do_not_mix_and_strides(tool, dt, W):
    A, Cp, Ci, pqs = fb.square_case()
    nnz, nC, most = A.nnz, len(Ci), 2 * W + 1
    av, bv, G = set_values(nnz, most, 300, dt), set_values(nnz, most, 700, dt), set_values(nC, most, 800, dt)
    G[1] = 0.0  # one set whose cotangent is all zero
    dAv, dBv, dG = up(tool, av, dt), up(tool, bv, dt), up(tool, G, dt)
    padA, padG = nans(tool, (most, nnz + 5), dt), nans(tool, (most, nC + 3), dt)  # NaN between the sets of the inputs
    padA[:, :nnz] = dAv
    padG[:, :nC] = dG
    torch.cuda.synchronize()
    refs = {}

    def ref(ia, ib, ig):
        if (ia, ib, ig) not in refs:
            refs[ia, ib, ig] = grad_reference(pqs, nnz, nnz, av[ia], bv[ib], G[ig], dt)
        return refs[ia, ib, ig]

    plan = make_plan(tool, A, A, Cp, Ci, dt, W)
    try:
        for nb in sorted({1, W, W + 1, 2 * W + 1}):
            modes = {"A shared": (dAv[0], dBv[:nb], dG[:nb], lambda b: (0, b, b)),
                     "B shared": (dAv[:nb], dBv[0], dG[:nb], lambda b: (b, 0, b)),
                     "both shared": (dAv[0], dBv[0], dG[:nb], lambda b: (0, 0, b)),
                     "both 2-D": (dAv[:nb], dBv[:nb], dG[:nb], lambda b: (b, b, b)),
                     "padded": (padA[:nb, :nnz], dBv[:nb], padG[:nb, :nC], lambda b: (b, b, b))}
            for mode, (ta, tb, tg, pick) in modes.items():
                if mode == "padded" and nb > 1:
                    assert ta.stride(0) == nnz + 5 and tg.stride(0) == nC + 3
                gA, gB = call(tool, plan, dt, tg, ta, tb, nb)
                assert_sets(gA, gB, [ref(*pick(b)) for b in range(nb)], dt, f"{mode} nb={nb}")
                if nb > 1:  # the all-zero cotangent: exactly 0 on both sides (the bound is 0 there: S = 0)
                    assert not gA[1].any() and not gB[1].any(), f"{mode} nb={nb}: a zero cotangent's gradients"
        # A*A with one tensor as both operands: the two gradients still come back apart
        gA, gB = call(tool, plan, dt, dG[:W + 1], dAv[:W + 1], dAv[:W + 1], W + 1)
        assert_sets(gA, gB, [grad_reference(pqs, nnz, nnz, av[b], av[b], G[b], dt) for b in range(W + 1)], dt, "A*A")
        assert torch.isnan(padA[:, nnz:]).all().item() and torch.isnan(padG[:, nC:]).all().item()
        # outputs allocated by the call: [nb, nnz] of the plan's type, and the timed call
        dA, dB, ms = plan.grad_batched(dG[:3], dAv[:3], dBv[0], timed=True)
        torch.cuda.synchronize()
        assert ms > 0.0 and dA.shape == (3, nnz) and dB.shape == (3, nnz) and dA.dtype == dB.dtype == TYPES[dt][0]
        assert_sets(dA.cpu().numpy(), dB.cpu().numpy(), [ref(b, 0, b) for b in range(3)], dt, "allocated outputs")
    finally:
        plan.close()


@plans
@pytest.mark.parametrize("shape", [(200, 256, 1000), (3000, 4992, 4000)], ids=["wave_direct", "block_direct"])
def test_grad_batched_zero_cotangents_on_direct_rows(tool, shape, dt, W):
    """A cotangent that is zero at a slot in one set and not in another: the direct classes skip a slot only when
    every set's cotangent is 0 there.  Integer values: exact."""
    A, B, Cp, Ci, pqs = fb.edge_rows_of(*shape)
    nb = W + 1
    av, bv, G = integer_sets(A.nnz, nb, 20), integer_sets(B.nnz, nb, 30), integer_sets(len(Ci), nb, 40)
    rng = np.random.default_rng(5)
    for b in range(nb):
        G[b, rng.random(len(Ci)) < 0.5] = 0.0  # zero at other slots in every set
    G[:, ::7] = 0.0  # zero in all sets at some slots
    G[W - 1] = 0.0   # one whole set of a full pass
    plan = make_plan(tool, A, B, Cp, Ci, dt, W)
    try:
        rows = plan.info()["rows"]
        assert rows[WAVE_DIRECT if shape[0] == 200 else BLOCK_DIRECT] == A.M, rows
        gA, gB = call(tool, plan, dt, up(tool, G, dt), up(tool, av, dt), up(tool, bv, dt), nb)
    finally:
        plan.close()
    for b in range(nb):
        wA, wB = integer_grads(pqs, A.nnz, B.nnz, av[b], bv[b], G[b])
        assert np.array_equal(gA[b].astype(np.float64), wA) and np.array_equal(gB[b].astype(np.float64), wB), f"set {b}"
    assert not gA[W - 1].any() and not gB[W - 1].any()


# ------------------------------------------------------------------ 6. one-sided calls; the width-1 plan ---
@plans
def test_grad_batched_one_sided_calls(tool, dt, W):
    A, Cp, Ci, pqs = fb.square_case()
    nnz, nC, nb = A.nnz, len(Ci), W + 1
    av, bv, G = set_values(nnz, nb, 300, dt), set_values(nnz, nb, 700, dt), set_values(nC, nb, 800, dt)
    refs = [grad_reference(pqs, nnz, nnz, av[b], bv[b], G[b], dt) for b in range(nb)]
    dAv, dBv, dG = up(tool, av, dt), up(tool, bv, dt), up(tool, G, dt)
    L = _lib.lib()
    fn = L.mhs_spgemm_values_grad_batched_f32 if dt == "f32" else L.mhs_spgemm_values_grad_batched
    plan = make_plan(tool, A, A, Cp, Ci, dt, W)
    try:
        oA, oB = nans(tool, (nb, nnz), dt), nans(tool, (nb, nnz), dt)
        # dA only, Aval NULL (stride and all); the dB buffer is given to nobody
        assert fn(tool.ctx, plan.plan, nb, None, 0, dBv.data_ptr(), nnz, dG.data_ptr(), nC, oA.data_ptr(), nnz, None, 0, None) == 0
        torch.cuda.synchronize()
        assert torch.isnan(oB).all().item(), "a dA-only call leaves the other buffer alone"
        gA = oA.cpu().numpy()
        oA.fill_(float("nan"))
        torch.cuda.synchronize()
        assert fn(tool.ctx, plan.plan, nb, dAv.data_ptr(), nnz, None, 0, dG.data_ptr(), nC, None, 0, oB.data_ptr(), nnz, None) == 0
        torch.cuda.synchronize()
        assert torch.isnan(oA).all().item(), "a dB-only call leaves the other buffer alone"
        gB = oB.cpu().numpy()
        # the wrapper's one-sided calls: None for the side not asked for, its operand not needed
        rA = plan.grad_batched(dG, None, dBv, need_B=False)
        rB = plan.grad_batched(dG, dAv, None, need_A=False)
        torch.cuda.synchronize()
        assert rA[1] is None and rB[0] is None
        assert np.array_equal(bits(rA[0].cpu().numpy()), bits(gA)), "dA alone through the wrapper: the same bits"
        wB = rB[1].cpu().numpy()
    finally:
        plan.close()
    assert_sets(gA, gB, refs, dt, f"one-sided {dt} W={W}")
    assert_sets(None, wB, refs, dt, f"one-sided wrapper {dt} W={W}")


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_grad_batched_on_a_width_1_plan(tool, dt):
    """The general fallback: nb = 3 on a width-1 plan is three runs of the unbatched kernels."""
    A, B, Cp, Ci, pqs = fb.product_input("bin_zoo")
    av, bv, G, refs = product_grad_sets("bin_zoo", dt)
    plan = make_plan(tool, A, B, Cp, Ci, dt, 1)
    try:
        dG, dAv, dBv = up(tool, G[:3], dt), up(tool, av[:3], dt), up(tool, bv[:3], dt)
        gA, gB = call(tool, plan, dt, dG, dAv, dBv, 3)
        one = [unbatched(tool, plan, dG, dAv, dBv, b) for b in range(3)]
    finally:
        plan.close()
    assert_sets(gA, gB, refs[:3], dt, f"width 1 {dt}")
    for b in range(3):
        assert np.array_equal(bits(gA[b]), bits(one[b][0])), f"set {b}: the bits of mhs_spgemm_values_grad"


# ------------------------------------------------------------------ 7. apply_batched ---
@functools.lru_cache(maxsize=None)
def smallest_golden():
    best = None
    for name in fb.PRODUCT_CASES:
        A, B, Cp, Ci, pqs = fb.product_input(name)
        if len(pqs[0]) and (best is None or A.nnz + B.nnz < best[1]):
            best = (name, A.nnz + B.nnz)
    return best[0]


@pytest.mark.parametrize("masked", [False, True])
def test_grad_batched_apply_gradcheck(tool, masked):
    A, B, Cp, Ci, _ = fb.product_input(smallest_golden())
    if masked:  # every second entry of the product's pattern
        keep = np.arange(len(Ci)) % 2 == 0
        rows = np.repeat(np.arange(A.M), np.diff(Cp))
        ptr = np.zeros(A.M + 1, np.int64)
        np.cumsum(np.bincount(rows[keep], minlength=A.M), out=ptr[1:])
        Cp, Ci = ptr.astype(np.int32), Ci[keep]
    nb = 3
    plan = make_plan(tool, A, B, Cp, Ci, "f64", 2, masked=masked, form="auto")
    try:
        a = up(tool, set_values(A.nnz, nb, 5, "f64"), "f64").requires_grad_(True)
        b = up(tool, set_values(B.nnz, nb, 6, "f64"), "f64").requires_grad_(True)
        shared = up(tool, rounded(new_values(B.nnz, 7, signed=True), "f64"), "f64").requires_grad_(True)
        out = plan.apply_batched(a, b)
        assert out.shape == (nb, len(Ci)) and out.requires_grad
        assert torch.autograd.gradcheck(plan.apply_batched, (a, b), nondet_tol=1e-9)
        # a shared 1-D Bval: its gradient is the per-set gradients summed over the sets
        assert torch.autograd.gradcheck(plan.apply_batched, (a, shared), nondet_tol=1e-9)
        g = torch.ones_like(out)
        (dB_sum,) = torch.autograd.grad(plan.apply_batched(a.detach(), shared), (shared,), g)
        _, per_set = plan.grad_batched(g, a.detach(), shared.detach(), need_A=False)
        torch.cuda.synchronize()
        assert dB_sum.shape == (B.nnz,) and torch.allclose(dB_sum, per_set.sum(0), rtol=1e-12, atol=1e-12)
    finally:
        plan.close()
        tool.set_stream(None)


# ------------------------------------------------------------------ 8. stream and sync contract ---
@plans
@pytest.mark.parametrize("where", ["side", "default"])
def test_grad_batched_stream_ordered(tool, where, dt, W):
    """MHS_OPT_SYNC 0: the inputs hold NaN until copies queued behind a long torch kernel on the same stream fill
    them; the batched backward is queued after them, a torch op consumes its outputs at once, and only that stream
    is synchronised."""
    A, Cp, Ci, pqs = fb.square_case()
    nnz, nC, nb = A.nnz, len(Ci), W + 1
    av, bv, G = set_values(nnz, nb, 300, dt), set_values(nnz, nb, 700, dt), set_values(nC, nb, 800, dt)
    src = [up(tool, v, dt) for v in (G, av, bv)]
    dG, dAv, dBv = nans(tool, (nb, nC), dt), nans(tool, (nb, nnz), dt), nans(tool, (nb, nnz), dt)
    oA, oB = nans(tool, (nb, nnz), dt), nans(tool, (nb, nnz), dt)
    plan = make_plan(tool, A, A, Cp, Ci, dt, W)
    ballast = torch.ones(1 << 24, dtype=torch.float64, device=f"cuda:{tool.device}")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(tool.device) if where == "side" else torch.cuda.default_stream(tool.device)
    tool.set_option(_lib.MHS_OPT_SYNC, 0)
    try:
        with torch.cuda.stream(stream):
            assert (torch.cuda.current_stream(tool.device).cuda_stream != 0) == (where == "side")
            fb.busy(ballast)
            for dst, s_ in zip((dG, dAv, dBv), src):
                dst.copy_(s_, non_blocking=True)
            plan._ordered_on_current_stream(lambda: plan.grad_batched(dG, dAv, dBv, out_A=oA, out_B=oB))
            keptA, keptB = oA.clone(), oB.clone()  # (queued behind the call on the same stream)
            stream.synchronize()
            gA, gB = keptA.cpu().numpy(), keptB.cpu().numpy()
            r = plan._ordered_on_current_stream(lambda: plan.grad_batched(dG, dAv, dBv, out_A=oA, out_B=oB, timed=True))
            assert r[2] > 0.0
            stream.synchronize()
            tA, tB = oA.cpu().numpy(), oB.cpu().numpy()
    finally:
        tool.set_option(_lib.MHS_OPT_SYNC, 1)
        tool.set_stream(None)
        plan.close()
    refs = [grad_reference(pqs, nnz, nnz, av[b], bv[b], G[b], dt) for b in range(nb)]
    assert_sets(gA, gB, refs, dt, f"{where} stream")
    assert_sets(tA, tB, refs, dt, f"{where} stream, timed call")
    assert np.array_equal(bits(gA), bits(tA))


# ------------------------------------------------------------------ 9. refusals with a context ---
def test_grad_batched_refusals(tool):
    A, Cp, Ci, _ = fb.square_case()
    A.H2D(tool.device)
    C = device_csr(tool, A.M, A.N, Cp, Ci)
    L = _lib.lib()
    nnz, nC = A.nnz, len(Ci)

    def message():
        return L.mhs_last_error(tool.ctx).decode()

    p2 = mhspgemm.ValuesPlan(tool, A, A, C, width=2)
    try:
        v64, v32 = up(tool, set_values(nnz, 2, 1, "f64"), "f64"), up(tool, set_values(nnz, 2, 1, "f32"), "f32")
        g64, g32 = up(tool, set_values(nC, 2, 2, "f64"), "f64"), up(tool, set_values(nC, 2, 2, "f32"), "f32")
        o64, o32 = nans(tool, (4, nnz), "f64"), nans(tool, (4, nnz), "f32")
        ms = ctypes.c_double(-1.0)
        x, g, oa, ob = v64.data_ptr(), g64.data_ptr(), o64.data_ptr(), o64.data_ptr() + 8 * 2 * nnz
        x32, h32, oa32, ob32 = v32.data_ptr(), g32.data_ptr(), o32.data_ptr(), o32.data_ptr() + 4 * 2 * nnz
        f, f32, r = L.mhs_spgemm_values_grad_batched, L.mhs_spgemm_values_grad_batched_f32, ctypes.byref(ms)
        calls = [
            (lambda: f(tool.ctx, None, 2, x, nnz, x, nnz, g, nC, oa, nnz, ob, nnz, r), "null plan"),
            (lambda: f(tool.ctx, p2.plan, 0, x, nnz, x, nnz, g, nC, oa, nnz, ob, nnz, r), "nb"),
            (lambda: f(tool.ctx, p2.plan, -1, x, nnz, x, nnz, g, nC, oa, nnz, ob, nnz, r), "nb"),
            (lambda: f(tool.ctx, p2.plan, 2, x, -nnz, x, nnz, g, nC, oa, nnz, ob, nnz, r), "negative stride"),
            (lambda: f(tool.ctx, p2.plan, 2, x, nnz, x, nnz, g, -1, oa, nnz, ob, nnz, r), "negative stride"),
            (lambda: f(tool.ctx, p2.plan, 2, x, nnz, x, nnz, g, nC, oa, nnz, ob, -nnz, r), "negative stride"),
            (lambda: f(tool.ctx, p2.plan, 2, x, nnz - 1, x, nnz, g, nC, oa, nnz, ob, nnz, r), "input stride"),
            (lambda: f(tool.ctx, p2.plan, 2, x, nnz, x, 1, g, nC, oa, nnz, ob, nnz, r), "input stride"),
            (lambda: f(tool.ctx, p2.plan, 2, x, nnz, x, nnz, g, nC - 1, oa, nnz, ob, nnz, r), "strideG"),
            (lambda: f(tool.ctx, p2.plan, 2, x, nnz, x, nnz, g, 0, oa, nnz, ob, nnz, r), "strideG"),
            (lambda: f(tool.ctx, p2.plan, 2, x, nnz, x, nnz, g, nC, oa, nnz - 1, ob, nnz, r), "output stride"),
            (lambda: f(tool.ctx, p2.plan, 2, x, nnz, x, nnz, g, nC, oa, nnz, ob, 0, r), "output stride"),
            (lambda: f(tool.ctx, p2.plan, 2, x, nnz, x, nnz, None, nC, oa, nnz, ob, nnz, r), "null dCval"),
            (lambda: f(tool.ctx, p2.plan, 2, x, nnz, x, nnz, g, nC, None, nnz, None, nnz, r), "no output"),
            (lambda: f(tool.ctx, p2.plan, 2, x, nnz, None, nnz, g, nC, oa, nnz, ob, nnz, r), "dAval needs Bval"),
            (lambda: f(tool.ctx, p2.plan, 2, None, nnz, x, nnz, g, nC, oa, nnz, ob, nnz, r), "dBval needs Aval"),
            (lambda: f32(tool.ctx, p2.plan, 2, x32, nnz, x32, nnz, h32, nC, oa32, nnz, ob32, nnz, r), "FP32"),
            # the unbatched entry point on the width-2 plan is still refused, unchanged
            (lambda: L.mhs_spgemm_values_grad(tool.ctx, p2.plan, x, x, g, oa, ob, r), "backward of batched plans is not built"),
        ]
        for use, cause in calls:
            assert use() == 3, cause
            assert cause in message(), (cause, message())
            assert "mhs_spgemm_values_grad" in message()
            assert ms.value == -1.0
        assert "width-1" in message()
        if torch.cuda.device_count() > 1:  # a plan of another device
            other = mhspgemm.Tool(1)
            try:
                assert f(other.ctx, p2.plan, 2, x, nnz, x, nnz, g, nC, oa, nnz, ob, nnz, r) == 3
                assert "another device" in L.mhs_last_error(other.ctx).decode() and ms.value == -1.0
            finally:
                other.close()
        p32 = mhspgemm.ValuesPlan(tool, A, A, C, dtype="float32", width=2)
        try:  # and the double call on an FP32 plan
            assert f(tool.ctx, p32.plan, 2, x, nnz, x, nnz, g, nC, oa, nnz, ob, nnz, r) == 3 and "FP64" in message()
        finally:
            p32.close()
        torch.cuda.synchronize()
        assert torch.isnan(o64).all().item() and torch.isnan(o32).all().item(), "a refused call writes nothing"
        assert ms.value == -1.0
        # nb = 1 takes any stride for the cotangent and the outputs; the context and the plan stay usable
        assert f(tool.ctx, p2.plan, 1, x, 0, x, 0, g, 0, oa, 0, ob, 0, None) == 0
        torch.cuda.synchronize()
        assert not torch.isnan(o64[0]).any().item() and not torch.isnan(o64[2]).any().item()
        assert torch.isnan(o64[1]).all().item() and torch.isnan(o64[3]).all().item()
    finally:
        p2.close()
