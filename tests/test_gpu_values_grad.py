"""GPU tests of the values backward (mhspgemm.ValuesPlan.grad / .apply over mhs_spgemm_values_grad): the
gradients of Aval and Bval for a cotangent on C's pattern, against a numpy reference that expands every
product as index arrays and sums with bincount -- independent of the library.  Tolerances are the
project's (tests/test_gpu_values.py): 1e-6 relative / 1e-12 absolute; with mixed signs 1e-6 of the same
gradient computed on absolute values; beside them grad_check holds dA and dB to the FP64 rounding bound,
1.01 m 2^-53 S per entry against sums in long double (tests/_util.py).  Every call writes into NaN-filled
buffers; entries that no kept product reaches must come back exactly 0.0."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mhspgemm
from mhspgemm import _lib, synth
from oracle import oracle as orc
from _util import (ATOL, GOLDEN, PRODUCT_CASES, RTOL, assert_f64_bound, bin_zoo, csr_of, device_csr, exact_grad, expand, filled,
                   load_golden, new_values, random_csr, ref_grad, tiny_zoo, upload)

pytestmark = pytest.mark.gpu

TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL, DOT = 1, 2, 3, 4, 5, 6, 7


def assert_grad(got, want, absw, reached, what):
    assert got.shape == want.shape and not np.isnan(got).any(), f"{what}: every entry is written"
    assert np.all(got[~reached] == 0.0), f"{what}: entries no kept product reaches are exactly 0.0"
    if absw is not None:
        assert np.all(np.abs(got - want) <= 1e-6 * absw + 1e-300), what
        return
    err = np.abs(got - want)
    bad = err > RTOL * np.abs(want) + ATOL
    assert not bad.any(), f"{what}: {bad.sum()} entries outside 1e-6 relative (max abs error {err.max():.3e})"


def grad_check(tool, A, B, Cp, Ci, seed=1, signed=False, masked=False, form="auto"):
    """The shared checker: a plan of A*B on the pattern (Cp, Ci), seeded Aval, Bval and cotangent, one
    backward call into NaN-filled buffers, compared with the reference.  Returns (info(), dA, dB)."""
    A.H2D(tool.device)
    if B is not A:
        B.H2D(tool.device)
    C = device_csr(tool, A.M, B.N, Cp, Ci)
    av, bv, G = new_values(A.nnz, seed, signed), new_values(B.nnz, seed + 1000, signed), new_values(len(Ci), seed + 2000, signed)
    plan = mhspgemm.ValuesPlan(tool, A, B, C, masked=masked, form=form)
    try:
        info = plan.info()
        oA, oB = filled(tool, A.nnz), filled(tool, B.nnz)
        dA, dB = plan.grad(upload(tool, G), upload(tool, av), upload(tool, bv), out_A=oA, out_B=oB)
        torch.cuda.synchronize()
        assert dA is oA and dB is oB
        gA, gB = dA.cpu().numpy(), dB.cpu().numpy()
    finally:
        plan.close()
    pqs = expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)
    assert len(pqs[0]) == info["kept_products"]
    wA, wB = ref_grad(pqs, av, bv, G, A.nnz, B.nnz)
    absA = absB = None
    if signed:
        absA, absB = ref_grad(pqs, np.abs(av), np.abs(bv), np.abs(G), A.nnz, B.nnz)
    assert_grad(gA, wA, absA, np.bincount(pqs[0], minlength=A.nnz) > 0, "dA")
    assert_grad(gB, wB, absB, np.bincount(pqs[1], minlength=B.nnz) > 0, "dB")
    exA, exB = exact_grad(pqs, av, bv, G, A.nnz, B.nnz)  # the FP64 contract: 1.01 m 2^-53 S, m = 0 exactly 0.0
    kind = f"masked plan, {form} form" if masked else "values plan"
    assert_f64_bound(gA, *exA, f"{kind}, dA")
    assert_f64_bound(gB, *exB, f"{kind}, dB")
    return info, gA, gB


def pattern_of(A, B):
    Cp, Ci, _ = orc.spgemm(A.ptr, A.col, np.ones(A.nnz), B.ptr, B.col, np.ones(B.nnz), B.N)
    return Cp, Ci


# 1. golden products: empty product, duplicates in A / B, rectangular, dense row and column, tile edges
@pytest.mark.parametrize("name", PRODUCT_CASES)
def test_grad_golden_products(tool, name):
    d, _, _, _ = load_golden(name)
    A = mhspgemm.CSR()
    assert mhspgemm.readMtxFile(A, str(GOLDEN / d["A"])) == 0
    B = A
    if d["B"]:
        B = mhspgemm.CSR()
        assert mhspgemm.readMtxFile(B, str(GOLDEN / d["B"])) == 0
    grad_check(tool, A, B, *pattern_of(A, B))


# 2. the zoos: every product-form class between them, so every backward kernel runs
@functools.lru_cache(maxsize=None)
def zoo(name):
    At, Bt = bin_zoo() if name == "bin_zoo" else tiny_zoo(7)
    A, B = csr_of(At), csr_of(Bt)
    return A, B, pattern_of(A, B)


_ZOO_INFO = {}


def zoo_info(tool, name):
    if name not in _ZOO_INFO:
        A, B, (Cp, Ci) = zoo(name)
        _ZOO_INFO[name] = grad_check(tool, A, B, Cp, Ci, seed=3)[0]
    return _ZOO_INFO[name]


def test_grad_bin_zoo(tool):
    info = zoo_info(tool, "bin_zoo")
    assert info["rows"][GLOBAL] >= 3 and info["rows"][BLOCK_DIRECT] > 0


def test_grad_tiny_zoo(tool):
    info = zoo_info(tool, "tiny_zoo")
    assert info["rows"][TEAM] > 0.5 * sum(info["rows"])


def test_grad_every_class_has_rows(tool):
    rows = np.add(zoo_info(tool, "bin_zoo")["rows"], zoo_info(tool, "tiny_zoo")["rows"])
    for cls in (TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL):
        assert rows[cls] > 0, f"class {cls} has no rows in bin_zoo + tiny_zoo"
    assert rows[DOT] == 0


# 3. shaped to catch a misplaced group reduction: B rows one below, at and one above the group widths (8 and
# 16 lanes) and the 128-entry piece loop, A rows whose entry count leaves groups idle in the last step
# (65 and 130 entries over a wave's 4 groups and its 64-entry stage, 257 over a block's 16 or 64 groups
# and its 256-entry stage), in a narrow column window (direct classes) and a wide one (searched)
B_LENS = (1, 15, 16, 17, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def reduction_case():
    rng = np.random.default_rng(41)
    per, N = 120, 200_000
    half = per * len(B_LENS)
    brows = []
    for k in range(2 * half):
        ln = B_LENS[k % len(B_LENS)]
        brows.append(np.sort(rng.choice(1000 if k < half else N, ln, replace=False)))
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
    for base in (0, half):
        arows.append(arow(base, {1: 45, 15: 6, 16: 6, 17: 6, 127: 1, 129: 1}))     # 65 entries, 589 products: a wave
        arows.append(arow(base, {1: 110, 15: 6, 16: 6, 17: 6, 128: 1, 129: 1}))    # 130 entries, 655 products: a wave
        arows.append(arow(base, {1: 40, 15: 50, 16: 50, 17: 57, 127: 20, 128: 20, 129: 20}))  # 257 entries: a block
        for mix in ({1: 1, 15: 1, 17: 1}, {16: 2, 1: 3}, {17: 3}, {15: 1}, {1: 7, 16: 1, 17: 1}):  # teams
            arows.append(arow(base, mix))
    Ap = np.zeros(len(arows) + 1, np.int64)
    Ap[1:] = np.cumsum([len(r) for r in arows])
    Ac = np.array([k for r in arows for k in r], np.int32)
    A = mhspgemm.CSR(len(arows), 2 * half, Ap.astype(np.int32), Ac, rng.uniform(0.1, 1.0, len(Ac)))
    B = mhspgemm.CSR(2 * half, N, Bp.astype(np.int32), Bc, rng.uniform(0.1, 1.0, len(Bc)))
    return A, B, pattern_of(A, B)


def test_grad_group_reduction_placement(tool):
    A, B, (Cp, Ci) = reduction_case()
    na = np.diff(A.ptr)
    assert {65, 130, 257} <= set(na.tolist()) and set(np.diff(B.ptr).tolist()) == set(B_LENS)
    info, _, _ = grad_check(tool, A, B, Cp, Ci, seed=5)
    rows = info["rows"]
    assert rows[WAVE_DIRECT] == 2 and rows[WAVE_SEARCH] == 2, info      # the 65- and 130-entry rows, narrow and wide
    assert rows[BLOCK_DIRECT] == 1 and rows[BLOCK_SEARCH] == 1, info    # the 257-entry rows
    assert rows[TEAM] == 10, info


# 4. mixed signs, rectangular
def test_grad_random_rect_signed(tool):
    p, c, v = random_csr(3000, 2000, 7, 1)
    Bp, Bc, Bv = random_csr(2000, 50_000, 12, 101)
    A, B = mhspgemm.CSR(3000, 2000, p, c, v), mhspgemm.CSR(2000, 50_000, Bp, Bc, Bv)
    grad_check(tool, A, B, *pattern_of(A, B), signed=True)


# 5. entries nothing reaches: an A entry at an empty B row, an A row whose C row is empty, a B row no A column reaches
def test_grad_unreached_entries_are_zero(tool):
    # B: row 0 empty, rows 1 and 2 filled, row 3 filled and never pointed at, row 4 empty
    Bp = np.array([0, 0, 3, 5, 9, 9], np.int32)
    Bc = np.array([0, 2, 5, 1, 2, 0, 3, 4, 5], np.int32)
    # A: row 0 -> B rows 0 (empty) and 1; row 1 -> B rows 0 and 4 only (its C row is empty); row 2 -> 1, 2; row 3 empty
    Ap = np.array([0, 2, 4, 6, 6], np.int32)
    Ac = np.array([0, 1, 0, 4, 1, 2], np.int32)
    A = mhspgemm.CSR(4, 5, Ap, Ac, np.ones(6))
    B = mhspgemm.CSR(5, 6, Bp, Bc, np.ones(9))
    Cp, Ci = pattern_of(A, B)
    assert Cp[2] == Cp[1], "row 1 of C is empty"
    _, gA, gB = grad_check(tool, A, B, Cp, Ci, seed=7)
    assert np.all(gA[[0, 2, 3]] == 0.0) and np.all(gA[[1, 4, 5]] > 0.0)
    assert np.all(gB[5:9] == 0.0) and np.all(gB[0:5] > 0.0)


@functools.lru_cache(maxsize=None)
def square_case():
    p, c, v = random_csr(2000, 2000, 8, 21)
    A = mhspgemm.CSR(2000, 2000, p, c, v)
    return A, pattern_of(A, A)


# 6. one side only: the other buffer is not touched, and the other operand's values are not needed
def test_grad_one_side_only(tool):
    A, (Cp, Ci) = square_case()
    A.H2D(tool.device)
    C = device_csr(tool, A.M, A.N, Cp, Ci)
    av, bv, G = new_values(A.nnz, 61), new_values(A.nnz, 62), new_values(len(Ci), 63)
    wA, wB = ref_grad(expand(A.ptr, A.col, A.ptr, A.col, Cp, Ci, A.N), av, bv, G, A.nnz, A.nnz)
    plan = mhspgemm.ValuesPlan(tool, A, A, C)
    try:
        dG, dAv, dBv = upload(tool, G), upload(tool, av), upload(tool, bv)
        oA, oB = filled(tool, A.nnz, -7.5), filled(tool, A.nnz, -7.5)
        rA = plan.grad(dG, Bval=dBv, need_B=False, out_A=oA, out_B=oB)
        torch.cuda.synchronize()
        assert rA[0] is oA and rA[1] is None
        assert torch.all(oB == -7.5).item(), "need_B=False: out_B untouched"
        gA = oA.cpu().numpy()
        oA.fill_(-7.5)
        torch.cuda.synchronize()
        rB = plan.grad(dG, Aval=dAv, need_A=False, out_A=oA, out_B=oB, timed=True)
        torch.cuda.synchronize()
        assert rB[0] is None and rB[1] is oB and rB[2] > 0.0
        assert torch.all(oA == -7.5).item(), "need_A=False: out_A untouched"
        gB = oB.cpu().numpy()
        with pytest.raises(ValueError):
            plan.grad(dG, need_A=False, need_B=False)
        with pytest.raises(ValueError):
            plan.grad(dG[:-1])
    finally:
        plan.close()
    assert_grad(gA, wA, None, wA != 0, "dA alone")  # (positive values: a sum is 0 only when it has no term)
    assert_grad(gB, wB, None, wB != 0, "dB alone")


# 7. dA has a fixed summation order: two calls, the same bits (on the zoo: every class)
def test_grad_dA_bit_equal_across_calls(tool):
    A, B, (Cp, Ci) = zoo("bin_zoo")
    A.H2D(tool.device)
    B.H2D(tool.device)
    C = device_csr(tool, A.M, B.N, Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, A, B, C)
    try:
        dG = upload(tool, new_values(len(Ci), 71, signed=True))
        a1, _ = plan.grad(dG)
        a2, _ = plan.grad(dG, out_A=filled(tool, A.nnz))
        torch.cuda.synchronize()
        g1, g2 = a1.cpu().numpy(), a2.cpu().numpy()
    finally:
        plan.close()
    assert np.array_equal(g1, g2) and np.any(g1 != 0.0)


# 8. A is B: the two gradients come back apart; their sum, and what autograd makes of plan.apply(x, x)
def test_grad_a_times_a(tool):
    A, (Cp, Ci) = square_case()
    A.H2D(tool.device)
    C = device_csr(tool, A.M, A.N, Cp, Ci)
    xv, G = new_values(A.nnz, 81), new_values(len(Ci), 82)
    wA, wB = ref_grad(expand(A.ptr, A.col, A.ptr, A.col, Cp, Ci, A.N), xv, xv, G, A.nnz, A.nnz)
    plan = mhspgemm.ValuesPlan(tool, A, A, C)
    try:
        x, dG = upload(tool, xv), upload(tool, G)
        dA, dB = plan.grad(dG, x, x)
        xg = x.clone().requires_grad_(True)
        out = plan.apply(xg, xg)
        out.backward(dG)
        torch.cuda.synchronize()
        got, auto, fwd = (dA + dB).cpu().numpy(), xg.grad.cpu().numpy(), out.detach().cpu().numpy()
    finally:
        plan.close()
    everywhere = np.ones(A.nnz, bool)
    assert_grad(got, wA + wB, None, everywhere, "dA + dB")
    assert_grad(auto, wA + wB, None, everywhere, "autograd of apply(x, x)")
    _, _, Cv = orc.spgemm(A.ptr, A.col, xv, A.ptr, A.col, xv, A.N)
    assert np.allclose(fwd, Cv, rtol=1e-9, atol=0.0), "apply's forward is run's"


# 9. masked plans: L*L on L's pattern, L the strictly lower triangle of a small symmetrised power-law graph
@functools.lru_cache(maxsize=None)
def triangle_case(n=3000):
    Gm = synth.powerlaw(n, seed=3)
    r = np.repeat(np.arange(Gm.M, dtype=np.int64), np.diff(Gm.ptr))
    c = Gm.col.astype(np.int64)
    off = r != c
    key = np.unique(np.maximum(r[off], c[off]) * n + np.minimum(r[off], c[off]))
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(key // n, minlength=n), out=ptr[1:])
    return mhspgemm.CSR(n, n, ptr.astype(np.int32), (key % n).astype(np.int32), np.ones(len(key)))


def test_grad_masked_forms(tool):
    L = triangle_case()
    got = {}
    for form in ("product", "dot", "auto"):
        info, gA, gB = grad_check(tool, L, L, L.ptr, L.col, seed=9, masked=True, form=form)
        assert 0 < info["kept_products"] < info["products"], "the case needs products outside the mask"
        assert (info["dot"] > 0) == (form != "product"), (form, info)
        got[form] = (gA, gB)
    for form in ("dot", "auto"):
        for x, y in zip(got[form], got["product"]):
            assert np.all(np.abs(x - y) <= RTOL * np.abs(y) + ATOL), form


# 10. stream order with MHS_OPT_SYNC 0.  The inputs hold NaN until a copy that is queued behind a long torch
# kernel on the same stream fills them; the call follows at once, a torch op consumes its outputs, and only
# that stream is synchronised.  A call that ran anywhere else than in the stream's order would read the NaNs
# (or be read before it wrote).  "side": a stream of torch's making, handed to the tool.  "default": torch's
# default stream, the null stream, whose handle 0 the tool cannot take -- there the caller fences
# (Tool.fence_default_stream) and ValuesPlan.apply does so itself.
def busy(x, rounds=150):
    """About 40 ms of work on the current stream (x: 512 MiB), queued in about a millisecond."""
    for _ in range(rounds):
        x.mul_(1.0000001)


@functools.lru_cache(maxsize=None)
def stream_case():
    A, (Cp, Ci) = square_case()
    av, bv, G = new_values(A.nnz, 91), new_values(A.nnz, 92), new_values(len(Ci), 93)
    wA, wB = ref_grad(expand(A.ptr, A.col, A.ptr, A.col, Cp, Ci, A.N), av, bv, G, A.nnz, A.nnz)
    return A, Cp, Ci, av, bv, G, wA, wB


def stream_of(tool, where):
    return torch.cuda.Stream(tool.device) if where == "side" else torch.cuda.default_stream(tool.device)


@pytest.mark.parametrize("where", ["side", "default"])
def test_grad_stream_ordered(tool, where):
    A, Cp, Ci, av, bv, G, wA, wB = stream_case()
    A.H2D(tool.device)
    C = device_csr(tool, A.M, A.N, Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, A, A, C)
    src = [upload(tool, v) for v in (G, av, bv)]
    dG, dAv, dBv = filled(tool, len(Ci)), filled(tool, A.nnz), filled(tool, A.nnz)
    oA, oB = filled(tool, A.nnz), filled(tool, A.nnz)
    ballast = torch.ones(1 << 26, dtype=torch.float64, device=f"cuda:{tool.device}")
    torch.cuda.synchronize()
    stream = stream_of(tool, where)
    tool.set_option(_lib.MHS_OPT_SYNC, 0)
    try:
        with torch.cuda.stream(stream):
            handle = torch.cuda.current_stream(tool.device).cuda_stream
            assert (handle != 0) == (where == "side")
            tool.set_stream(handle)
            busy(ballast)
            for dst, s_ in zip((dG, dAv, dBv), src):
                dst.copy_(s_, non_blocking=True)
            if where == "default":
                tool.fence_default_stream(after=False)
            dA, dB = plan.grad(dG, dAv, dBv, out_A=oA, out_B=oB)
            if where == "default":
                tool.fence_default_stream(after=True)
            twice = dA * 2.0 + dB  # queued behind the call
            stream.synchronize()
            got = twice.cpu().numpy()
    finally:
        tool.set_option(_lib.MHS_OPT_SYNC, 1)
        tool.set_stream(None)
        plan.close()
    assert_grad(got, 2.0 * wA + wB, None, np.ones(A.nnz, bool), "2 dA + dB")


@pytest.mark.parametrize("where", ["side", "default"])
def test_grad_apply_stream_ordered(tool, where):
    A, Cp, Ci, av, bv, G, wA, wB = stream_case()
    A.H2D(tool.device)
    C = device_csr(tool, A.M, A.N, Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, A, A, C)
    src = [upload(tool, v) for v in (G, av, bv)]
    dG = filled(tool, len(Ci))
    a, b = filled(tool, A.nnz).requires_grad_(True), filled(tool, A.nnz).requires_grad_(True)
    ballast = torch.ones(1 << 26, dtype=torch.float64, device=f"cuda:{tool.device}")
    torch.cuda.synchronize()
    stream = stream_of(tool, where)
    tool.set_option(_lib.MHS_OPT_SYNC, 0)
    try:
        with torch.cuda.stream(stream):
            busy(ballast)
            with torch.no_grad():
                for dst, s_ in zip((dG, a, b), src):
                    dst.copy_(s_, non_blocking=True)
            out = plan.apply(a, b)
            busy(ballast, 50)  # the backward's cotangent is late too
            (out * dG).sum().backward()
            both = a.grad * 2.0 + b.grad
            stream.synchronize()
            got, fwd = both.cpu().numpy(), out.detach().cpu().numpy()
    finally:
        tool.set_option(_lib.MHS_OPT_SYNC, 1)
        tool.set_stream(None)
        plan.close()
    assert_grad(got, 2.0 * wA + wB, None, np.ones(A.nnz, bool), "2 dA + dB through apply")
    _, _, Cv = orc.spgemm(A.ptr, A.col, av, A.ptr, A.col, bv, A.N)
    assert not np.isnan(fwd).any() and np.allclose(fwd, Cv, rtol=1e-9, atol=0.0)


# 10b. the argument checks that need a context and a plan: each returns MHS_ERR_INVALID with its reason in
# mhs_last_error, before any work is queued -- NaN-filled outputs stay as they are
def test_grad_argument_checks(tool):
    A, (Cp, Ci) = square_case()
    A.H2D(tool.device)
    C = device_csr(tool, A.M, A.N, Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, A, A, C)
    try:
        L = _lib.lib()
        g, av, bv = (upload(tool, new_values(n, 7)) for n in (len(Ci), A.nnz, A.nnz))
        oA, oB = filled(tool, A.nnz), filled(tool, A.nnz)
        G, Av, Bv, dA, dB = (t.data_ptr() for t in (g, av, bv, oA, oB))
        cases = [((None, Av, Bv, G, dA, dB), "null plan"),
                 ((plan.plan, Av, Bv, None, dA, dB), "null dCval"),
                 ((plan.plan, Av, Bv, G, None, None), "no output"),
                 ((plan.plan, Av, None, G, dA, None), "dAval needs Bval"),
                 ((plan.plan, None, Bv, G, None, dB), "dBval needs Aval"),
                 ((plan.plan, None, Bv, G, dA, dB), "dBval needs Aval"),
                 ((plan.plan, Av, None, G, dA, dB), "dAval needs Bval")]
        for args, word in cases:
            ms = ctypes.c_double(-1.0)
            assert L.mhs_spgemm_values_grad(tool.ctx, *args, ctypes.byref(ms)) == 3, word
            assert word in L.mhs_last_error(tool.ctx).decode(), (word, L.mhs_last_error(tool.ctx))
            assert ms.value == -1.0
        assert L.mhs_ctx_fence_default_stream(tool.ctx, 2) == 3 and "after is 0 or 1" in L.mhs_last_error(tool.ctx).decode()
        torch.cuda.synchronize()
        assert torch.isnan(oA).all().item() and torch.isnan(oB).all().item(), "a refused call writes nothing"
        # the context and the plan stay usable: one-sided calls with the unused input NULL
        assert L.mhs_spgemm_values_grad(tool.ctx, plan.plan, None, Bv, G, dA, None, None) == 0
        assert L.mhs_spgemm_values_grad(tool.ctx, plan.plan, Av, None, G, None, dB, None) == 0
        torch.cuda.synchronize()
        gA, gB = oA.cpu().numpy(), oB.cpu().numpy()
    finally:
        plan.close()
    wA, wB = ref_grad(expand(A.ptr, A.col, A.ptr, A.col, Cp, Ci, A.N), av.cpu().numpy(), bv.cpu().numpy(),
                      g.cpu().numpy(), A.nnz, A.nnz)
    assert_grad(gA, wA, None, wA != 0, "dA with Aval NULL")
    assert_grad(gB, wB, None, wB != 0, "dB with Bval NULL")


# 11. the adjoint identity, without the reference: the product is bilinear, so <G, run(X, B)> = <grad_A, X> and
# <G, run(A, Y)> = <grad_B, Y> -- the same terms summed in another order (positive values: 1e-6 relative)
def test_grad_adjoint_identity(tool):
    A = synth.fem_grid(13, 13, 40, 3, seed=5)  # 20,280 rows
    assert 15_000 <= A.M <= 25_000
    A.H2D(tool.device)
    Cd, _ = mhspgemm.spgemm(tool, A, A, timing=False)
    try:
        plan = mhspgemm.ValuesPlan(tool, A, A, Cd)
        try:
            dev = f"cuda:{tool.device}"
            gen = torch.Generator(device=dev).manual_seed(17)
            rnd = lambda n: torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * 0.9 + 0.1  # noqa: E731
            av, bv, X, Y, G = rnd(A.nnz), rnd(A.nnz), rnd(A.nnz), rnd(A.nnz), rnd(Cd.nnz)
            torch.cuda.synchronize()  # (made on torch's default stream; the tool runs on its own)
            dA, dB = plan.grad(G, av, bv)
            out = torch.empty(Cd.nnz, dtype=torch.float64, device=dev)
            plan.run(X, bv, out=out)
            lhsA = float((G * out).sum())
            plan.run(av, Y, out=out)
            lhsB = float((G * out).sum())
            rhsA, rhsB = float((dA * X).sum()), float((dB * Y).sum())
        finally:
            plan.close()
    finally:
        Cd.release()
    assert lhsA > 0 and abs(lhsA - rhsA) <= 1e-6 * lhsA, (lhsA, rhsA)
    assert lhsB > 0 and abs(lhsB - rhsB) <= 1e-6 * lhsB, (lhsB, rhsB)


# 12. torch.autograd.gradcheck on plan.apply: a few dozen rows with duplicate entries in A and in B,
# one plan on the product's pattern and one masked plan (every second entry of it); nondet_tol for dB's atomics
@functools.lru_cache(maxsize=None)
def gradcheck_case():
    p, c, v = random_csr(40, 30, 4, 3, sorted_unique=False)
    Bp, Bc, Bv = random_csr(30, 50, 5, 4, sorted_unique=False)
    Bc = Bc.copy()
    for k in range(30):  # B's rows ascending, duplicates kept
        Bc[Bp[k]:Bp[k + 1]].sort()
    A, B = mhspgemm.CSR(40, 30, p, c, v), mhspgemm.CSR(30, 50, Bp, Bc, Bv)
    dup = lambda ptr, col: any(len(set(col[ptr[i]:ptr[i + 1]].tolist())) < ptr[i + 1] - ptr[i] for i in range(len(ptr) - 1))  # noqa: E731
    assert dup(p, c) and dup(Bp, Bc), "the case needs duplicate entries in A and in B"
    return A, B, pattern_of(A, B)


@pytest.mark.parametrize("masked", [False, True])
def test_grad_gradcheck(tool, masked):
    A, B, (Cp, Ci) = gradcheck_case()
    A.H2D(tool.device)
    B.H2D(tool.device)
    if masked:
        keep = np.arange(len(Ci)) % 2 == 0
        rows = np.repeat(np.arange(A.M), np.diff(Cp))
        ptr = np.zeros(A.M + 1, np.int64)
        np.cumsum(np.bincount(rows[keep], minlength=A.M), out=ptr[1:])
        Cp, Ci = ptr.astype(np.int32), Ci[keep]
    C = device_csr(tool, A.M, B.N, Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, A, B, C, masked=masked, form="auto")
    try:
        a = upload(tool, new_values(A.nnz, 5, signed=True)).requires_grad_(True)
        b = upload(tool, new_values(B.nnz, 6, signed=True)).requires_grad_(True)
        assert torch.autograd.gradcheck(plan.apply, (a, b), nondet_tol=1e-9)
        assert torch.autograd.gradcheck(lambda x: plan.apply(x, b.detach()), (a,), nondet_tol=1e-9)
        assert torch.autograd.gradcheck(lambda y: plan.apply(a.detach(), y), (b,), nondet_tol=1e-9)
    finally:
        plan.close()
        tool.set_stream(None)
