"""GPU tests of the FP32 values plans (mhspgemm.ValuesPlan(..., dtype=torch.float32) over
mhs_values_plan_create_typed, mhs_spgemm_values_f32 and mhs_spgemm_values_grad_f32): forward, masked and backward.

The accuracy contract is derived, not measured.  The reference is the oracle (forward) or ref_grad (backward) in
FP64 on the float32-rounded inputs.  An output entry summed from m kept products, S the same sum over absolute
values, must satisfy |got - ref| <= 1.01 * m * 2^-24 * S: the any-order bound gamma_m * S of a float sum of m
rounded products (u = 2^-24, m < 2^16).  Inputs have magnitude in [0.1, 1), so nothing is subnormal.  Entries
with m = 0 must be exactly 0.0; every output starts NaN-filled and no NaN may remain.  Rows on the class edges
carry integer values and are compared exactly."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mhspgemm
from mhspgemm import _lib, synth
from oracle import oracle as orc
from _util import GOLDEN, PRODUCT_CASES, bin_zoo, device_csr, edge_val, expand, load_golden, ref_grad, tiny_zoo

pytestmark = pytest.mark.gpu

TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL, DOT = 1, 2, 3, 4, 5, 6, 7
U = 2.0 ** -24
WIDE = 1_000_000  # a column span no direct class holds


# ------------------------------------------------------------ float32 helpers (local to this file) ---
def f32(v):
    """The values rounded to float32, as the float64 array the references compute on."""
    return np.asarray(v, np.float32).astype(np.float64)


def values32(n, seed, signed=False):
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.1, 1.0, n)
    if signed:
        v *= rng.choice([-1.0, 1.0], n)
    v = f32(v)
    assert np.all((np.abs(v) >= 0.1) & (np.abs(v) <= 1.0))
    return v


def up32(tool, v):
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(f"cuda:{tool.device}")
    torch.cuda.synchronize()
    return t


def up64(tool, v):
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(f"cuda:{tool.device}")
    torch.cuda.synchronize()
    return t


def nan32(tool, n, value=float("nan")):
    out = torch.full((n,), value, dtype=torch.float32, device=f"cuda:{tool.device}")
    torch.cuda.synchronize()
    return out


def host(t):
    assert t.dtype == torch.float32
    return t.cpu().numpy().astype(np.float64)


def assert_contract(got, ref, m, S, what):
    """got (float32 results as float64) against ref within 1.01 m 2^-24 S; m = 0: exactly 0.0; no NaN."""
    assert got.shape == ref.shape and not np.isnan(got).any(), f"{what}: every entry is written"
    assert m.max(initial=0) < 2 ** 16
    assert np.all(got[m == 0] == 0.0), f"{what}: entries no kept product reaches are exactly 0.0"
    err, bound = np.abs(got - ref), 1.01 * m * U * S
    bad = err > bound
    assert not bad.any(), (f"{what}: {bad.sum()} of {len(got)} entries outside m 2^-24 S "
                           f"(worst err / bound {np.max(err[bad] / bound[bad]):.3f})")


def references(A, B, Cp, Ci, av, bv, G):
    """Forward and both gradients on the pattern (Cp, Ci), which may be a mask: reference, m and S of each."""
    pqs = expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)
    p, q, s = pqs
    nC = len(Ci)
    fwd = (np.bincount(s, av[p] * bv[q], nC), np.bincount(s, minlength=nC), np.bincount(s, np.abs(av[p] * bv[q]), nC))
    wA, wB = ref_grad(pqs, av, bv, G, A.nnz, B.nnz)
    sA, sB = ref_grad(pqs, np.abs(av), np.abs(bv), np.abs(G), A.nnz, B.nnz)
    return fwd, (wA, np.bincount(p, minlength=A.nnz), sA), (wB, np.bincount(q, minlength=B.nnz), sB), len(p)


def check32(tool, A, B, Cp, Ci, seed=1, signed=False, masked=False, form="auto", oracle_forward=False):
    """The shared checker: an FP32 plan of A*B on (Cp, Ci), seeded float32 values and cotangent, one forward and
    one backward call into NaN-filled buffers, all three outputs against the contract.  Returns info()."""
    A.H2D(tool.device)
    if B is not A:
        B.H2D(tool.device)
    C = device_csr(tool, A.M, B.N, Cp, Ci)
    av, bv, G = values32(A.nnz, seed, signed), values32(B.nnz, seed + 1000, signed), values32(len(Ci), seed + 2000, signed)
    plan = mhspgemm.ValuesPlan(tool, A, B, C, masked=masked, form=form, dtype=torch.float32)
    try:
        info = plan.info()
        assert info["dtype"] == "float32" and plan.dtype == torch.float32
        dAv, dBv, dG = up32(tool, av), up32(tool, bv), up32(tool, G)
        oC, oA, oB = nan32(tool, len(Ci)), nan32(tool, A.nnz), nan32(tool, B.nnz)
        plan.run(dAv, dBv, out=oC)
        dA, dB = plan.grad(dG, dAv, dBv, out_A=oA, out_B=oB)
        torch.cuda.synchronize()
        assert dA is oA and dB is oB
        gC, gA, gB = host(oC), host(oA), host(oB)
    finally:
        plan.close()
    (wC, mC, sC), refA, refB, kept = references(A, B, Cp, Ci, av, bv, G)
    assert kept == info["kept_products"]
    if oracle_forward:  # a plain plan: the oracle itself, on the rounded values, all-ones values and absolute values
        p_, c_, wC = orc.spgemm(A.ptr, A.col, av, B.ptr, B.col, bv, B.N)
        assert np.array_equal(p_, Cp) and np.array_equal(c_, Ci)
        mC = np.rint(orc.spgemm(A.ptr, A.col, np.ones(A.nnz), B.ptr, B.col, np.ones(B.nnz), B.N)[2]).astype(np.int64)
        sC = orc.spgemm(A.ptr, A.col, np.abs(av), B.ptr, B.col, np.abs(bv), B.N)[2]
    assert_contract(gC, wC, mC, sC, "C")
    assert_contract(gA, *refA, "dA")
    assert_contract(gB, *refB, "dB")
    return info


def pattern_of(A, B):
    Cp, Ci, _ = orc.spgemm(A.ptr, A.col, np.ones(A.nnz), B.ptr, B.col, np.ones(B.nnz), B.N)
    return Cp, Ci


def csr(t):
    M, N, p, c, v = t
    return mhspgemm.CSR(M, N, p, c, v)


# 1. golden products, forward and backward, plain plans
@pytest.mark.parametrize("name", PRODUCT_CASES)
def test_f32_golden_products(tool, name):
    d, _, _, _ = load_golden(name)
    A = mhspgemm.CSR()
    assert mhspgemm.readMtxFile(A, str(GOLDEN / d["A"])) == 0
    B = A
    if d["B"]:
        B = mhspgemm.CSR()
        assert mhspgemm.readMtxFile(B, str(GOLDEN / d["B"])) == 0
    check32(tool, A, B, *pattern_of(A, B), oracle_forward=True)


# 2. the zoos, mixed signs.  Under the FP32 classification bin_zoo's rows past an FP64 workgroup fit a block
# (21,120 contiguous columns: 84,480 B; about 19,900 scattered entries: below 19,968), so the smallest rows that
# still land in the global class are added: 19,969 entries over a wide span.
@functools.lru_cache(maxsize=None)
def zoo(name):
    if name == "global_rows":
        At, Bt = edge_val(19969, WIDE, 20000, copies=2)
    else:
        At, Bt = bin_zoo() if name == "bin_zoo" else tiny_zoo(7)
    A, B = csr(At), csr(Bt)
    return A, B, pattern_of(A, B)


_ZOO_INFO = {}


def zoo_info(tool, name):
    if name not in _ZOO_INFO:
        A, B, (Cp, Ci) = zoo(name)
        _ZOO_INFO[name] = check32(tool, A, B, Cp, Ci, seed=3, signed=True, oracle_forward=True)
    return _ZOO_INFO[name]


@pytest.mark.parametrize("name", ["bin_zoo", "tiny_zoo", "global_rows"])
def test_f32_zoo(tool, name):
    info = zoo_info(tool, name)
    if name == "tiny_zoo":
        assert info["rows"][TEAM] > 0.5 * sum(info["rows"])
    if name == "global_rows":
        assert info["rows"][GLOBAL] == 2


def test_f32_every_class_has_rows(tool):
    rows = np.sum([zoo_info(tool, n)["rows"] for n in ("bin_zoo", "tiny_zoo", "global_rows")], axis=0)
    for cls in (TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL):
        assert rows[cls] > 0, f"class {cls} has no rows under the FP32 classification"
    assert rows[DOT] == 0


# 3. class edges, exact: rows on each side of every FP32 edge with integer values of +-{1, 2, 3} -- exact in
# float32 in any order while 9 * products < 2^24 -- forward and both gradients compared with array_equal.
# (below, above): edge_val's (n, span, products); f32 / f64: the classes of the two sides under each type.
EDGES = {
    "wave_direct_span": ((200, 2048, 1000), (200, 2049, 1000), (WAVE_DIRECT, BLOCK_DIRECT), (BLOCK_DIRECT, BLOCK_DIRECT)),
    "wave_search_n": ((1024, WIDE, 2000), (1025, WIDE, 2000), (WAVE_SEARCH, BLOCK_SEARCH), (BLOCK_SEARCH, BLOCK_SEARCH)),
    "block_direct_span": ((3000, 39936, 4000), (3000, 39937, 4000), (BLOCK_DIRECT, BLOCK_SEARCH), (BLOCK_SEARCH, BLOCK_SEARCH)),
    "block_search_n": ((19968, WIDE, 20000), (19969, WIDE, 20000), (BLOCK_SEARCH, GLOBAL), (GLOBAL, GLOBAL)),
    "team_n": ((64, 100, 200), (65, 100, 200), (TEAM, WAVE_DIRECT), (TEAM, WAVE_DIRECT)),
    "team_products": ((10, 50, 512), (10, 50, 513), (TEAM, WAVE_DIRECT), (TEAM, WAVE_DIRECT)),
}
BYTE_EDGES = ("wave_direct_span", "wave_search_n", "block_direct_span", "block_search_n")


def ints(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 4, n) * rng.choice([-1, 1], n)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def edge_side(name, side):
    n, span, products = EDGES[name][side]
    assert 9 * products < 2 ** 24
    At, Bt = edge_val(n, span, products)
    A, B = csr(At), csr(Bt)
    Cp, Ci, Cv = orc.spgemm(A.ptr, A.col, A.val, B.ptr, B.col, B.val, B.N)
    G = ints(len(Ci), 13)
    wA, wB = ref_grad(expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N), A.val, B.val, G, A.nnz, B.nnz)
    return A, B, Cp, Ci, Cv, G, wA, wB


@pytest.mark.parametrize("side", [0, 1], ids=["at", "above"])
@pytest.mark.parametrize("name", list(EDGES))
def test_f32_class_edges_exact(tool, name, side):
    A, B, Cp, Ci, Cv, G, wA, wB = edge_side(name, side)
    A.H2D(tool.device)
    B.H2D(tool.device)
    C = device_csr(tool, A.M, B.N, Cp, Ci)
    classes = {}
    for dtype in ("float32", "float64"):
        plan = mhspgemm.ValuesPlan(tool, A, B, C, dtype=dtype)
        try:
            info = plan.info()
            assert info["dtype"] == dtype
            classes[dtype] = [c for c in range(8) if info["rows"][c]]
            assert sum(info["rows"]) == A.M and len(classes[dtype]) == 1, info
            if dtype == "float32":
                oC, oA, oB = nan32(tool, len(Ci)), nan32(tool, A.nnz), nan32(tool, B.nnz)
                dAv, dBv = up32(tool, A.val), up32(tool, B.val)
                plan.run(dAv, dBv, out=oC)
                plan.grad(up32(tool, G), dAv, dBv, out_A=oA, out_B=oB)
                torch.cuda.synchronize()
                gC, gA, gB = host(oC), host(oA), host(oB)
        finally:
            plan.close()
    assert classes["float32"] == [EDGES[name][2][side]], classes
    assert classes["float64"] == [EDGES[name][3][side]], classes
    if name in BYTE_EDGES:  # the type reaches classification: over the two sides the FP64 plan reports other classes
        assert EDGES[name][2] != EDGES[name][3]
    assert np.array_equal(gC, Cv), "C"
    assert np.array_equal(gA, wA), "dA"
    assert np.array_equal(gB, wB), "dB"


# 4. reduction placement (the group-reduction case of tests/test_gpu_values_grad.py, rebuilt here): B rows one
# below, at and one above the group widths and the 128-entry piece loop, A rows whose entry count leaves groups
# idle in the last step, in a narrow column window (direct classes) and a wide one (searched); dA twice, equal bits
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
        arows.append(arow(base, {1: 45, 15: 6, 16: 6, 17: 6, 127: 1, 129: 1}))     # 65 entries: a wave
        arows.append(arow(base, {1: 110, 15: 6, 16: 6, 17: 6, 128: 1, 129: 1}))    # 130 entries: a wave
        arows.append(arow(base, {1: 40, 15: 50, 16: 50, 17: 57, 127: 20, 128: 20, 129: 20}))  # 257 entries: a block
        for mix in ({1: 1, 15: 1, 17: 1}, {16: 2, 1: 3}, {17: 3}, {15: 1}, {1: 7, 16: 1, 17: 1}):  # teams
            arows.append(arow(base, mix))
    Ap = np.zeros(len(arows) + 1, np.int64)
    Ap[1:] = np.cumsum([len(r) for r in arows])
    Ac = np.array([k for r in arows for k in r], np.int32)
    A = mhspgemm.CSR(len(arows), 2 * half, Ap.astype(np.int32), Ac, np.ones(len(Ac)))
    B = mhspgemm.CSR(2 * half, N, Bp.astype(np.int32), Bc, np.ones(len(Bc)))
    return A, B, pattern_of(A, B)


def test_f32_group_reduction_placement(tool):
    A, B, (Cp, Ci) = reduction_case()
    assert {65, 130, 257} <= set(np.diff(A.ptr).tolist()) and set(np.diff(B.ptr).tolist()) == set(B_LENS)
    info = check32(tool, A, B, Cp, Ci, seed=5, oracle_forward=True)
    rows = info["rows"]
    assert rows[WAVE_DIRECT] == 2 and rows[WAVE_SEARCH] == 2, info      # the 65- and 130-entry rows, narrow and wide
    assert rows[BLOCK_DIRECT] == 1 and rows[BLOCK_SEARCH] == 1, info    # the 257-entry rows
    assert rows[TEAM] == 10, info
    C = device_csr(tool, A.M, B.N, Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, A, B, C, dtype=torch.float32)
    try:
        dG = up32(tool, values32(len(Ci), 71, signed=True))
        dBv = up32(tool, values32(B.nnz, 72, signed=True))
        a1, _ = plan.grad(dG, Bval=dBv, need_B=False)
        a2, _ = plan.grad(dG, Bval=dBv, need_B=False, out_A=nan32(tool, A.nnz))
        torch.cuda.synchronize()
        assert a1.dtype == torch.float32
        g1, g2 = a1.cpu().numpy(), a2.cpu().numpy()
    finally:
        plan.close()
    assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32)) and np.any(g1 != 0.0), "dA: the same bits on every call"


# 5. masked plans: L*L on L's pattern (L the strictly lower triangle of a small symmetrised power-law graph),
# and a mask smaller than the product (every second entry of a random product's pattern), every form
@functools.lru_cache(maxsize=None)
def triangle_case(n=2000):
    Gm = synth.powerlaw(n, seed=3)
    r = np.repeat(np.arange(Gm.M, dtype=np.int64), np.diff(Gm.ptr))
    c = Gm.col.astype(np.int64)
    off = r != c
    key = np.unique(np.maximum(r[off], c[off]) * n + np.minimum(r[off], c[off]))
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(key // n, minlength=n), out=ptr[1:])
    return mhspgemm.CSR(n, n, ptr.astype(np.int32), (key % n).astype(np.int32), np.ones(len(key)))


@functools.lru_cache(maxsize=None)
def thinned_case():
    rng = np.random.default_rng(9)

    def rand(M, N, per, seed):
        r = np.random.default_rng(seed)
        lens = r.poisson(per, M)
        key = np.unique(np.repeat(np.arange(M, dtype=np.int64), lens) * N + r.integers(0, N, lens.sum()))
        ptr = np.zeros(M + 1, np.int64)
        np.cumsum(np.bincount(key // N, minlength=M), out=ptr[1:])
        return mhspgemm.CSR(M, N, ptr.astype(np.int32), (key % N).astype(np.int32), np.ones(len(key)))

    A, B = rand(600, 500, 7, 1), rand(500, 3000, 12, 2)
    Cp, Ci = pattern_of(A, B)
    keep = rng.random(len(Ci)) < 0.5
    rows = np.repeat(np.arange(A.M), np.diff(Cp))
    Mp = np.zeros(A.M + 1, np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=A.M), out=Mp[1:])
    return A, B, Mp.astype(np.int32), Ci[keep]


@pytest.mark.parametrize("form", ["product", "dot", "auto"])
@pytest.mark.parametrize("case", ["triangle", "thinned"])
def test_f32_masked_forms(tool, case, form):
    if case == "triangle":
        L = triangle_case()
        A, B, Mp, Mc = L, L, L.ptr, L.col
    else:
        A, B, Mp, Mc = thinned_case()
    info = check32(tool, A, B, Mp, Mc, seed=9, signed=True, masked=True, form=form)
    assert 0 < info["kept_products"] < info["products"], "the case needs products outside the mask"
    if form != "auto":
        assert (info["dot"] > 0) == (form == "dot"), (form, info)
    if case == "triangle":  # mask entries no product reaches: exactly 0.0 (assert_contract's m = 0), and they exist
        p, q, s = expand(A.ptr, A.col, B.ptr, B.col, Mp, Mc, B.N)
        assert np.count_nonzero(np.bincount(s, minlength=len(Mc)) == 0) > 0


# 6. one-sided backward: the other buffer's NaNs stay, and the other operand's values may be None
@functools.lru_cache(maxsize=None)
def square_case():
    rng = np.random.default_rng(21)
    M = 1500
    lens = rng.poisson(8, M)
    key = np.unique(np.repeat(np.arange(M, dtype=np.int64), lens) * M + rng.integers(0, M, lens.sum()))
    ptr = np.zeros(M + 1, np.int64)
    np.cumsum(np.bincount(key // M, minlength=M), out=ptr[1:])
    A = mhspgemm.CSR(M, M, ptr.astype(np.int32), (key % M).astype(np.int32), np.ones(len(key)))
    Cp, Ci = pattern_of(A, A)
    av, bv, G = values32(A.nnz, 91), values32(A.nnz, 92), values32(len(Ci), 93)
    return A, Cp, Ci, av, bv, G, references(A, A, Cp, Ci, av, bv, G)


def test_f32_one_side_only(tool):
    A, Cp, Ci, av, bv, G, (_, refA, refB, _) = square_case()
    A.H2D(tool.device)
    C = device_csr(tool, A.M, A.N, Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, A, A, C, dtype="float32")
    try:
        dG, dAv, dBv = up32(tool, G), up32(tool, av), up32(tool, bv)
        oA, oB = nan32(tool, A.nnz), nan32(tool, A.nnz)
        rA = plan.grad(dG, Aval=None, Bval=dBv, need_B=False, out_A=oA, out_B=oB)
        torch.cuda.synchronize()
        assert rA[0] is oA and rA[1] is None
        assert torch.isnan(oB).all().item(), "need_B=False: out_B's NaNs untouched"
        gA = host(oA)
        oA.fill_(float("nan"))
        torch.cuda.synchronize()
        rB = plan.grad(dG, Aval=dAv, Bval=None, need_A=False, out_A=oA, out_B=oB, timed=True)
        torch.cuda.synchronize()
        assert rB[0] is None and rB[1] is oB and rB[2] > 0.0
        assert torch.isnan(oA).all().item(), "need_A=False: out_A's NaNs untouched"
        gB = host(oB)
        with pytest.raises(ValueError):  # an FP32 plan has no values of its own to fall back on
            plan.grad(dG, Aval=dAv, Bval=None)
        with pytest.raises(ValueError):
            plan.run(dAv, None, out=nan32(tool, len(Ci)))
    finally:
        plan.close()
    assert_contract(gA, *refA, "dA alone")
    assert_contract(gB, *refB, "dB alone")


# 7. type checks: a tensor of the other type raises in the wrapper; at the C level both wrong-type calls return
# MHS_ERR_INVALID naming both types, before any work is queued -- NaN-filled outputs stay as they are
def test_f32_wrong_type_is_refused(tool):
    A, Cp, Ci, av, bv, G, _ = square_case()
    A.H2D(tool.device)
    C = device_csr(tool, A.M, A.N, Cp, Ci)
    L = _lib.lib()
    p32 = mhspgemm.ValuesPlan(tool, A, A, C, dtype=torch.float32)
    p64 = mhspgemm.ValuesPlan(tool, A, A, C)
    try:
        assert p32.info()["dtype"] == "float32" and p64.info()["dtype"] == "float64"
        dt = ctypes.c_int(-1)
        assert L.mhs_values_plan_dtype(p32.plan, ctypes.byref(dt)) == 0 and dt.value == _lib.MHS_F32
        assert L.mhs_values_plan_dtype(p64.plan, ctypes.byref(dt)) == 0 and dt.value == _lib.MHS_F64
        t32 = [up32(tool, v) for v in (av, bv, G)]
        t64 = [up64(tool, v) for v in (av, bv, G)]
        o32 = [nan32(tool, n) for n in (len(Ci), A.nnz, A.nnz)]
        o64 = [torch.full((n,), float("nan"), dtype=torch.float64, device=f"cuda:{tool.device}")
               for n in (len(Ci), A.nnz, A.nnz)]
        torch.cuda.synchronize()
        # the wrapper
        with pytest.raises(ValueError, match="float32"):
            p32.run(t64[0], t64[1], out=o32[0])
        with pytest.raises(ValueError, match="float32"):
            p32.run(t32[0], t32[1], out=o64[0])
        with pytest.raises(ValueError, match="float32"):
            p32.grad(t64[2], t32[0], t32[1])
        with pytest.raises(ValueError, match="float64"):
            p64.run(t32[0], t32[1], out=o64[0])
        with pytest.raises(ValueError, match="float64"):
            p64.grad(t32[2], t64[0], t64[1])
        with pytest.raises(ValueError, match="float64"):
            p64.apply(t32[0], t32[1])
        # the library
        ms = ctypes.c_double(-1.0)
        a32, b32, g32 = (t.data_ptr() for t in t32)
        a64, b64, g64 = (t.data_ptr() for t in t64)
        c32, da32, db32 = (t.data_ptr() for t in o32)
        c64, da64, db64 = (t.data_ptr() for t in o64)
        calls = [lambda: L.mhs_spgemm_values_f32(tool.ctx, p64.plan, a32, b32, c32, ctypes.byref(ms)),
                 lambda: L.mhs_spgemm_values_grad_f32(tool.ctx, p64.plan, a32, b32, g32, da32, db32, ctypes.byref(ms)),
                 lambda: L.mhs_spgemm_values(tool.ctx, p32.plan, a64, b64, c64, ctypes.byref(ms)),
                 lambda: L.mhs_spgemm_values_grad(tool.ctx, p32.plan, a64, b64, g64, da64, db64, ctypes.byref(ms))]
        for call in calls:
            assert call() == 3
            msg = L.mhs_last_error(tool.ctx).decode()
            assert "FP32" in msg and "FP64" in msg, msg
            assert ms.value == -1.0
        torch.cuda.synchronize()
        for o in o32 + o64:
            assert torch.isnan(o).all().item(), "a refused call writes nothing"
        # plan creation: a dtype that is no mhs_dtype; MHS_F64 through _typed is the plain plan
        a, c = A.c_view(), C.c_view()
        for bad in (2, -1, 8):
            out = ctypes.c_void_p()
            assert L.mhs_values_plan_create_typed(tool.ctx, ctypes.byref(a), ctypes.byref(a), ctypes.byref(c), 0, 0, bad,
                                                  ctypes.byref(out)) == 3
            assert "dtype" in L.mhs_last_error(tool.ctx).decode() and not out.value
        out = ctypes.c_void_p()
        assert L.mhs_values_plan_create_typed(tool.ctx, ctypes.byref(a), ctypes.byref(a), ctypes.byref(c), 0, 77, _lib.MHS_F64,
                                              ctypes.byref(out)) == 0  # (masked == 0 ignores form)
        try:
            i1, i2 = _lib.mhs_values_info(), _lib.mhs_values_info()
            assert L.mhs_values_plan_info(out, ctypes.byref(i1)) == 0 and L.mhs_values_plan_info(p64.plan, ctypes.byref(i2)) == 0
            assert list(i1.rows) == list(i2.rows) and i1.products == i2.products
            assert L.mhs_values_plan_dtype(out, ctypes.byref(dt)) == 0 and dt.value == _lib.MHS_F64
            assert L.mhs_spgemm_values(tool.ctx, out, a64, b64, c64, None) == 0
        finally:
            L.mhs_values_plan_destroy(tool.ctx, out)
        # the plans stay usable, each with its own type
        p32.run(t32[0], t32[1], out=o32[0])
        p64.run(t64[0], t64[1], out=o64[0])
        torch.cuda.synchronize()
        assert torch.all(o64[0] > 0).item() and torch.all(o32[0] > 0).item()
        assert torch.all((o32[0].double() - o64[0]).abs() <= 1e-3 * o64[0]).item()
    finally:
        p32.close()
        p64.close()


# 8. autograd on float32 leaves, ordered on torch's current stream with MHS_OPT_SYNC 0 (the method of
# tests/test_gpu_values_grad.py::test_grad_apply_stream_ordered): the inputs hold NaN until a copy queued behind
# a long torch kernel on the same stream fills them, and only that stream is synchronised
def busy(x, rounds=150):
    for _ in range(rounds):
        x.mul_(1.0000001)


@pytest.mark.parametrize("where", ["side", "default"])
def test_f32_apply_stream_ordered(tool, where):
    A, Cp, Ci, av, bv, G, ((wC, mC, sC), (wA, mA, sA), (wB, mB, sB), _) = square_case()
    A.H2D(tool.device)
    C = device_csr(tool, A.M, A.N, Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, A, A, C, dtype=torch.float32)
    src = [up32(tool, v) for v in (G, av, bv)]
    dG = nan32(tool, len(Ci))
    a, b = nan32(tool, A.nnz).requires_grad_(True), nan32(tool, A.nnz).requires_grad_(True)
    ballast = torch.ones(1 << 26, dtype=torch.float64, device=f"cuda:{tool.device}")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(tool.device) if where == "side" else torch.cuda.default_stream(tool.device)
    tool.set_option(_lib.MHS_OPT_SYNC, 0)
    try:
        with torch.cuda.stream(stream):
            assert (torch.cuda.current_stream(tool.device).cuda_stream != 0) == (where == "side")
            busy(ballast)
            with torch.no_grad():
                for dst, s_ in zip((dG, a, b), src):
                    dst.copy_(s_, non_blocking=True)
            out = plan.apply(a, b)
            busy(ballast, 50)  # the backward's cotangent is late too
            out.backward(dG)
            ga, gb = a.grad.clone(), b.grad.clone()
            stream.synchronize()
            assert out.dtype == torch.float32 and ga.dtype == torch.float32 and gb.dtype == torch.float32
            gA, gB, fwd = host(ga), host(gb), host(out.detach())
    finally:
        tool.set_option(_lib.MHS_OPT_SYNC, 1)
        tool.set_stream(None)
        plan.close()
    assert_contract(fwd, wC, mC, sC, "apply's forward")
    assert_contract(gA, wA, mA, sA, "dA through apply")
    assert_contract(gB, wB, mB, sB, "dB through apply")
