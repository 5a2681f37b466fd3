"""GPU tests of the mixed-precision values plans (mhspgemm.ValuesPlan(..., dtype="float32", accum="float64") over
mhs_values_plan_create_accum): float32 values, products and sums in double, one rounding to float at the store.

The contract is the header's and is derived, not measured.  On the team, wave, block and dot classes an entry of m
kept products, E their exact sum and S the sum of their absolute values, satisfies
    |got - E| <= 2^-24 |E| + m 2^-53 S (1 + 2^-24):
a float x float product is exact in double, a double sum of m terms in any order is within m 2^-53 S of E, and the
one rounding to float adds 2^-24 of the sum.  E is exact_forward's long-double sum on the float-rounded inputs.  Rows
of the global class keep C's float segment as their accumulator and are held to the FP32 plans' 1.01 m 2^-24 S; they
are picked out by the plan header's classification at the sum bytes 8 W, restated here and checked against info().
The backward is the FP32 plans': float kernels, 1.01 m 2^-24 S against ref_grad in double.  Integer-valued cases are
compared exactly.  Every output starts NaN-filled."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mhspgemm
from mhspgemm import _lib, synth
from oracle import oracle as orc
from _util import (FINITE, GOLDEN, PRODUCT_CASES, U64, bin_zoo, classes_of, device_csr, edge_val, edge_values, exact_forward,
                   expand, inject_nonfinite, load_edges, load_golden, nonfinite_reference, ref_grad, row_shapes, tiny_zoo)

pytestmark = pytest.mark.gpu

NONE, TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL, DOT = range(8)
LDS_CLASSES = (TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH)
U32 = 2.0 ** -24
WIDE = 1_000_000  # a column span no direct class holds
WIDTHS = (1, 2, 4)
# csrc/mhs_valplan.hpp at the sum bytes sb: wave-direct span, wave-search n, block-direct span, block-search n
CAPS = {4: (2048, 1024, 39936, 19968), 8: (1024, 682, 19968, 13312), 16: (512, 408, 9984, 7986), 32: (256, 226, 4992, 4436)}
BLOCK_SMALL = 32768  # block launches of at most this much LDS run 256 threads, else 1024


def val_class(n, span, products, sb):
    """The class of a plain plan's row at sum bytes sb (val_class of csrc/mhs_valplan.hpp, restated)."""
    wd, ws, bd, bs = CAPS[sb]
    if n <= 0:
        return NONE
    if n <= 64 and products <= 512:
        return TEAM
    if products <= 0:
        return GLOBAL
    wave = products <= 2048
    if wave and span <= wd:
        return WAVE_DIRECT
    if span <= bd and span <= 16 * n:
        return BLOCK_DIRECT
    if wave and n <= ws:
        return WAVE_SEARCH
    if span <= bd:
        return BLOCK_DIRECT
    return BLOCK_SEARCH if n <= bs else GLOBAL


def row_classes(At, Bt, Cp, Ci, sb):
    sh = row_shapes(At, Bt, Cp, Ci)
    return np.array([val_class(int(n), int(s), int(f), sb) for n, s, f in zip(sh["n"], sh["colspan"], sh["flop"])], np.int64)


# ------------------------------------------------------------------ values, uploads, the bounds ---
def f32(v):
    return np.asarray(v, np.float32).astype(np.float64)


def values32(shape, seed, signed=True):
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.1, 1.0, shape)
    if signed:
        v *= rng.choice([-1.0, 1.0], shape)
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


def nan32(tool, shape):
    out = torch.full(shape if isinstance(shape, tuple) else (shape,), float("nan"), dtype=torch.float32,
                     device=f"cuda:{tool.device}")
    torch.cuda.synchronize()
    return out


def host(t):
    assert t.dtype == torch.float32
    return t.cpu().numpy().astype(np.float64)


def assert_mixed(got, ref_ld, m, S, glob, what):
    """got (float32 results as float64) against the long-double reference: the mixed bound, or on the entries of
    global-class rows (glob) the FP32 bound; m = 0: exactly 0.0; no NaN.  Prints the worst err / bound of both kinds."""
    got = np.asarray(got, np.float64)
    glob = np.broadcast_to(np.asarray(glob, bool), got.shape)
    assert got.shape == ref_ld.shape == m.shape == S.shape, f"{what}: shape"
    assert not np.isnan(got).any(), f"{what}: every entry is written"
    assert np.all(got[m == 0] == 0.0), f"{what}: entries no kept product reaches are exactly 0.0"
    assert m.max(initial=0) < 2 ** 16
    ml = m.astype(np.longdouble)
    err = np.abs(got.astype(np.longdouble) - ref_ld)
    mixed = np.longdouble(U32) * np.abs(ref_ld) + ml * np.longdouble(U64) * S * (1 + np.longdouble(U32))
    bound = np.where(glob, np.longdouble(1.01 * U32) * ml * S, mixed)
    ratio = np.zeros(len(got), np.longdouble)
    np.divide(err, bound, out=ratio, where=bound > 0)
    worst = [float(ratio[k].max(initial=0.0)) for k in (~glob, glob)]
    print(f"mixed bound, {what}: worst err / bound {worst[0]:.3f} over {int((~glob).sum())} entries, "
          f"FP32 bound (global rows) {worst[1]:.3f} over {int(glob.sum())}, max m {m.max(initial=0)}")
    bad = err > bound
    assert not bad.any(), (f"{what}: {bad.sum()} of {len(got)} entries outside their bound "
                           f"({int((bad & ~glob).sum())} of them held to the mixed bound; worst err / bound {max(worst):.3e})")


def assert_f32_bound(got, ref, m, S, what):
    """The FP32 plans' contract (tests/test_gpu_values_f32.py): 1.01 m 2^-24 S; m = 0: exactly 0.0; no NaN."""
    assert got.shape == ref.shape and not np.isnan(got).any(), f"{what}: every entry is written"
    assert m.max(initial=0) < 2 ** 16
    assert np.all(got[m == 0] == 0.0), f"{what}: entries no kept product reaches are exactly 0.0"
    err, bound = np.abs(got - ref), 1.01 * m * U32 * S
    ratio = np.zeros(len(got))
    np.divide(err, bound, out=ratio, where=bound > 0)
    print(f"f32 bound, {what}: worst err / bound {ratio.max(initial=0.0):.3f} over {len(got)} entries")
    assert not (err > bound).any(), f"{what}: {(err > bound).sum()} entries outside 1.01 m 2^-24 S"


def csr(t):
    M, N, p, c, v = t
    return mhspgemm.CSR(M, N, p, c, v)


def pattern_of(A, B):
    Cp, Ci, _ = orc.spgemm(A.ptr, A.col, np.ones(A.nnz), B.ptr, B.col, np.ones(B.nnz), B.N)
    return Cp, Ci


def tuple_of(X):
    return (X.M, X.N, X.ptr, X.col, X.val)


def make_plan(tool, A, B, Cp, Ci, W=1, dtype="float32", accum="float64", **kw):
    A.H2D(tool.device)
    if B is not A:
        B.H2D(tool.device)
    C = device_csr(tool, A.M, B.N, Cp, Ci)
    return mhspgemm.ValuesPlan(tool, A, B, C, dtype=dtype, width=W, accum=accum, **kw)


def run_sets(tool, plan, av, bv, nC):
    """The forward on the value sets av [nb, nnzA] and bv [nb, nnzB] into a NaN-filled output: float64 [nb, nC]."""
    out = nan32(tool, (av.shape[0], nC))
    plan.run_batched(up32(tool, av), up32(tool, bv), out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------ 1. exact cancellation, once per class ---
# A C row of n entries over `span` columns: three B rows hold the row's columns with the values 4097, 4096 and small
# integers; the A row holds r pairs (4097, -4096) on the first two and t small integers on the third.  Every entry is
# r (4097^2 - 4096^2) = 8193 r plus small integers: an integer below 2^24, which a double sum reaches exactly in any
# order (every partial sum is an integer below 2^53) and a float sum cannot: 4097^2 = 16,785,409 rounds to 16,785,408.
# (n, span, r, t, copies): products = n (2 r + t)
CANCEL_SMALL = {TEAM: (20, 50, 2, 1, 40), WAVE_DIRECT: (100, 200, 2, 1, 5), WAVE_SEARCH: (100, WIDE, 2, 1, 5),
                BLOCK_DIRECT: (100, 300, 10, 1, 5), BLOCK_SEARCH: (300, WIDE, 3, 1, 5)}
CANCEL_BIG = {BLOCK_DIRECT: (300, 4500, 1, 1, 3), BLOCK_SEARCH: (3000, WIDE, 1, 1, 3)}  # past BLOCK_SMALL at every width


@functools.lru_cache(maxsize=None)
def cancel_case(big):
    rng = np.random.default_rng(23)
    spec = CANCEL_BIG if big else CANCEL_SMALL
    arows, brows, base = [], [], 0
    kinds = []
    for cls, (n, span, r, t, copies) in spec.items():
        for _ in range(copies):
            cols = base + np.unique(np.round(np.linspace(0, span - 1, n)).astype(np.int64))
            assert len(cols) == n and cols[-1] - cols[0] + 1 == span
            k = len(brows)
            brows += [(cols, np.full(n, 4097.0)), (cols, np.full(n, 4096.0)), (cols, edge_values(n, int(rng.integers(1 << 30))))]
            arows.append(([k, k + 1] * r + [k + 2] * t, [4097.0, -4096.0] * r + edge_values(t, int(rng.integers(1 << 30))).tolist()))
            kinds.append(cls)
            base += 64
    N = base + WIDE + 64
    Ap = np.zeros(len(arows) + 1, np.int64)
    Ap[1:] = np.cumsum([len(k) for k, _ in arows])
    Bp = np.zeros(len(brows) + 1, np.int64)
    Bp[1:] = np.cumsum([len(c) for c, _ in brows])
    A = mhspgemm.CSR(len(arows), len(brows), Ap.astype(np.int32), np.concatenate([k for k, _ in arows]).astype(np.int32),
                     np.concatenate([v for _, v in arows]).astype(np.float64))
    B = mhspgemm.CSR(len(brows), N, Bp.astype(np.int32), np.concatenate([c for c, _ in brows]).astype(np.int32),
                     np.concatenate([v for _, v in brows]))
    Cp, Ci = pattern_of(A, B)
    p, q, s = expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)
    want = np.bincount(s, A.val[p] * B.val[q], len(Ci))  # integers: exact in float64
    assert np.all(want == np.rint(want)) and np.abs(want).max() < 2 ** 24 and np.all(f32(want) == want)
    # the test's own guard that the inputs discriminate: float32 products summed in float32 miss every entry
    w32 = A.val[p].astype(np.float32) * B.val[q].astype(np.float32)
    assert w32.dtype == np.float32
    naive = np.zeros(len(Ci), np.float32)
    np.add.at(naive, s, w32)
    assert naive.dtype == np.float32 and np.all(naive.astype(np.float64) != want), "float32 sums must miss the integer reference"
    return A, B, Cp, Ci, want, np.array(kinds)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("big", [False, True], ids=["block256", "block1024"])
def test_mixed_exact_cancellation_every_class(tool, big, W):
    A, B, Cp, Ci, want, kinds = cancel_case(big)
    sb = 8 * W
    cls = row_classes(tuple_of(A), tuple_of(B), Cp, Ci, sb)
    assert np.array_equal(cls, kinds), "the rows are of the classes they were built for"
    need = {c: max((sb * s if c == BLOCK_DIRECT else (sb + 4) * n) for cc, (n, s, _, _, _) in
                   (CANCEL_BIG if big else CANCEL_SMALL).items() if cc == c) for c in (BLOCK_DIRECT, BLOCK_SEARCH)}
    assert all((v > BLOCK_SMALL) == big for v in need.values()), need  # 1024-thread block kernels, or 256-thread ones
    nb = W + 1  # (a remainder pass; the sets differ by an exact power of two)
    scale = 2.0 ** -np.arange(nb)
    av = A.val[None, :] * scale[:, None]
    bv = np.repeat(B.val[None, :], nb, axis=0)
    plan = make_plan(tool, A, B, Cp, Ci, W)
    try:
        info = plan.info()
        assert info["accum"] == "float64" and info["dtype"] == "float32" and info["width"] == W
        for c in kinds:
            assert info["rows"][c] == np.count_nonzero(kinds == c) > 0, info
        got = run_sets(tool, plan, av, bv, len(Ci))
    finally:
        plan.close()
    for b in range(nb):
        assert np.array_equal(got[b], want * scale[b]), f"set {b}: the double sum is the integer reference"
    # the dot class: the same rows on a masked plan in dot form (the mask is the whole product)
    if not big:
        plan = make_plan(tool, A, B, Cp, Ci, W, masked=True, form="dot")
        try:
            info = plan.info()
            assert info["rows"][DOT] == A.M and info["accum"] == "float64", info
            got = run_sets(tool, plan, av, bv, len(Ci))
        finally:
            plan.close()
        for b in range(nb):
            assert np.array_equal(got[b], want * scale[b]), f"dot rows, set {b}"


def test_mixed_cancellation_is_missed_by_float_sums(tool):
    """The FP32 plan on the same inputs sums in float and misses the integer reference: the case discriminates on the
    device too."""
    A, B, Cp, Ci, want, _ = cancel_case(False)
    plan = make_plan(tool, A, B, Cp, Ci, 1, accum=None)
    try:
        assert plan.info()["accum"] is None
        got = run_sets(tool, plan, A.val[None, :], B.val[None, :], len(Ci))[0]
    finally:
        plan.close()
    assert np.all(got != want)


# ------------------------------------------------------------------ 2. the bound ---
@functools.lru_cache(maxsize=None)
def bound_input(name):
    if name in PRODUCT_CASES:
        d, _, _, _ = load_golden(name)
        A = mhspgemm.CSR()
        assert mhspgemm.readMtxFile(A, str(GOLDEN / d["A"])) == 0
        B = A
        if d["B"]:
            B = mhspgemm.CSR()
            assert mhspgemm.readMtxFile(B, str(GOLDEN / d["B"])) == 0
    else:
        At, Bt = bin_zoo() if name == "bin_zoo" else tiny_zoo(7)
        A, B = csr(At), csr(Bt)
    Cp, Ci = pattern_of(A, B)
    return A, B, Cp, Ci


@functools.lru_cache(maxsize=None)
def bound_reference(name, nb, shared_b=False):
    """Seeded float32 value sets with mixed signs and, per set, exact_forward's (E, m, S).  Computed once, read only."""
    A, B, Cp, Ci = bound_input(name)
    av = values32((nb, A.nnz), 31)
    bv = values32((1 if shared_b else nb, B.nnz), 32)
    refs = [exact_forward(A, B, Cp, Ci, av[b], bv[0 if shared_b else b]) for b in range(nb)]
    for x in (av, bv):
        x.setflags(write=False)
    return av, bv, refs


def global_entries(name, W, info):
    """Per C entry, whether its row is of the global class at sb = 8 W; the count agrees with info()."""
    A, B, Cp, Ci = bound_input(name)
    cls = row_classes(tuple_of(A), tuple_of(B), Cp, Ci, 8 * W)
    for c in range(7):
        assert info["rows"][c] == np.count_nonzero(cls == c), (c, info)
    return np.repeat(cls == GLOBAL, np.diff(Cp))


@pytest.mark.parametrize("name", PRODUCT_CASES + ["bin_zoo", "tiny_zoo"])
def test_mixed_bound(tool, name):
    A, B, Cp, Ci = bound_input(name)
    av, bv, refs = bound_reference(name, 1)
    plan = make_plan(tool, A, B, Cp, Ci, 1)
    try:
        info = plan.info()
        out = nan32(tool, len(Ci))
        plan.run(up32(tool, av[0]), up32(tool, bv[0]), out=out)  # (the unbatched entry point)
        torch.cuda.synchronize()
        got = host(out)
    finally:
        plan.close()
    glob = global_entries(name, 1, info)
    if name == "bin_zoo":
        assert glob.any() and info["rows"][GLOBAL] > 0, "bin_zoo has rows past one workgroup"
        assert all(info["rows"][c] > 0 for c in LDS_CLASSES), info
    assert_mixed(got, *refs[0], glob, name)  # every entry: none of a non-global row is left out


# ------------------------------------------------------------------ 3. the classes are FP64's ---
@pytest.mark.parametrize("W", WIDTHS)
def test_mixed_classes_are_fp64s(tool, W):
    A, B, Cp, Ci = bound_input("bin_zoo")
    rows = {}
    for key, dtype, accum in (("mixed", "float32", "float64"), ("f64", "float64", None), ("f32", "float32", None),
                              ("f64acc", "float64", "float64")):
        plan = make_plan(tool, A, B, Cp, Ci, W, dtype=dtype, accum=accum)
        try:
            info = plan.info()
            rows[key] = info["rows"]
            assert info["accum"] == ("float64" if key == "mixed" else None) and info["dtype"] == dtype and info["width"] == W
        finally:
            plan.close()
    assert rows["mixed"] == rows["f64"] == rows["f64acc"], rows
    assert rows["mixed"] != rows["f32"], "the FP32 plan's rows move (tests/test_gpu_values_f32.py)"


# (at, above): edge_val's (n, span, products) and the classes of the two sides at the sum bytes sb = 8 W
BYTE_EDGES = {
    8: {"wave_direct_span": ((200, 1024, 1000), (200, 1025, 1000), (WAVE_DIRECT, BLOCK_DIRECT)),
        "wave_search_n": ((682, WIDE, 2000), (683, WIDE, 2000), (WAVE_SEARCH, BLOCK_SEARCH)),
        "block_direct_span": ((3000, 19968, 4000), (3000, 19969, 4000), (BLOCK_DIRECT, BLOCK_SEARCH)),
        "block_search_n": ((13312, WIDE, 13400), (13313, WIDE, 13400), (BLOCK_SEARCH, GLOBAL))},
    16: {"wave_direct_span": ((200, 512, 1000), (200, 513, 1000), (WAVE_DIRECT, BLOCK_DIRECT)),
         "wave_search_n": ((408, WIDE, 2000), (409, WIDE, 2000), (WAVE_SEARCH, BLOCK_SEARCH)),
         "block_direct_span": ((3000, 9984, 4000), (3000, 9985, 4000), (BLOCK_DIRECT, BLOCK_SEARCH)),
         "block_search_n": ((7986, WIDE, 8000), (7987, WIDE, 8000), (BLOCK_SEARCH, GLOBAL))},
    32: {"wave_direct_span": ((200, 256, 1000), (200, 257, 1000), (WAVE_DIRECT, BLOCK_DIRECT)),
         "wave_search_n": ((226, WIDE, 2000), (227, WIDE, 2000), (WAVE_SEARCH, BLOCK_SEARCH)),
         "block_direct_span": ((3000, 4992, 4000), (3000, 4993, 4000), (BLOCK_DIRECT, BLOCK_SEARCH)),
         "block_search_n": ((4436, WIDE, 4500), (4437, WIDE, 4500), (BLOCK_SEARCH, GLOBAL))},
}
TEAM_EDGES = {"team_n": ((64, 100, 200), (65, 100, 200), (TEAM, WAVE_DIRECT)),
              "team_products": ((10, 50, 512), (10, 50, 513), (TEAM, WAVE_DIRECT))}
EDGE_NAMES = list(BYTE_EDGES[8]) + list(TEAM_EDGES)


@functools.lru_cache(maxsize=None)
def edge_rows_of(n, span, products):
    assert 9 * products < 2 ** 24  # integers of +-{1, 2, 3}: exact in float32 too, in any order
    A, B = (csr(t) for t in edge_val(n, span, products))
    Cp, Ci = pattern_of(A, B)
    return A, B, Cp, Ci, expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)


def run_edge(tool, n, span, products, W, want_class):
    A, B, Cp, Ci, (p, q, s) = edge_rows_of(n, span, products)
    nb = W + 1
    av = np.stack([edge_values(A.nnz, 50 + b) for b in range(nb)])
    bv = np.stack([edge_values(B.nnz, 80 + b) for b in range(nb)])
    plan = make_plan(tool, A, B, Cp, Ci, W)
    try:
        info = plan.info()
        classes = [c for c in range(8) if info["rows"][c]]
        assert sum(info["rows"]) == A.M and classes == [want_class] == [val_class(n, span, products, 8 * W)], info
        got = run_sets(tool, plan, av, bv, len(Ci))
    finally:
        plan.close()
    for b in range(nb):
        assert np.array_equal(got[b], np.bincount(s, av[b][p] * bv[b][q], len(Ci))), f"set {b}"


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("side", [0, 1], ids=["at", "above"])
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_mixed_class_edges_exact(tool, name, side, W):
    edge = TEAM_EDGES[name] if name in TEAM_EDGES else BYTE_EDGES[8 * W][name]
    run_edge(tool, *edge[side], W, edge[2][side])


VALUE_RUNGS = load_edges()["values"]  # the sb = 8 table's rungs, printed from the header


@pytest.mark.parametrize("side", ["last", "first"])
@pytest.mark.parametrize("rung", VALUE_RUNGS, ids=[r["name"] for r in VALUE_RUNGS])
def test_mixed_header_rungs_exact(tool, rung, side):
    """A width-1 mixed plan classifies at sb = 8: the rows on both sides of every rung of the header's own table."""
    r = rung[side]
    run_edge(tool, r["params"]["n"], r["params"]["span"], r["params"]["products"], 1, r["class_index"])


# ------------------------------------------------------------------ 4. masked plans ---
@functools.lru_cache(maxsize=None)
def triangle_case(n=2000):
    Gm = synth.powerlaw(n, seed=3)
    r = np.repeat(np.arange(Gm.M, dtype=np.int64), np.diff(Gm.ptr))
    c = Gm.col.astype(np.int64)
    off = r != c
    key = np.unique(np.maximum(r[off], c[off]) * n + np.minimum(r[off], c[off]))
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(key // n, minlength=n), out=ptr[1:])
    L = mhspgemm.CSR(n, n, ptr.astype(np.int32), (key % n).astype(np.int32), np.ones(len(key)))
    return L, L, L.ptr, L.col


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


@functools.lru_cache(maxsize=None)
def mask_reference(case, nb):
    A, B, Mp, Mc = triangle_case() if case == "triangle" else thinned_case()
    av, bv = values32((nb, A.nnz), 41), values32((nb, B.nnz), 42)
    refs = [exact_forward(A, B, Mp, Mc, av[b], bv[b]) for b in range(nb)]
    return av, bv, refs


@pytest.mark.parametrize("form", ["product", "dot", "auto"])
@pytest.mark.parametrize("case", ["triangle", "thinned"])
def test_mixed_masked_forms(tool, case, form):
    A, B, Mp, Mc = triangle_case() if case == "triangle" else thinned_case()
    nb = 3
    av, bv, refs = mask_reference(case, nb)
    plan = make_plan(tool, A, B, Mp, Mc, 2, masked=True, form=form)
    one = make_plan(tool, A, B, Mp, Mc, 1, masked=True, form=form)
    try:
        info = plan.info()
        assert info["accum"] == "float64" and 0 < info["kept_products"] < info["products"], info
        assert info["rows"][GLOBAL] == 0, "no row of these masks is of the global class: every entry has the mixed bound"
        if form != "auto":
            assert (info["dot"] > 0) == (form == "dot"), (form, info)
        dA, dB = up32(tool, av), up32(tool, bv)
        outs = [nan32(tool, (nb, len(Mc))) for _ in range(2)]
        for o in outs:  # twice, each into a NaN-filled output
            plan.run_batched(dA, dB, out=o)
        alone = nan32(tool, (nb, len(Mc)))
        for b in range(nb):
            one.run(dA[b], dB[b], out=alone[b])
        torch.cuda.synchronize()
        g1, g2, ga = (o.cpu().numpy() for o in (*outs, alone))
    finally:
        plan.close()
        one.close()
    for b in range(nb):
        assert_mixed(g1[b].astype(np.float64), *refs[b], False, f"{case} {form} set {b}")
        assert_mixed(ga[b].astype(np.float64), *refs[b], False, f"{case} {form} set {b} alone")
    if form == "dot":  # every row with mask and A entries is a dot row: a fixed order, the same bits
        assert info["dot"] == np.count_nonzero((np.diff(Mp) > 0) & (np.diff(A.ptr) > 0))
        assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32)), "dot rows: the same bits on two calls"
        assert np.array_equal(g1.view(np.uint32), ga.view(np.uint32)), "dot rows: a batched set has the unbatched call's bits"
        assert np.any(g1 != 0.0)
    if case == "triangle":
        assert np.count_nonzero(refs[0][1] == 0) > 0, "mask entries no product reaches exist (exactly 0.0 above)"


# ------------------------------------------------------------------ 5. batched calls ---
@pytest.mark.parametrize("W", [2, 4])
def test_mixed_batched_remainder_shared_b_padded(tool, W):
    name, nb, pad = "bin_zoo", 5, 7
    A, B, Cp, Ci = bound_input(name)
    av, bv, refs = bound_reference(name, nb, shared_b=True)
    nC = len(Ci)
    plan = make_plan(tool, A, B, Cp, Ci, W)
    try:
        info = plan.info()
        assert info["width"] == W and nb % W != 0  # a remainder pass
        a_full = torch.full((nb, A.nnz + pad), float("nan"), dtype=torch.float32, device=f"cuda:{tool.device}")
        a_full[:, :A.nnz] = up32(tool, av)
        sentinel = np.float32(-12345.5)
        o_full = torch.full((nb, nC + pad), float(sentinel), dtype=torch.float32, device=f"cuda:{tool.device}")
        o_full[:, :nC] = float("nan")
        torch.cuda.synchronize()
        out = plan.run_batched(a_full[:, :A.nnz], up32(tool, bv[0]), out=o_full[:, :nC])  # B: one array for all sets
        torch.cuda.synchronize()
        assert out.data_ptr() == o_full.data_ptr()
        full = o_full.cpu().numpy()
    finally:
        plan.close()
    assert np.all(full[:, nC:].view(np.uint32) == sentinel.view(np.uint32)), "padding between the sets keeps its bytes"
    glob = global_entries(name, W, info)
    if W == 4:
        assert glob.any()
    for b in range(nb):
        assert_mixed(full[b, :nC].astype(np.float64), *refs[b], glob, f"{name} W={W} set {b}")


# ------------------------------------------------------------------ 6. non-finite values ---
@functools.lru_cache(maxsize=None)
def nonfinite_case():
    A, B, Cp, Ci = bound_input("tiny_zoo")
    av = inject_nonfinite(values32(A.nnz, 51), 61)
    bv = inject_nonfinite(values32(B.nnz, 52), 62)
    p, q, s = expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)
    return av, bv, nonfinite_reference(s, av[p], bv[q], len(Ci), U64)  # products classified in double; long-double sums


@pytest.mark.parametrize("W", [1, 4])
def test_mixed_nonfinite(tool, W):
    A, B, Cp, Ci = bound_input("tiny_zoo")
    av, bv, (want, ref, m, S, _) = nonfinite_case()
    assert all(np.count_nonzero(want == c) > 0 for c in range(4)), "every class of entry occurs"
    plan = make_plan(tool, A, B, Cp, Ci, W)
    try:
        info = plan.info()
        got = run_sets(tool, plan, av[None, :], bv[None, :], len(Ci))[0]
    finally:
        plan.close()
    assert info["rows"][GLOBAL] == 0
    have = classes_of(got)
    assert np.array_equal(have, want), f"{np.count_nonzero(have != want)} entries in another class than their products'"
    fin = want == FINITE
    assert_mixed(got[fin], ref, m, S, False, f"tiny_zoo with Inf, NaN and zeros, W={W}")


@pytest.mark.parametrize("form", [None, "dot"])
def test_mixed_float_overflowing_product_does_not_poison(tool, form):
    """3e38 * 2 and -3e38 * 2 overflow in float and are finite in double; with the third product, 2^50 * 2^50, every
    partial sum in any order is a multiple of 2^76 below 2^130: exact in double.  The entry is exactly 2^100 on a
    mixed plan and not finite on an FP32 plan, whose first product is already Inf."""
    big = float(np.float32(3e38))
    A = mhspgemm.CSR(1, 3, np.array([0, 3], np.int32), np.array([0, 1, 2], np.int32), np.array([big, -big, 2.0 ** 50]))
    B = mhspgemm.CSR(3, 1, np.array([0, 1, 2, 3], np.int32), np.zeros(3, np.int32), np.array([2.0, 2.0, 2.0 ** 50]))
    Cp, Ci = np.array([0, 1], np.int32), np.zeros(1, np.int32)
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(big) * np.float32(2.0)) and np.isfinite(big * 2.0)
    kw = {} if form is None else {"masked": True, "form": form}
    got = {}
    for accum in ("float64", None):
        plan = make_plan(tool, A, B, Cp, Ci, 1, accum=accum, **kw)
        try:
            info = plan.info()
            assert info["rows"][DOT if form else TEAM] == 1, info
            got[accum] = run_sets(tool, plan, A.val[None, :], B.val[None, :], 1)[0, 0]
        finally:
            plan.close()
    assert got["float64"] == 2.0 ** 100, got
    # (the FP32 plan: Inf - Inf = NaN where the products are rounded, +-Inf where a fused multiply-add keeps one exact)
    assert not np.isfinite(got[None]), got


# ------------------------------------------------------------------ 7. the backward ---
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
    return A, Cp, Ci, expand(A.ptr, A.col, A.ptr, A.col, Cp, Ci, A.N)


def grad_references(pqs, av, bv, G, nnzA, nnzB):
    p, q, _ = pqs
    wA, wB = ref_grad(pqs, av, bv, G, nnzA, nnzB)
    sA, sB = ref_grad(pqs, np.abs(av), np.abs(bv), np.abs(G), nnzA, nnzB)
    return (wA, np.bincount(p, minlength=nnzA), sA), (wB, np.bincount(q, minlength=nnzB), sB)


def test_mixed_backward_is_the_f32_backward(tool):
    A, Cp, Ci, pqs = square_case()
    av, bv, G = values32(A.nnz, 71), values32(A.nnz, 72), values32(len(Ci), 73)
    refA, refB = grad_references(pqs, av, bv, G, A.nnz, A.nnz)
    plan = make_plan(tool, A, A, Cp, Ci, 1)
    try:
        dG, dAv, dBv = up32(tool, G), up32(tool, av), up32(tool, bv)
        oA, oB = nan32(tool, A.nnz), nan32(tool, A.nnz)
        plan.grad(dG, dAv, dBv, out_A=oA, out_B=oB)
        a2, _ = plan.grad(dG, Bval=dBv, need_B=False, out_A=nan32(tool, A.nnz))
        torch.cuda.synchronize()
        gA, gB, gA2 = oA.cpu().numpy(), oB.cpu().numpy(), a2.cpu().numpy()
        # autograd: float32 leaves, float32 gradients
        a, b = dAv.clone().requires_grad_(True), dBv.clone().requires_grad_(True)
        out = plan.apply(a, b)
        out.backward(dG)
        torch.cuda.synchronize()
        assert out.dtype == torch.float32 and a.grad.dtype == torch.float32 and b.grad.dtype == torch.float32
        fwd, hA, hB = host(out.detach()), host(a.grad), host(b.grad)
    finally:
        plan.close()
    assert_f32_bound(gA.astype(np.float64), *refA, "dA")
    assert_f32_bound(gB.astype(np.float64), *refB, "dB")
    assert np.array_equal(gA.view(np.uint32), gA2.view(np.uint32)) and np.any(gA != 0), "dA: the same bits on two calls"
    assert_f32_bound(hA, *refA, "dA through apply")
    assert_f32_bound(hB, *refB, "dB through apply")
    assert_mixed(fwd, *exact_forward(A, A, Cp, Ci, av, bv), False, "apply's forward")


@pytest.mark.parametrize("W", [2, 4])
def test_mixed_backward_batched(tool, W):
    name, nb = "bin_zoo", W + 1
    A, B, Cp, Ci = bound_input(name)
    pqs = expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)
    av, bv, G = values32((nb, A.nnz), 81), values32((nb, B.nnz), 82), values32((nb, len(Ci)), 83)
    plan = make_plan(tool, A, B, Cp, Ci, W)
    try:
        oA, oB = nan32(tool, (nb, A.nnz)), nan32(tool, (nb, B.nnz))
        dG, dAv, dBv = up32(tool, G), up32(tool, av), up32(tool, bv)
        plan.grad_batched(dG, dAv, dBv, out_A=oA, out_B=oB)
        a2, _ = plan.grad_batched(dG, None, dBv, need_B=False, out_A=nan32(tool, (nb, A.nnz)))
        torch.cuda.synchronize()
        gA, gB, gA2 = oA.cpu().numpy(), oB.cpu().numpy(), a2.cpu().numpy()
    finally:
        plan.close()
    assert np.array_equal(gA.view(np.uint32), gA2.view(np.uint32)), "dA: the same bits on two calls"
    for b in range(nb):
        refA, refB = grad_references(pqs, av[b], bv[b], G[b], A.nnz, B.nnz)
        assert_f32_bound(gA[b].astype(np.float64), *refA, f"dA, W={W} set {b}")
        assert_f32_bound(gB[b].astype(np.float64), *refB, f"dB, W={W} set {b}")


@pytest.mark.parametrize("W", WIDTHS)
def test_mixed_backward_team_rows_at_the_cap(tool, W):
    """Team rows of 64 entries: at W = 4 the launch planned at sb = 32 is 73,728 B of dynamic LDS, which the float
    backward team kernel is registered for.  Integer values: both gradients compared exactly."""
    A, B, Cp, Ci, pqs = edge_rows_of(64, 100, 200)
    nb = W
    av = np.stack([edge_values(A.nnz, 150 + b) for b in range(nb)])
    bv = np.stack([edge_values(B.nnz, 180 + b) for b in range(nb)])
    G = np.stack([edge_values(len(Ci), 190 + b) for b in range(nb)])
    plan = make_plan(tool, A, B, Cp, Ci, W)
    try:
        info = plan.info()
        assert info["rows"][TEAM] == A.M, info
        oA, oB = nan32(tool, (nb, A.nnz)), nan32(tool, (nb, B.nnz))
        plan.grad_batched(up32(tool, G), up32(tool, av), up32(tool, bv), out_A=oA, out_B=oB)
        torch.cuda.synchronize()
        gA, gB = oA.cpu().numpy().astype(np.float64), oB.cpu().numpy().astype(np.float64)
    finally:
        plan.close()
    for b in range(nb):
        wA, wB = ref_grad(pqs, av[b], bv[b], G[b], A.nnz, B.nnz)
        assert np.array_equal(gA[b], wA) and np.array_equal(gB[b], wB), f"set {b}"


# ------------------------------------------------------------------ 8. refusals ---
def test_mixed_refusals(tool):
    A, Cp, Ci, _ = square_case()
    A.H2D(tool.device)
    C = device_csr(tool, A.M, A.N, Cp, Ci)
    L = _lib.lib()
    a, c = A.c_view(), C.c_view()

    def create(dtype, width, accum):
        out = ctypes.c_void_p()
        rc = L.mhs_values_plan_create_accum(tool.ctx, ctypes.byref(a), ctypes.byref(a), ctypes.byref(c), 0, 0, dtype, width,
                                            accum, ctypes.byref(out))
        return rc, out

    # accum that is no mhs_accum: refused with a message naming the argument, no plan
    for bad in (-1, 2):
        for dtype in (_lib.MHS_F32, _lib.MHS_F64):
            rc, out = create(dtype, 1, bad)
            assert rc == 3 and not out.value
            assert "accum" in L.mhs_last_error(tool.ctx).decode()
    rc, out = create(2, 1, _lib.MHS_ACC_F64)  # dtype 2 stays invalid: the sum type is no new dtype
    assert rc == 3 and not out.value and "dtype" in L.mhs_last_error(tool.ctx).decode()
    rc, out = create(_lib.MHS_F32, 3, _lib.MHS_ACC_F64)
    assert rc == 3 and not out.value and "width" in L.mhs_last_error(tool.ctx).decode()
    # the getter: (F64, ACC_F64) is the plain FP64 plan, (F32, NATIVE) the FP32 plan, (F32, ACC_F64) the mixed one
    plans = {}
    try:
        for key, dtype, accum, want in (("f64", _lib.MHS_F64, _lib.MHS_ACC_F64, _lib.MHS_ACC_NATIVE),
                                        ("f32", _lib.MHS_F32, _lib.MHS_ACC_NATIVE, _lib.MHS_ACC_NATIVE),
                                        ("mixed", _lib.MHS_F32, _lib.MHS_ACC_F64, _lib.MHS_ACC_F64)):
            rc, out = create(dtype, 1, accum)
            assert rc == 0 and out.value, L.mhs_last_error(tool.ctx).decode()
            plans[key] = out
            acc, dt = ctypes.c_int(-7), ctypes.c_int(-7)
            assert L.mhs_values_plan_accum(out, ctypes.byref(acc)) == 0 and acc.value == want
            assert L.mhs_values_plan_dtype(out, ctypes.byref(dt)) == 0 and dt.value == dtype
            assert L.mhs_values_plan_accum(out, None) == 3
        mixed = plans["mixed"]
        av, G = values32(A.nnz, 91), values32(len(Ci), 93)
        t32 = [up32(tool, v) for v in (av, av, G)]
        t64 = [up64(tool, v) for v in (av, av, G)]
        o64 = [torch.full((n,), float("nan"), dtype=torch.float64, device=f"cuda:{tool.device}") for n in (len(Ci), A.nnz, A.nnz)]
        o32 = [nan32(tool, n) for n in (len(Ci), A.nnz, A.nnz)]
        ties = torch.full((len(Ci),), -3, dtype=torch.int32, device=f"cuda:{tool.device}")
        torch.cuda.synchronize()
        a64, b64, g64 = (t.data_ptr() for t in t64)
        a32, b32, g32 = (t.data_ptr() for t in t32)
        c64, da64, db64 = (t.data_ptr() for t in o64)
        c32, da32, db32 = (t.data_ptr() for t in o32)
        ms = ctypes.c_double(-1.0)
        # a double hot call on a mixed plan: refused like on any FP32 plan, the message names the plan
        for call in (lambda: L.mhs_spgemm_values(tool.ctx, mixed, a64, b64, c64, ctypes.byref(ms)),
                     lambda: L.mhs_spgemm_values_batched(tool.ctx, mixed, 1, a64, 0, b64, 0, c64, 0, ctypes.byref(ms)),
                     lambda: L.mhs_spgemm_values_grad(tool.ctx, mixed, a64, b64, g64, da64, db64, ctypes.byref(ms)),
                     lambda: L.mhs_spgemm_values_grad_batched(tool.ctx, mixed, 1, a64, 0, b64, 0, g64, 0, da64, 0, db64, 0,
                                                              ctypes.byref(ms))):
            assert call() == 3
            msg = L.mhs_last_error(tool.ctx).decode()
            assert "FP32, FP64 sums" in msg and "the call's FP64" in msg, msg
            assert ms.value == -1.0
        # subgrad and witness keep refusing plus-times plans, mixed ones included
        assert L.mhs_spgemm_values_subgrad_f32(tool.ctx, mixed, a32, b32, c32, g32, ties.data_ptr(), da32, db32, ctypes.byref(ms)) == 3
        assert "plus_times" in L.mhs_last_error(tool.ctx).decode()
        assert L.mhs_spgemm_values_witness_f32(tool.ctx, mixed, a32, b32, c32, ties.data_ptr(), ctypes.byref(ms)) == 3
        assert "plus_times" in L.mhs_last_error(tool.ctx).decode()
        torch.cuda.synchronize()
        assert ms.value == -1.0 and torch.all(ties == -3).item()
        for o in o64 + o32:
            assert torch.isnan(o).all().item(), "a refused call writes nothing"
        # the mixed plan stays usable through the _f32 entry points; the FP64 plan made with ACC_F64 runs double calls
        assert L.mhs_spgemm_values_f32(tool.ctx, mixed, a32, b32, c32, None) == 0
        assert L.mhs_spgemm_values(tool.ctx, plans["f64"], a64, b64, c64, None) == 0
        torch.cuda.synchronize()
        assert not torch.isnan(o32[0]).any().item() and not torch.isnan(o64[0]).any().item()
        assert torch.all((o32[0].double() - o64[0]).abs() <= 1e-6 * o64[0].abs() + 1e-7).item()
    finally:
        for p in plans.values():
            L.mhs_values_plan_destroy(tool.ctx, p)
    # the wrapper: subgrad and witness on a mixed plan raise the library's refusal; a float64 tensor raises
    plan = mhspgemm.ValuesPlan(tool, A, A, C, dtype=torch.float32, accum=torch.float64)
    try:
        assert plan.info()["accum"] == "float64" and plan.accum == "float64"
        with pytest.raises(mhspgemm.MHSpGEMMError):
            plan.subgrad(t32[2], o32[0], t32[0], t32[1])
        with pytest.raises(mhspgemm.MHSpGEMMError):
            plan.witness(o32[0], t32[0], t32[1])
        with pytest.raises(ValueError, match="float32"):
            plan.run(t64[0], t64[1], out=o32[0])
    finally:
        plan.close()
