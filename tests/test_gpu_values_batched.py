"""GPU tests of the batched values calls (mhspgemm.ValuesPlan(..., width=W).run_batched over
mhs_values_plan_create_batched and mhs_spgemm_values_batched / _f32): W value sets in one walk of the patterns.

Every set has the contract of the unbatched call, and the references are per set.  FP64 plans: the long-double sums
of tests/_util.py and assert_f64_bound, |got - ref| <= 1.01 m 2^-53 S for an entry of m kept products with absolute
sum S.  FP32 plans: the contract of tests/test_gpu_values_f32.py restated here on float32-rounded inputs,
|got - ref| <= 1.01 m 2^-24 S against the FP64 sum (u = 2^-24, m < 2^16: gamma_m S of a float sum of m rounded
products; the reference's own error, m 2^-53 S, is 2^-29 of it).  Inputs have magnitude in [0.1, 1): nothing is
subnormal.  Entries with m = 0 must be exactly 0; every output starts NaN-filled and no NaN may remain.  Rows on the
class edges carry integer values of +-{1, 2, 3}, exact in either type in any order while 9 * products < 2^24, and
are compared with np.array_equal.  Nothing here is a measured tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mhspgemm
from mhspgemm import _lib, synth
from oracle import oracle as orc
from _util import (GOLDEN, PRODUCT_CASES, assert_f64_bound, bin_zoo, csr_of, device_csr, edge_val, edge_values, expand,
                   load_golden, new_values, seg_sum_ld, tiny_zoo)

pytestmark = pytest.mark.gpu

TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL, DOT = 1, 2, 3, 4, 5, 6, 7
U32 = 2.0 ** -24
WIDE = 1_000_000  # a column span no direct class holds
TYPES = {"f64": (torch.float64, np.float64, 8), "f32": (torch.float32, np.float32, 4)}
PLANS = [("f64", 2), ("f64", 4), ("f32", 2), ("f32", 4)]
plans = pytest.mark.parametrize("dt,W", PLANS, ids=[f"{d}-w{w}" for d, w in PLANS])
# the class table as a function of the sum bytes sb = W x value size: wave-direct span, wave-search n, block-direct
# span, block-search n (sb 4 and 8: the FP32 and FP64 tables of the unbatched plans)
CAPS = {4: (2048, 1024, 39936, 19968), 8: (1024, 682, 19968, 13312), 16: (512, 408, 9984, 7986), 32: (256, 226, 4992, 4436)}


def val_class(n, span, products, sb):
    """The class of a row at sum bytes sb (csrc/mhs_valplan.hpp's val_class on the table above)."""
    wd, ws, bd, bs = CAPS[sb]
    if n <= 64 and products <= 512:
        return TEAM
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


# ------------------------------------------------------------------ values, uploads, references ---
def rounded(v, dt):
    """The values as the plan's type holds them, as the float64 array the references compute on."""
    return np.asarray(v, TYPES[dt][1]).astype(np.float64)


def set_values(n, nb, seed, dt):
    """nb value sets of n entries, different per set: magnitudes in [0.1, 1), mixed signs, rounded to the type."""
    return np.stack([rounded(new_values(n, seed + 17 * b, signed=True), dt) for b in range(nb)]) if nb else np.zeros((0, n))


def up(tool, v, dt):
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=TYPES[dt][1])).to(f"cuda:{tool.device}")
    torch.cuda.synchronize()
    return t


def nans(tool, shape, dt):
    out = torch.full(shape, float("nan"), dtype=TYPES[dt][0], device=f"cuda:{tool.device}")
    torch.cuda.synchronize()
    return out


def reference(pqs, nC, av, bv, dt):
    """(ref, m, S) of one set over the kept products pqs: long double for FP64 plans, float64 for FP32 ones."""
    p, q, s = pqs
    m = np.bincount(s, minlength=nC).astype(np.int64)
    if dt == "f64":
        w = np.asarray(av[p], np.longdouble) * np.asarray(bv[q], np.longdouble)
        return seg_sum_ld(s, w, nC), m, seg_sum_ld(s, np.abs(w), nC)
    w = av[p] * bv[q]
    return np.bincount(s, w, nC), m, np.bincount(s, np.abs(w), nC)


def assert_set(got, ref, dt, what):
    """One set's values (host array of the plan's type) against its reference within the type's bound."""
    wref, m, S = ref
    assert got.dtype == TYPES[dt][1]
    if dt == "f64":
        return assert_f64_bound(got, wref, m, S, what)
    got = got.astype(np.float64)
    assert got.shape == wref.shape and not np.isnan(got).any(), f"{what}: every entry is written"
    assert m.max(initial=0) < 2 ** 16
    assert np.all(got[m == 0] == 0.0), f"{what}: entries no kept product reaches are exactly 0.0"
    err, bound = np.abs(got - wref), 1.01 * m * U32 * S
    bad = err > bound
    worst = float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0), initial=0.0))
    print(f"f32 bound, {what}: worst err / bound {worst:.3f} over {len(got)} entries, max m {m.max(initial=0)}")
    assert not bad.any(), f"{what}: {bad.sum()} of {len(got)} entries outside 1.01 m 2^-24 S (worst err / bound {worst:.3e})"
    return worst


def pattern_of(A, B):
    Cp, Ci, _ = orc.spgemm(A.ptr, A.col, np.ones(A.nnz), B.ptr, B.col, np.ones(B.nnz), B.N)
    return Cp, Ci


def make_plan(tool, A, B, Cp, Ci, dt, W, **kw):
    A.H2D(tool.device)
    if B is not A:
        B.H2D(tool.device)
    C = device_csr(tool, A.M, B.N, Cp, Ci)
    return mhspgemm.ValuesPlan(tool, A, B, C, dtype=TYPES[dt][0], width=W, **kw)


# ------------------------------------------------------------------ 1. every class, every set ---
NB1 = 5  # W = 2: two full passes and a tail of 1; W = 4: one full pass and a tail of 1
INPUTS = ["bin_zoo", "tiny_zoo", "global_rows"] + PRODUCT_CASES


@functools.lru_cache(maxsize=None)
def product_input(name):
    if name == "bin_zoo":
        A, B = (csr_of(t) for t in bin_zoo())
    elif name == "tiny_zoo":
        A, B = (csr_of(t) for t in tiny_zoo(7))
    elif name == "global_rows":  # past the block-search cap of every batched plan (sb >= 8: n > 13,312)
        A, B = (csr_of(t) for t in edge_val(13313, WIDE, 13400, copies=2))
    else:
        d, _, _, _ = load_golden(name)
        A = mhspgemm.CSR()
        assert mhspgemm.readMtxFile(A, str(GOLDEN / d["A"])) == 0
        B = A
        if d["B"]:
            B = mhspgemm.CSR()
            assert mhspgemm.readMtxFile(B, str(GOLDEN / d["B"])) == 0
    Cp, Ci = pattern_of(A, B)
    return A, B, Cp, Ci, expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)


@functools.lru_cache(maxsize=None)
def product_sets(name, dt):
    """The NB1 value sets of an input and each set's reference: shared by the widths, never changed."""
    A, B, Cp, Ci, pqs = product_input(name)
    av, bv = set_values(A.nnz, NB1, 100, dt), set_values(B.nnz, NB1, 900, dt)
    return av, bv, [reference(pqs, len(Ci), av[b], bv[b], dt) for b in range(NB1)]


_INFO = {}


def run_every_set(tool, name, dt, W, between=None):
    """The NB1 sets of an input through a plan of (dt, W) made on `tool`, every set against its reference.  Returns
    info().  between: called after the batched call (other work on the plan's context); the call then runs again,
    into NaNs again, and is held to the references like the first."""
    A, B, Cp, Ci, _ = product_input(name)
    av, bv, refs = product_sets(name, dt)
    plan = make_plan(tool, A, B, Cp, Ci, dt, W)
    try:
        info = plan.info()
        assert info["width"] == W and plan.width == W and info["dtype"] == ("float64" if dt == "f64" else "float32")
        out = nans(tool, (NB1, len(Ci)), dt)
        dav, dbv = up(tool, av, dt), up(tool, bv, dt)
        assert plan.run_batched(dav, dbv, out=out) is out
        torch.cuda.synchronize()
        got = [out.cpu().numpy()]
        if between is not None:
            between()
            out.fill_(float("nan"))
            assert plan.run_batched(dav, dbv, out=out) is out
            torch.cuda.synchronize()
            got.append(out.cpu().numpy())
            assert plan.info() == info, "the plan after other work on its context"
    finally:
        plan.close()
    for k, g in enumerate(got):
        for b in range(NB1):
            assert_set(g[b], refs[b], dt, f"{name} {dt} W={W} set {b}" + ", after other work on the context" * k)
    return info


def every_set(tool, name, dt, W):
    if (name, dt, W) not in _INFO:
        _INFO[name, dt, W] = run_every_set(tool, name, dt, W)
    return _INFO[name, dt, W]


@plans
@pytest.mark.parametrize("name", INPUTS)
def test_batched_every_class_every_set(tool, name, dt, W):
    info = every_set(tool, name, dt, W)
    if name == "global_rows":
        assert info["rows"][GLOBAL] == 2, info
    if name == "tiny_zoo":
        assert info["rows"][TEAM] > 0.5 * sum(info["rows"])


@plans
def test_batched_every_class_has_rows(tool, dt, W):
    rows = np.sum([every_set(tool, name, dt, W)["rows"] for name in INPUTS], axis=0)
    for cls in (TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL):
        assert rows[cls] > 0, f"class {cls} has no rows at {dt} W={W}"
    assert rows[DOT] == 0


# ------------------------------------------------------------------ 2. sets do not mix; strides ---
@functools.lru_cache(maxsize=None)
def square_case():
    rng = np.random.default_rng(21)
    M = 300
    lens = rng.poisson(6, M)
    key = np.unique(np.repeat(np.arange(M, dtype=np.int64), lens) * M + rng.integers(0, M, lens.sum()))
    ptr = np.zeros(M + 1, np.int64)
    np.cumsum(np.bincount(key // M, minlength=M), out=ptr[1:])
    A = mhspgemm.CSR(M, M, ptr.astype(np.int32), (key % M).astype(np.int32), np.ones(len(key)))
    Cp, Ci = pattern_of(A, A)
    return A, Cp, Ci, expand(A.ptr, A.col, A.ptr, A.col, Cp, Ci, A.N)


PAD = 7


@plans
def test_batched_sets_do_not_mix_and_strides(tool, dt, W):
    A, Cp, Ci, pqs = square_case()
    nnz, nC, most = A.nnz, len(Ci), 2 * W + 1
    av, bv = set_values(nnz, most, 300, dt), set_values(nnz, most, 700, dt)
    dA, dB = up(tool, av, dt), up(tool, bv, dt)
    padA = nans(tool, (most, nnz + 5), dt)  # a 2-D input with a padded row stride: NaN between the sets
    padA[:, :nnz] = dA
    torch.cuda.synchronize()
    refs, alone = {}, {}
    plan, plan1 = make_plan(tool, A, A, Cp, Ci, dt, W), make_plan(tool, A, A, Cp, Ci, dt, 1)
    try:
        def one(ia, ib):  # the reference of set (ia, ib), and the set computed alone on the width-1 plan
            if (ia, ib) not in refs:
                refs[ia, ib] = reference(pqs, nC, av[ia], bv[ib], dt)
                o = nans(tool, (nC,), dt)
                plan1.run(dA[ia], dB[ib], out=o)
                torch.cuda.synchronize()
                alone[ia, ib] = o.cpu().numpy()
            return refs[ia, ib], alone[ia, ib]

        for nb in sorted({1, W - 1, W, W + 1, 2 * W + 1}):
            modes = {"A shared": (dA[0], dB[:nb], lambda b: (0, b)), "B shared": (dA[:nb], dB[0], lambda b: (b, 0)),
                     "both 2-D": (dA[:nb], dB[:nb], lambda b: (b, b)), "A padded": (padA[:nb, :nnz], dB[:nb], lambda b: (b, b))}
            for mode, (ta, tb, pick) in modes.items():
                if mode == "A padded" and nb > 1:
                    assert ta.stride(0) == nnz + 5
                full = nans(tool, (nb, nC + PAD), dt)
                out = full[:, :nC]  # strideC = nnzC + 7
                assert plan.run_batched(ta, tb, out=out) is out
                torch.cuda.synchronize()
                got = full.cpu().numpy()
                assert np.isnan(got[:, nC:]).all(), f"{mode} nb={nb}: the padding between the sets is not written"
                for b in range(nb):
                    ref, single = one(*pick(b))
                    what = f"{mode} nb={nb} set {b}"
                    assert_set(got[b, :nC], ref, dt, what)
                    # both are within the bound of the exact sum: they differ by at most twice the bound
                    _, m, S = ref
                    u = 2.0 ** -53 if dt == "f64" else U32
                    diff = np.abs(got[b, :nC].astype(np.float64) - single.astype(np.float64))
                    assert np.all(diff <= 2 * 1.01 * m * u * np.asarray(S, np.float64)), f"{what}: against the set run alone"
        assert torch.isnan(padA[:, nnz:]).all().item()
        # an output allocated by the call: [nb, nnzC] of the plan's type
        fresh = plan.run_batched(dA[:3], dB[0])
        torch.cuda.synchronize()
        assert fresh.shape == (3, nC) and fresh.dtype == TYPES[dt][0]
        assert_set(fresh[2].cpu().numpy(), one(2, 0)[0], dt, "allocated out, set 2")
    finally:
        plan.close()
        plan1.close()


# ------------------------------------------------------------------ 3. class edges, exact ---
# (at, above): edge_val's (n, span, products); then the classes of the two sides at this sum-byte size
BYTE_EDGES = {
    16: {"wave_direct_span": ((200, 512, 1000), (200, 513, 1000), (WAVE_DIRECT, BLOCK_DIRECT)),
         "wave_search_n": ((408, WIDE, 2000), (409, WIDE, 2000), (WAVE_SEARCH, BLOCK_SEARCH)),
         "block_direct_span": ((3000, 9984, 4000), (3000, 9985, 4000), (BLOCK_DIRECT, BLOCK_SEARCH)),
         "block_search_n": ((7986, WIDE, 8000), (7987, WIDE, 8000), (BLOCK_SEARCH, GLOBAL))},
    32: {"wave_direct_span": ((200, 256, 1000), (200, 257, 1000), (WAVE_DIRECT, BLOCK_DIRECT)),
         "wave_search_n": ((226, WIDE, 2000), (227, WIDE, 2000), (WAVE_SEARCH, BLOCK_SEARCH)),
         "block_direct_span": ((3000, 4992, 4000), (3000, 4993, 4000), (BLOCK_DIRECT, BLOCK_SEARCH)),
         "block_search_n": ((4436, WIDE, 4500), (4437, WIDE, 4500), (BLOCK_SEARCH, GLOBAL))},
    8: {"wave_direct_span": ((200, 1024, 1000), (200, 1025, 1000), (WAVE_DIRECT, BLOCK_DIRECT)),  # FP32 W=2: the FP64 edges
        "wave_search_n": ((682, WIDE, 2000), (683, WIDE, 2000), (WAVE_SEARCH, BLOCK_SEARCH)),
        "block_direct_span": ((3000, 19968, 4000), (3000, 19969, 4000), (BLOCK_DIRECT, BLOCK_SEARCH)),
        "block_search_n": ((13312, WIDE, 13400), (13313, WIDE, 13400), (BLOCK_SEARCH, GLOBAL))},
}
TEAM_EDGES = {"team_n": ((64, 100, 200), (65, 100, 200), (TEAM, WAVE_DIRECT)),
              "team_products": ((10, 50, 512), (10, 50, 513), (TEAM, WAVE_DIRECT))}
EDGE_NAMES = list(BYTE_EDGES[16]) + list(TEAM_EDGES)


@functools.lru_cache(maxsize=None)
def edge_rows_of(n, span, products):
    assert 9 * products < 2 ** 24
    A, B = (csr_of(t) for t in edge_val(n, span, products))
    Cp, Ci = pattern_of(A, B)
    return A, B, Cp, Ci, expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)


@plans
@pytest.mark.parametrize("side", [0, 1], ids=["at", "above"])
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_batched_class_edges_exact(tool, name, side, dt, W):
    vb = TYPES[dt][2]
    sb = W * vb
    edge = TEAM_EDGES[name] if name in TEAM_EDGES else BYTE_EDGES[sb][name]
    n, span, products = edge[side]
    A, B, Cp, Ci, (p, q, s) = edge_rows_of(n, span, products)
    nb = W + 1
    av = np.stack([edge_values(A.nnz, 50 + b) for b in range(nb)])  # integers of +-{1, 2, 3}, different per set
    bv = np.stack([edge_values(B.nnz, 80 + b) for b in range(nb)])
    got = None
    for width in (W, 1):
        plan = make_plan(tool, A, B, Cp, Ci, dt, width)
        try:
            info = plan.info()
            classes = [c for c in range(8) if info["rows"][c]]
            assert info["width"] == width and sum(info["rows"]) == A.M and len(classes) == 1, info
            if width == W:
                assert classes == [edge[2][side]], (classes, info)
                assert classes == [val_class(n, span, products, sb)]
                out = nans(tool, (nb, len(Ci)), dt)
                plan.run_batched(up(tool, av, dt), up(tool, bv, dt), out=out)
                torch.cuda.synchronize()
                got = out.cpu().numpy()
            else:
                assert classes == [val_class(n, span, products, vb)], (classes, info)
        finally:
            plan.close()
    for b in range(nb):
        want = np.bincount(s, av[b][p] * bv[b][q], len(Ci))  # integers: exact in float64, and below 2^24
        assert np.array_equal(got[b].astype(np.float64), want), f"set {b}"


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
def rect_mask_case():
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
def mask_input(case):
    A, B, Mp, Mc = triangle_case() if case == "triangle" else rect_mask_case()
    return A, B, Mp, Mc, expand(A.ptr, A.col, B.ptr, B.col, Mp, Mc, B.N)


@functools.lru_cache(maxsize=None)
def mask_sets(case, dt, nb):
    A, B, Mp, Mc, pqs = mask_input(case)
    av, bv = set_values(A.nnz, nb, 400, dt), set_values(B.nnz, nb, 500, dt)
    return av, bv, [reference(pqs, len(Mc), av[b], bv[b], dt) for b in range(nb)]


@plans
@pytest.mark.parametrize("form", ["product", "dot", "auto"])
@pytest.mark.parametrize("case", ["triangle", "rect"])
def test_batched_masked_forms(tool, case, form, dt, W):
    A, B, Mp, Mc, (p, q, s) = mask_input(case)
    nb = W + 1
    av, bv, refs = mask_sets(case, dt, nb)
    dA, dB = up(tool, av, dt), up(tool, bv, dt)
    plan, plan1 = make_plan(tool, A, B, Mp, Mc, dt, W, masked=True, form=form), None
    try:
        info = plan.info()
        plan1 = make_plan(tool, A, B, Mp, Mc, dt, 1, masked=True, form=form)
        assert info["kept_products"] == plan1.info()["kept_products"] == len(p)
        assert 0 < info["kept_products"] < info["products"], "the case needs products outside the mask"
        if form != "auto":
            assert (info["dot"] > 0) == (form == "dot"), (form, info)
        out, again = nans(tool, (nb, len(Mc)), dt), nans(tool, (nb, len(Mc)), dt)
        plan.run_batched(dA, dB, out=out)
        plan.run_batched(dA, dB, out=again)
        torch.cuda.synchronize()
        got, got2 = out.cpu().numpy(), again.cpu().numpy()
        for b in range(nb):
            assert_set(got[b], refs[b], dt, f"{case} {form} set {b}")  # (m counts kept products only)
        if form == "dot":  # the dot rows' fixed order: the unbatched DOT call's bits, and the same on every call
            assert info["dot"] == plan1.info()["dot"] and sum(info["rows"][1:7]) == 0
            bits = np.uint64 if dt == "f64" else np.uint32
            assert np.array_equal(got.view(bits), got2.view(bits)), "two batched calls, the same bits"
            for b in range(nb):
                o = nans(tool, (len(Mc),), dt)
                plan1.run(dA[b], dB[b], out=o)
                torch.cuda.synchronize()
                assert np.array_equal(o.cpu().numpy().view(bits), got[b].view(bits)), f"set {b}: the unbatched DOT call's bits"
        if case == "triangle":  # mask entries no product reaches exist (exactly 0: assert_set's m = 0)
            assert np.count_nonzero(np.bincount(s, minlength=len(Mc)) == 0) > 0
    finally:
        plan.close()
        if plan1 is not None:
            plan1.close()


# ------------------------------------------------------------------ 5. stream and sync contract ---
def busy(x, rounds=150):
    for _ in range(rounds):
        x.mul_(1.0000001)


@plans
@pytest.mark.parametrize("where", ["side", "default"])
def test_batched_stream_ordered(tool, where, dt, W):
    """MHS_OPT_SYNC 0: the inputs hold NaN until copies queued behind a long torch kernel on the same stream fill
    them; the batched call is queued after them and only that stream is synchronised."""
    A, Cp, Ci, pqs = square_case()
    nb = W + 1
    av, bv = set_values(A.nnz, nb, 300, dt), set_values(A.nnz, nb, 700, dt)
    srcA, srcB = up(tool, av, dt), up(tool, bv, dt)
    dA, dB, out = nans(tool, (nb, A.nnz), dt), nans(tool, (nb, A.nnz), dt), nans(tool, (nb, len(Ci)), dt)
    plan = make_plan(tool, A, A, Cp, Ci, dt, W)
    ballast = torch.ones(1 << 24, dtype=torch.float64, device=f"cuda:{tool.device}")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(tool.device) if where == "side" else torch.cuda.default_stream(tool.device)
    tool.set_option(_lib.MHS_OPT_SYNC, 0)
    try:
        with torch.cuda.stream(stream):
            assert (torch.cuda.current_stream(tool.device).cuda_stream != 0) == (where == "side")
            busy(ballast)
            dA.copy_(srcA, non_blocking=True)
            dB.copy_(srcB, non_blocking=True)
            plan._ordered_on_current_stream(lambda: plan.run_batched(dA, dB, out=out))
            kept = out.clone()  # (queued behind the call on the same stream)
            stream.synchronize()
            got = kept.cpu().numpy()
            _, ms = plan._ordered_on_current_stream(lambda: plan.run_batched(dA, dB, out=out, timed=True))
            assert ms > 0.0
            stream.synchronize()
            timed = out.cpu().numpy()
    finally:
        tool.set_option(_lib.MHS_OPT_SYNC, 1)
        tool.set_stream(None)
        plan.close()
    for b in range(nb):
        ref = reference(pqs, len(Ci), av[b], bv[b], dt)
        assert_set(got[b], ref, dt, f"{where} stream, set {b}")
        assert_set(timed[b], ref, dt, f"{where} stream, timed call, set {b}")


# ------------------------------------------------------------------ 6. refusals with a context ---
def test_batched_refusals(tool):
    A, Cp, Ci, _ = square_case()
    A.H2D(tool.device)
    C = device_csr(tool, A.M, A.N, Cp, Ci)
    L = _lib.lib()
    a, c = A.c_view(), C.c_view()
    nnz, nC = A.nnz, len(Ci)

    def message():
        return L.mhs_last_error(tool.ctx).decode()

    for bad in (3, 8, 0, -2):  # plan creation: a width that is not 1, 2 or 4
        out = ctypes.c_void_p()
        assert L.mhs_values_plan_create_batched(tool.ctx, ctypes.byref(a), ctypes.byref(a), ctypes.byref(c), 0, 0, _lib.MHS_F64,
                                                bad, ctypes.byref(out)) == 3
        assert "width" in message() and not out.value
    p2 = mhspgemm.ValuesPlan(tool, A, A, C, width=2)
    p1 = None
    try:
        v64 = up(tool, set_values(nnz, 2, 1, "f64"), "f64")
        v32 = up(tool, set_values(nnz, 2, 1, "f32"), "f32")
        o64, o32 = nans(tool, (2, nC), "f64"), nans(tool, (2, nC), "f32")
        g64 = nans(tool, (2, nnz), "f64")
        ms = ctypes.c_double(-1.0)
        x, o, g = v64.data_ptr(), o64.data_ptr(), g64.data_ptr()
        batched, batched32 = L.mhs_spgemm_values_batched, L.mhs_spgemm_values_batched_f32
        calls = [
            (lambda: batched(tool.ctx, p2.plan, 0, x, nnz, x, nnz, o, nC, ctypes.byref(ms)), "nb"),
            (lambda: batched(tool.ctx, p2.plan, -1, x, nnz, x, nnz, o, nC, ctypes.byref(ms)), "nb"),
            (lambda: batched(tool.ctx, p2.plan, 2, x, nnz - 1, x, nnz, o, nC, ctypes.byref(ms)), "stride"),
            (lambda: batched(tool.ctx, p2.plan, 2, x, nnz, x, nnz - 1, o, nC, ctypes.byref(ms)), "stride"),
            (lambda: batched(tool.ctx, p2.plan, 2, x, -nnz, x, nnz, o, nC, ctypes.byref(ms)), "stride"),
            (lambda: batched(tool.ctx, p2.plan, 2, x, nnz, x, nnz, o, nC - 1, ctypes.byref(ms)), "strideC"),
            (lambda: batched(tool.ctx, p2.plan, 2, x, nnz, x, nnz, o, 0, ctypes.byref(ms)), "strideC"),
            (lambda: batched(tool.ctx, p2.plan, 2, None, nnz, x, nnz, o, nC, ctypes.byref(ms)), "null"),
            (lambda: batched(tool.ctx, p2.plan, 2, x, nnz, x, nnz, None, nC, ctypes.byref(ms)), "null"),
            (lambda: batched32(tool.ctx, p2.plan, 2, v32.data_ptr(), nnz, v32.data_ptr(), nnz, o32.data_ptr(), nC,
                               ctypes.byref(ms)), "FP32"),
            (lambda: L.mhs_spgemm_values_f32(tool.ctx, p2.plan, v32.data_ptr(), v32.data_ptr(), o32.data_ptr(),
                                             ctypes.byref(ms)), "FP64"),
            (lambda: L.mhs_spgemm_values_grad(tool.ctx, p2.plan, x, x, o, g, g + 8 * nnz, ctypes.byref(ms)), "width-1"),
        ]
        for call, cause in calls:
            assert call() == 3
            assert cause in message(), (cause, message())
            assert ms.value == -1.0
        assert "backward of batched plans is not built" in message()
        # the wrapper: grad and apply raise with the library's message
        for use in (lambda: p2.grad(o64[0], v64[0], v64[1]), lambda: p2.apply(v64[0], v64[1])):
            with pytest.raises(mhspgemm.MHSpGEMMError, match="backward of batched plans is not built") as e:
                use()
            assert e.value.status == 3
        torch.cuda.synchronize()
        for t in (o64, o32, g64):
            assert torch.isnan(t).all().item(), "a refused call writes nothing"
        # nb = 1 takes any strideC; the unbatched entry point runs on the width-2 plan
        assert batched(tool.ctx, p2.plan, 1, x, 0, x, 0, o, 0, None) == 0
        assert L.mhs_spgemm_values(tool.ctx, p2.plan, x, x, o + 8 * nC, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(o64[0], o64[1]) and not torch.isnan(o64).any().item()
        # a width-1 plan made through create_batched runs the backward as before
        out = ctypes.c_void_p()
        assert L.mhs_values_plan_create_batched(tool.ctx, ctypes.byref(a), ctypes.byref(a), ctypes.byref(c), 0, 0, _lib.MHS_F64,
                                                1, ctypes.byref(out)) == 0
        try:
            w = ctypes.c_int(-1)
            assert L.mhs_values_plan_width(out, ctypes.byref(w)) == 0 and w.value == 1
            assert L.mhs_values_plan_width(p2.plan, ctypes.byref(w)) == 0 and w.value == 2
            assert L.mhs_spgemm_values_grad(tool.ctx, out, x, x, o, g, g + 8 * nnz, None) == 0
            p1 = mhspgemm.ValuesPlan(tool, A, A, C)
            dA, dB = p1.grad(o64[0], v64[0], v64[0])
            torch.cuda.synchronize()
            assert torch.equal(dA, g64[0]), "dA has a fixed order: the bits of the plain plan's"
            assert torch.allclose(dB, g64[1], rtol=1e-10, atol=1e-10)  # (dB is summed by atomics, in any order)
        finally:
            L.mhs_values_plan_destroy(tool.ctx, out)
    finally:
        p2.close()
        if p1 is not None:
            p1.close()


# ------------------------------------------------------------------ 7. width 1 is today's plan ---
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_batched_width_1_is_todays_plan(tool, dt):
    A, B, Cp, Ci, _ = product_input("bin_zoo")
    av, bv, refs = product_sets("bin_zoo", dt)
    A.H2D(tool.device)
    B.H2D(tool.device)
    C = device_csr(tool, A.M, B.N, Cp, Ci)
    L = _lib.lib()
    a, b, c = A.c_view(), B.c_view(), C.c_view()
    typed = mhspgemm.ValuesPlan(tool, A, B, C, dtype=TYPES[dt][0])  # (mhs_values_plan_create / _typed)
    raw = ctypes.c_void_p()
    code = _lib.MHS_F64 if dt == "f64" else _lib.MHS_F32
    assert L.mhs_values_plan_create_batched(tool.ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), 0, 0, code, 1,
                                            ctypes.byref(raw)) == 0
    try:
        i1, i2 = _lib.mhs_values_info(), _lib.mhs_values_info()
        assert L.mhs_values_plan_info(raw, ctypes.byref(i1)) == 0 and L.mhs_values_plan_info(typed.plan, ctypes.byref(i2)) == 0
        assert list(i1.rows) == list(i2.rows) and (i1.products, i1.nnzC, i1.plan_bytes) == (i2.products, i2.nnzC, i2.plan_bytes)
        assert typed.info()["width"] == 1
        out = nans(tool, (NB1, len(Ci)), dt)
        assert typed.run_batched(up(tool, av, dt), up(tool, bv, dt), out=out) is out  # NB1 runs of the unbatched kernels
        torch.cuda.synchronize()
        got = out.cpu().numpy()
    finally:
        L.mhs_values_plan_destroy(tool.ctx, raw)
        typed.close()
    for s in range(NB1):
        assert_set(got[s], refs[s], dt, f"width 1, {dt}, set {s}")
