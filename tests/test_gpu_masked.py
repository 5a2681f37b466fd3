"""GPU tests of the masked product (mhspgemm.ValuesPlan(masked=True) over mhs_values_plan_create_masked):
C<M> = A*B on a given pattern, in the product form (walk the products, drop the misses) and the dot
form (per mask entry, A's row against B's column through B^T's pattern).  Expected values are the CPU
oracle's full product restricted to the mask with numpy; mask entries outside the product expect
exactly 0.0.  Tolerances are those of tests/test_gpu_values.py: 1e-6 relative / 1e-12 absolute and the
reference's 1e-9 rule; with mixed signs 1e-6 of the same product on absolute values.  Beside them every form
that check_forms runs is held to the FP64 rounding bound on the mask, 1.01 m 2^-53 S per entry (tests/_util.py)."""
import functools

import numpy as np
import pytest
import torch

import mhspgemm
from mhspgemm import _lib
from oracle import oracle as orc
from _util import (GOLDEN, PRODUCT_CASES, assert_f64_bound, assert_values, bin_zoo, csr_of, device_csr, exact_forward, filled,
                   keys, load_golden, new_values, random_csr, tiny_zoo, upload)

pytestmark = pytest.mark.gpu

TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL, DOT = 1, 2, 3, 4, 5, 6, 7


def on_mask(Cp, Ci, Cv, Mp, Mc, N):
    """The product (Cp, Ci, Cv) restricted to the mask (Mp, Mc): its values at the mask's entries, 0.0 where
    the product has none, and which mask entries the product reaches."""
    kC, kM = keys(Cp, Ci, N), keys(Mp, Mc, N)
    if len(kC) == 0:
        return np.zeros(len(kM)), np.zeros(len(kM), bool)
    pos = np.minimum(np.searchsorted(kC, kM), len(kC) - 1)
    hit = kC[pos] == kM
    return np.where(hit, Cv[pos], 0.0), hit


def kept_products(A, B, Mp, Mc):
    """Products of A*B that land in the mask: the product of the patterns with all values 1.0 counts them per entry."""
    Cp, Ci, Cn = orc.spgemm(A.ptr, A.col, np.ones(A.nnz), B.ptr, B.col, np.ones(B.nnz), B.N)
    n, _ = on_mask(Cp, Ci, Cn, Mp, Mc, B.N)
    return int(round(n.sum()))


def run_masked(tool, A, B, Mp, Mc, form, av=None, bv=None, calls=1):
    """A masked plan of A*B (both on the device) on the mask, `calls` calls into NaN-filled outputs.
    Returns (the values of each call, info())."""
    C = device_csr(tool, A.M, B.N, Mp, Mc)
    plan = mhspgemm.ValuesPlan(tool, A, B, C, masked=True, form=form)
    try:
        info = plan.info()
        dA = None if av is None else upload(tool, av)
        dB = None if bv is None else upload(tool, bv)
        got = []
        for _ in range(calls):
            out = filled(tool, C.nnz)
            plan.run(dA, dB, out=out)
            torch.cuda.synchronize()
            got.append(out.cpu().numpy())
    finally:
        plan.close()
    assert info["nnzC"] == len(Mc) and sum(info["rows"]) == A.M
    return got, info


def check_forms(tool, A, B, Mp, Mc, forms, seed=1, signed=False):
    """Both operands get new seeded values; every form in `forms` is compared with the oracle on the mask.
    Returns {form: info()}."""
    A.H2D(tool.device)
    if B is not A:
        B.H2D(tool.device)
    av, bv = new_values(A.nnz, seed, signed), new_values(B.nnz, seed + 1000, signed)
    Cp, Ci, Cv = orc.spgemm(A.ptr, A.col, av, B.ptr, B.col, bv, B.N)
    want, hit = on_mask(Cp, Ci, Cv, Mp, Mc, B.N)
    absv = None
    if signed:
        absv, _ = on_mask(*orc.spgemm(A.ptr, A.col, np.abs(av), B.ptr, B.col, np.abs(bv), B.N), Mp, Mc, B.N)
    kept, products = kept_products(A, B, Mp, Mc), orc.flop(A.col, B.ptr)
    exact = exact_forward(A, B, Mp, Mc, av, bv)  # the FP64 contract on the mask: 1.01 m 2^-53 S, m = 0 exactly 0.0
    assert np.array_equal(exact[1] > 0, hit) and exact[1].sum() == kept
    infos = {}
    for form in forms:
        (got,), info = run_masked(tool, A, B, Mp, Mc, form, av, bv)
        assert_values(Mp, Mc, want, Mp, Mc, got, absv)
        assert_f64_bound(got, *exact, f"masked plan, {form} form, C")
        assert np.all(got[~hit] == 0.0), "mask entries no product reaches are exactly 0.0"
        assert info["products"] == products and info["kept_products"] == kept, (form, info, kept)
        infos[form] = info
    return infos


# 1. mask = the product's own pattern: empty product, duplicates in A / B, rectangular, dense row and column, tile edges
@pytest.mark.parametrize("name", PRODUCT_CASES)
def test_masked_golden_products(tool, name):
    d, _, _, _ = load_golden(name)
    A = mhspgemm.CSR()
    assert mhspgemm.readMtxFile(A, str(GOLDEN / d["A"])) == 0
    B = A
    if d["B"]:
        B = mhspgemm.CSR()
        assert mhspgemm.readMtxFile(B, str(GOLDEN / d["B"])) == 0
    Cp, Ci, _ = orc.spgemm(A.ptr, A.col, A.val, B.ptr, B.col, B.val, B.N)
    infos = check_forms(tool, A, B, Cp, Ci, ("product", "dot"))
    for info in infos.values():
        assert info["kept_products"] == info["products"]
    assert infos["product"]["rows"][DOT] == 0
    assert infos["dot"]["rows"][DOT] == np.count_nonzero((np.diff(Cp) > 0) & (np.diff(A.ptr) > 0))


@functools.lru_cache(maxsize=None)
def rect_pair():
    """The operands of tests 2 and 4, and their product's pattern."""
    p, c, v = random_csr(1500, 1000, 7, 5)
    Bp, Bc, Bv = random_csr(1000, 20_000, 10, 6)
    Cp, Ci, _ = orc.spgemm(p, c, v, Bp, Bc, Bv, 20_000)
    return (p, c, v), (Bp, Bc, Bv), (Cp, Ci)


# 2. AUTO on a mask that contains the product (B's rows without duplicates): n * nA >= products, no dot row
def test_masked_auto_on_containing_mask_is_product_form(tool):
    (p, c, v), (Bp, Bc, Bv), (Cp, Ci) = rect_pair()
    A, B = device_csr(tool, 1500, 1000, p, c, v), device_csr(tool, 1000, 20_000, Bp, Bc, Bv)
    C = device_csr(tool, 1500, 20_000, Cp, Ci)
    plain = mhspgemm.ValuesPlan(tool, A, B, C)
    try:
        plain_info = plain.info()
    finally:
        plain.close()
    (got,), info = run_masked(tool, A, B, Cp, Ci, "auto")
    assert info["rows"] == plain_info["rows"] and info["rows"][DOT] == 0 and info["dot"] == 0
    assert info["plan_bytes"] == plain_info["plan_bytes"], "B^T is freed again when no row chose the dot class"
    assert plain_info["kept_products"] == plain_info["products"] == info["kept_products"]
    want, _ = on_mask(*orc.spgemm(p, c, v, Bp, Bc, Bv, B.N), Cp, Ci, B.N)
    assert_values(Cp, Ci, want, Cp, Ci, got)


# 3. triangle counting: L*L on L's pattern, all values 1.0 -- small integers, so exact
def test_masked_triangle_count_exact(tool):
    n = 2000
    rng = np.random.default_rng(5)
    pairs = rng.integers(0, n, (16_000, 2))
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    lower = np.unique(np.maximum(pairs[:, 0], pairs[:, 1]).astype(np.int64) * n + np.minimum(pairs[:, 0], pairs[:, 1]))
    r, c = lower // n, (lower % n).astype(np.int32)  # the strictly lower triangle of the symmetrised graph
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=ptr[1:])
    L = device_csr(tool, n, n, ptr.astype(np.int32), c, np.ones(len(c)))
    Cp, Ci, Cv = orc.spgemm(L.ptr, L.col, L.val, L.ptr, L.col, L.val, n)
    want, hit = on_mask(Cp, Ci, Cv, L.ptr, L.col, n)
    triangles = want.sum()
    assert triangles > 0 and hit.any() and not hit.all() and Cp[-1] > 50 * hit.sum(), "the case needs a thin mask"
    for form in ("product", "dot"):
        (got,), info = run_masked(tool, L, L, L.ptr, L.col, form)
        assert np.array_equal(got, want), form
        assert got.sum() == triangles and np.all(got[~hit] == 0.0)
        assert info["kept_products"] == int(triangles) and info["products"] == orc.flop(L.col, L.ptr)
        assert (info["rows"][DOT] > 0) == (form == "dot")


def thinned_mask_with_strangers(Cp, Ci, N, seed=77):
    """Every second entry of the pattern, every 50th row emptied, and per row up to 2 columns the pattern lacks."""
    M = len(Cp) - 1
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(Cp))
    keep = (np.arange(len(Ci)) % 2 == 0) & (rows % 50 != 0)
    rng = np.random.default_rng(seed)
    srow = np.repeat(np.arange(M, dtype=np.int64), 2)
    srow = srow[srow % 50 != 0]
    skey = srow * N + rng.integers(0, N, len(srow))
    skey = np.setdiff1d(skey, keys(Cp, Ci, N))  # strangers: not in the product
    key = np.union1d(rows[keep] * N + Ci[keep], skey)
    Mp = np.zeros(M + 1, np.int64)
    np.cumsum(np.bincount(key // N, minlength=M), out=Mp[1:])
    return Mp.astype(np.int32), (key % N).astype(np.int32), len(skey)


# 4. a thinned mask with strangers, both forms, mixed signs
def test_masked_thinned_with_strangers_signed(tool):
    (p, c, v), (Bp, Bc, Bv), (Cp, Ci) = rect_pair()
    A, B = mhspgemm.CSR(1500, 1000, p, c, v), mhspgemm.CSR(1000, 20_000, Bp, Bc, Bv)
    Mp, Mc, strangers = thinned_mask_with_strangers(Cp, Ci, B.N)
    assert strangers > 1000 and np.count_nonzero(np.diff(Mp) == 0) >= 30
    infos = check_forms(tool, A, B, Mp, Mc, ("product", "dot"), seed=7, signed=True)
    assert 0 < infos["dot"]["kept_products"] < infos["dot"]["products"]
    assert infos["dot"]["rows"][DOT] == np.count_nonzero((np.diff(Mp) > 0) & (np.diff(p) > 0))
    # the unmasked entry still wants containment
    with pytest.raises(mhspgemm.MHSpGEMMError) as e:
        mhspgemm.ValuesPlan(tool, A, B, device_csr(tool, A.M, B.N, Mp, Mc))
    assert e.value.status == 3 and "misses a column" in str(e.value), str(e.value)


def every_third(Cp, Ci, drop=False):
    """Per row every third entry kept, and always the row's first and last (spans stay); drop: every third
    entry removed instead."""
    M = len(Cp) - 1
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(Cp))
    at = np.arange(len(Ci)) - Cp[rows]
    third = at % 3 == 0
    keep = (~third if drop else third) | (at == 0) | (np.arange(len(Ci)) == Cp[rows + 1] - 1)
    Mp = np.zeros(M + 1, np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=M), out=Mp[1:])
    return Mp.astype(np.int32), Ci[keep]


# 5. every product-form class with misses: the zoos on their product's pattern thinned to every third entry.
# (Thinned to a third, the zoo's longest rows -- 20,000 and 21,120 entries -- fit a block's LDS and leave
# the global class empty, so bin_zoo also runs with every third entry removed: the contiguous row keeps
# 14,081 entries over 21,120 columns, past a workgroup's 160 KiB either way (n > 13,312, span > 19,968).
# Outputs start as NaN: the global class's zero fill shows here.)
def test_masked_every_product_class_with_misses(tool):
    rows = np.zeros(8, np.int64)
    for name, drop in (("bin_zoo", False), ("tiny_zoo", False), ("bin_zoo", True)):
        At, Bt = bin_zoo() if name == "bin_zoo" else tiny_zoo(7)
        A, B = csr_of(At), csr_of(Bt)
        Cp, Ci, _ = orc.spgemm(A.ptr, A.col, A.val, B.ptr, B.col, B.val, B.N)
        Mp, Mc = every_third(Cp, Ci, drop)
        info = check_forms(tool, A, B, Mp, Mc, ("product",), seed=3)["product"]
        assert info["kept_products"] < info["products"]
        if drop:
            assert info["rows"][GLOBAL] >= 1, info
        rows += info["rows"]
    for cls in (TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL):
        assert rows[cls] > 0, f"class {cls} has no rows"
    assert rows[DOT] == 0


@functools.lru_cache(maxsize=None)
def dot_edges():
    """B 600 x 3000: column 7 (the hub) in every row, columns 2990..2999 in none, 8 random others per row.
    A: 40 rows of 1, 63, 64, 65 or 200 entries, some reversed, some with a repeated entry.  Mask rows of
    1, 63, 64, 65 or 300 entries, the hub and the empty columns among them."""
    rng = np.random.default_rng(66)
    K, N, HUB = 600, 3000, 7
    brows = [np.union1d(rng.choice(np.setdiff1d(np.arange(2990), [HUB]), 8, replace=False), [HUB]) for _ in range(K)]
    Bp = np.zeros(K + 1, np.int64)
    Bp[1:] = np.cumsum([len(r) for r in brows])
    Bc = np.concatenate(brows).astype(np.int32)
    arows, mrows = [], []
    for i in range(40):
        na = (1, 63, 64, 65, 200)[i % 5]
        ks = np.sort(rng.choice(K, na, replace=False))
        if i % 3 == 1:
            ks = ks[::-1]                                  # unsorted A row
        if i % 4 == 2:
            ks = np.insert(ks, len(ks) // 2, ks[0])        # a repeated entry, not adjacent to its twin
        arows.append(ks)
        nm = (300, 1, 65, 64, 63)[i % 5]                   # (n, nA) pairs vary: 300 x 1, 1 x 63, 65 x 64, ...
        if i >= 20:
            nm = (1, 63, 64, 65, 300)[i % 5]               # ... and 1 x 1, 63 x 63, 64 x 64, 65 x 65, 300 x 200
        special = [HUB, 2990 + i % 10]
        if nm == 1:
            cols = np.array([special[i % 2]])              # only the hub, or only an empty column
        else:
            cols = np.union1d(rng.choice(np.setdiff1d(np.arange(2990), [HUB]), nm - 2, replace=False), special)
        mrows.append(np.sort(cols))
    Ap = np.zeros(41, np.int64)
    Ap[1:] = np.cumsum([len(r) for r in arows])
    Ac = np.concatenate(arows).astype(np.int32)
    Mp = np.zeros(41, np.int64)
    Mp[1:] = np.cumsum([len(r) for r in mrows])
    Mc = np.concatenate(mrows).astype(np.int32)
    return (40, K, Ap.astype(np.int32), Ac), (K, N, Bp.astype(np.int32), Bc), (Mp.astype(np.int32), Mc)


# 6. dot-class edges: n and nA at 1, 63, 64, 65 and past, a B^T row of 600, empty B^T rows, unsorted A, duplicates
def test_masked_dot_edges_bit_identical(tool):
    (M, K, Ap, Ac), (_, N, Bp, Bc), (Mp, Mc) = dot_edges()
    assert set(np.diff(Ap)) >= {1, 63, 64, 65, 200} and set(np.diff(Mp)) == {1, 63, 64, 65, 300}
    av, bv = new_values(len(Ac), 12, signed=True), new_values(len(Bc), 13, signed=True)
    A, B = device_csr(tool, M, K, Ap, Ac, av), device_csr(tool, K, N, Bp, Bc, bv)
    assert np.bincount(Bc, minlength=N)[7] == K and not np.isin(Bc, np.arange(2990, 3000)).any()
    want, hit = on_mask(*orc.spgemm(Ap, Ac, av, Bp, Bc, bv, N), Mp, Mc, N)
    absv, _ = on_mask(*orc.spgemm(Ap, Ac, np.abs(av), Bp, Bc, np.abs(bv), N), Mp, Mc, N)
    (g1, g2), info = run_masked(tool, A, B, Mp, Mc, "dot", calls=2)
    assert info["rows"][DOT] == M and info["plan_bytes"] >= 4 * (N + 1) + 8 * len(Bc)
    assert_values(Mp, Mc, want, Mp, Mc, g1, absv)
    assert np.all(g1[~hit] == 0.0) and (~hit).sum() >= 30
    assert np.array_equal(g1, g2), "a dot row's sum order is fixed: two calls give the same bits"
    assert info["kept_products"] == kept_products(A, B, Mp, Mc)


@functools.lru_cache(maxsize=None)
def hub_case():
    """B 64 x 4096 dense, A 512 x 64 with 8 distinct entries per row, a mask of 2 columns per row:
    32,768 products a row against a dot cost of 8 x 2 x (1 + ceil_log2(65)) = 128."""
    rng = np.random.default_rng(70)
    Bp = (np.arange(65) * 4096).astype(np.int32)
    Bc = np.tile(np.arange(4096, dtype=np.int32), 64)
    Bv = rng.uniform(0.1, 1.0, len(Bc))
    Ac = np.concatenate([np.sort(rng.choice(64, 8, replace=False)) for _ in range(512)]).astype(np.int32)
    Ap = (np.arange(513) * 8).astype(np.int32)
    Av = rng.uniform(0.1, 1.0, len(Ac))
    Mc = np.concatenate([np.sort(rng.choice(4096, 2, replace=False)) for _ in range(512)]).astype(np.int32)
    Mp = (np.arange(513) * 2).astype(np.int32)
    want, _ = on_mask(*orc.spgemm(Ap, Ac, Av, Bp, Bc, Bv, 4096), Mp, Mc, 4096)
    return (Ap, Ac, Av), (Bp, Bc, Bv), (Mp, Mc), want


# 7. AUTO picks the dot class where it must (a factor 256 between the forms; VAL_DOT_RATIO is at most 64)
def test_masked_auto_picks_dot(tool):
    (Ap, Ac, Av), (Bp, Bc, Bv), (Mp, Mc), want = hub_case()
    A, B = device_csr(tool, 512, 64, Ap, Ac, Av), device_csr(tool, 64, 4096, Bp, Bc, Bv)
    (ga,), auto = run_masked(tool, A, B, Mp, Mc, "auto")
    (gp,), prod = run_masked(tool, A, B, Mp, Mc, "product")
    assert auto["rows"][DOT] == 512 and auto["dot"] == 512 and prod["rows"][DOT] == 0
    assert auto["products"] == prod["products"] == 512 * 32768
    assert auto["kept_products"] == prod["kept_products"] == 512 * 8 * 2
    assert_values(Mp, Mc, want, Mp, Mc, ga)
    assert_values(Mp, Mc, want, Mp, Mc, gp)
    assert prod["plan_bytes"] + 8 * len(Bc) <= auto["plan_bytes"], "the product form keeps no B^T"


# 8. stream order (MHS_OPT_SYNC 0, torch's stream, a separate output), and B^T is not context workspace
def test_masked_stream_ordered_and_survives_trim(tool):
    (Ap, Ac, Av), (Bp, Bc, Bv), (Mp, Mc), want = hub_case()
    A, B = device_csr(tool, 512, 64, Ap, Ac, Av), device_csr(tool, 64, 4096, Bp, Bc, Bv)
    C = device_csr(tool, 512, 4096, Mp, Mc)
    q, d, w = random_csr(1200, 900, 6, 42)
    Yp, Yc, Yv = random_csr(900, 4000, 8, 43)
    X, Y = device_csr(tool, 1200, 900, q, d, w), device_csr(tool, 900, 4000, Yp, Yc, Yv)
    plan = mhspgemm.ValuesPlan(tool, A, B, C, masked=True, form="auto")
    try:
        assert plan.info()["rows"][DOT] == 512
        out = filled(tool, C.nnz)
        tool.set_option(_lib.MHS_OPT_SYNC, 0)
        tool.set_stream(torch.cuda.current_stream(tool.device).cuda_stream)
        try:
            assert plan.run(out=out) is None
            torch.cuda.synchronize()
            g1 = out.cpu().numpy()
        finally:
            tool.set_option(_lib.MHS_OPT_SYNC, 1)
            tool.set_stream(None)
        Z, _ = mhspgemm.spgemm(tool, X, Y, timing=False)  # an unrelated pair through the same context
        try:
            zp, zc, zv = Z.to_host()
        finally:
            Z.release()
        tool.release()  # mhs_ctx_trim: the workspace goes, the plan's B^T stays
        out2 = filled(tool, C.nnz)
        plan.run(out=out2)
        torch.cuda.synchronize()
        g2 = out2.cpu().numpy()
    finally:
        plan.close()
    assert_values(Mp, Mc, want, Mp, Mc, g1)
    assert_values(Mp, Mc, want, Mp, Mc, g2)
    assert np.array_equal(g1, g2)
    Zp, Zi, Zv = orc.spgemm(q, d, w, Yp, Yc, Yv, 4000)
    assert np.array_equal(zp, Zp) and np.array_equal(zc, Zi) and orc.compare_ref(Zp, Zi, Zv, zp, zc, zv) == 1


# 9. rejections at create; the context stays usable
def test_masked_rejections_at_create(tool):
    p, c, v = random_csr(400, 300, 6, 61)
    Bp, Bc, Bv = random_csr(300, 2000, 8, 62)
    A, B = device_csr(tool, 400, 300, p, c, v), device_csr(tool, 300, 2000, Bp, Bc, Bv)
    Cp, Ci, Cv = orc.spgemm(p, c, v, Bp, Bc, Bv, B.N)
    row = int(np.argmax(np.diff(Cp) >= 3))
    k = Cp[row] + 1
    col2 = Ci.copy()
    col2[[k, k + 1]] = col2[[k + 1, k]]  # two columns of one row swapped
    ptr3 = np.append(Cp, Cp[-1]).astype(np.int32)  # C.M != A.M
    for form in ("auto", "product", "dot"):
        with pytest.raises(mhspgemm.MHSpGEMMError) as e:
            mhspgemm.ValuesPlan(tool, A, B, device_csr(tool, A.M, B.N, Cp, col2), masked=True, form=form)
        assert e.value.status == 3 and "ascending" in str(e.value) and f"row {row}" in str(e.value), str(e.value)
        with pytest.raises(mhspgemm.MHSpGEMMError) as e:
            mhspgemm.ValuesPlan(tool, A, B, device_csr(tool, A.M + 1, B.N, ptr3, Ci), masked=True, form=form)
        assert e.value.status == 3 and "C.M != A.M" in str(e.value), str(e.value)
    with pytest.raises(mhspgemm.MHSpGEMMError) as e:
        mhspgemm.ValuesPlan(tool, A, B, device_csr(tool, A.M, B.N, Cp, Ci), masked=True, form=7)
    assert e.value.status == 3
    (got,), _ = run_masked(tool, A, B, Cp, Ci, "dot")  # the context is still usable
    assert_values(Cp, Ci, Cv, Cp, Ci, got)
