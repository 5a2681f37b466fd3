"""GPU tests of the values-only SpGEMM (mhspgemm.ValuesPlan over mhs_values_plan_create /
mhs_spgemm_values): C's values recomputed on a kept pattern, against the oracle on the new
operands.  Pattern equal by construction (it is C's own); values within the project's two
tolerances (tests/test_gpu_parity.py): 1e-6 relative / 1e-12 absolute, and the reference's 1e-9
rule.  With mixed signs the bound is 1e-6 of the same product on absolute values.  Beside them every values
call of the shared checker is held to the FP64 rounding bound, 1.01 m 2^-53 S per entry (tests/_util.py)."""
import functools

import numpy as np
import pytest
import torch

import mhspgemm
from mhspgemm import _lib, synth
from oracle import oracle as orc
from _util import (GOLDEN, PRODUCT_CASES, assert_f64_bound, assert_values, bin_zoo, csr_of, exact_forward, load_golden,
                   new_values, random_csr, tiny_zoo, upload)

pytestmark = pytest.mark.gpu

TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL = 1, 2, 3, 4, 5, 6


def product(tool, A, B):
    """C of mhspgemm.spgemm on device-resident A, B (uploaded here)."""
    A.H2D(tool.device)
    if B is not A:
        B.H2D(tool.device)
    C, _ = mhspgemm.spgemm(tool, A, B, timing=False)
    return C


def values_check(tool, A, B, seed=1, signed=False):
    """The shared checker: pattern from the full product, new seeded values, one values call,
    compared with the oracle on the new operands.  Returns the plan's info()."""
    C = product(tool, A, B)
    try:
        plan = mhspgemm.ValuesPlan(tool, A, B, C)
        try:
            info = plan.info()
            av, bv = new_values(A.nnz, seed, signed), new_values(B.nnz, seed + 1000, signed)
            dA, dB = upload(tool, av), upload(tool, bv)
            plan.run(dA, dB)
            p, c, v = C.to_host()
        finally:
            plan.close()
    finally:
        C.release()
    Cp, Ci, Cv = orc.spgemm(A.ptr, A.col, av, B.ptr, B.col, bv, B.N)
    absv = None
    if signed:
        _, _, absv = orc.spgemm(A.ptr, A.col, np.abs(av), B.ptr, B.col, np.abs(bv), B.N)
    assert_values(Cp, Ci, Cv, p, c, v, absv)
    assert_f64_bound(v, *exact_forward(A, B, Cp, Ci, av, bv), "values plan, C")  # the FP64 contract: 1.01 m 2^-53 S
    assert info["nnzC"] == Cp[-1] and info["products"] == orc.flop(A.col, B.ptr)
    assert sum(info["rows"]) == A.M and info["plan_bytes"] >= 4 * A.M
    return info


# 1. golden products: empty product, duplicates in A / B, rectangular, dense row and column, tile edges
@pytest.mark.parametrize("name", PRODUCT_CASES)
def test_values_golden_products(tool, name):
    d, _, _, _ = load_golden(name)
    A = mhspgemm.CSR()
    assert mhspgemm.readMtxFile(A, str(GOLDEN / d["A"])) == 0
    B = A
    if d["B"]:
        B = mhspgemm.CSR()
        assert mhspgemm.readMtxFile(B, str(GOLDEN / d["B"])) == 0
    values_check(tool, A, B)


# 2., 3. the zoos: every class between them
_ZOO_INFO = {}


def zoo_info(tool, name):
    if name not in _ZOO_INFO:
        At, Bt = bin_zoo() if name == "bin_zoo" else tiny_zoo(7)
        _ZOO_INFO[name] = values_check(tool, csr_of(At), csr_of(Bt), seed=3)
    return _ZOO_INFO[name]


def test_values_bin_zoo(tool):
    info = zoo_info(tool, "bin_zoo")
    # the 20,000-entry scattered rows (12 B an entry searched) and the 21,120-column contiguous row
    # (8 B a column direct) are past one workgroup's 160 KiB
    assert info["rows"][GLOBAL] >= 3
    assert info["rows"][BLOCK_DIRECT] > 0  # the 3000-duplicate row among them


def test_values_tiny_zoo(tool):
    info = zoo_info(tool, "tiny_zoo")
    assert info["rows"][TEAM] > 0.5 * sum(info["rows"])


def test_values_every_class_has_rows(tool):
    rows = np.add(zoo_info(tool, "bin_zoo")["rows"], zoo_info(tool, "tiny_zoo")["rows"])
    for cls in (TEAM, WAVE_DIRECT, WAVE_SEARCH, BLOCK_DIRECT, BLOCK_SEARCH, GLOBAL):
        assert rows[cls] > 0, f"class {cls} has no rows in bin_zoo + tiny_zoo"
    assert rows[7] == 0


# wave rows whose A entries need more than one stage (64 entries a stage, 256 in a block)
def test_values_wave_rows_with_many_a_entries(tool):
    (_, K, _, _, _), Bt = tiny_zoo(7)
    _, N, Bp, Bc, Bv = Bt
    rng = np.random.default_rng(23)
    blen = np.diff(Bp)
    narrow = np.nonzero((np.arange(K) % 5 == 1))[0]               # B rows inside columns [0, 200): a direct span
    wide = np.nonzero((np.arange(K) % 5 >= 2) & (blen > 0))[0]    # B rows anywhere in [0, 5000): searched
    arows = []
    for na in (65, 100, 150, 257, 300):
        arows.append(np.sort(rng.choice(narrow, na, replace=False)))
        arows.append(np.sort(rng.choice(wide, na, replace=False)))
    arows.append(np.sort(rng.choice(wide, 700, replace=False)))    # past the wave's product cap: a block's row
    Ap = np.zeros(len(arows) + 1, np.int64)
    Ap[1:] = np.cumsum([len(r) for r in arows])
    Ac = np.concatenate(arows).astype(np.int32)
    A = mhspgemm.CSR(len(arows), K, Ap.astype(np.int32), Ac, rng.uniform(0.1, 1.0, len(Ac)))
    info = values_check(tool, A, csr_of(Bt), seed=9)
    # narrow rows: wave-direct with 65..300 A entries (2..5 stages); wide rows: the 65-entry one is searched
    # by a wave (span > 16 n), the denser ones go to a block's direct table, three of them past its 256-entry stage
    assert info["rows"][WAVE_DIRECT] >= 5 and info["rows"][WAVE_SEARCH] >= 1 and info["rows"][BLOCK_DIRECT] >= 3, info


# 4. mixed signs: the bound is 1e-6 of the product on absolute values
def test_values_random_rect_signed(tool):
    p, c, v = random_csr(3000, 2000, 7, 1)
    Bp, Bc, Bv = random_csr(2000, 50_000, 12, 101)
    values_check(tool, mhspgemm.CSR(3000, 2000, p, c, v), mhspgemm.CSR(2000, 50_000, Bp, Bc, Bv), signed=True)


# 5. banded: the direct classes take most rows
def test_values_fem_grid_is_direct(tool):
    A = synth.fem_grid(12, 10, 8)
    info = values_check(tool, A, A)
    assert info["rows"][WAVE_DIRECT] + info["rows"][BLOCK_DIRECT] > 0.5 * A.M, info


def scatter_into(Cp, Ci, N, Sp, Si, Sv):
    """Values Sv of the pattern (Sp, Si), a subset of (Cp, Ci), at C's positions; 0.0 elsewhere."""
    rowsC = np.repeat(np.arange(len(Cp) - 1, dtype=np.int64), np.diff(Cp))
    rowsS = np.repeat(np.arange(len(Sp) - 1, dtype=np.int64), np.diff(Sp))
    keyC = rowsC * N + Ci
    keyS = rowsS * N + Si
    pos = np.searchsorted(keyC, keyS)
    assert np.array_equal(keyC[pos], keyS)
    out = np.zeros(len(Ci))
    out[pos] = Sv
    return out, pos


# 6. C's pattern a strict superset of the product's
def test_values_superset_pattern(tool):
    p, c, v = random_csr(1500, 1000, 7, 5)
    Bp, Bc, Bv = random_csr(1000, 20_000, 10, 6)
    A, B = mhspgemm.CSR(1500, 1000, p, c, v), mhspgemm.CSR(1000, 20_000, Bp, Bc, Bv)
    keep = np.ones(A.nnz, bool)
    keep[::7] = False  # every 7th entry of A removed: ptr rebuilt, columns a subset
    rows = np.repeat(np.arange(A.M), np.diff(p))
    p2 = np.zeros(A.M + 1, np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=A.M), out=p2[1:])
    A2 = mhspgemm.CSR(A.M, A.N, p2.astype(np.int32), c[keep], v[keep])
    A2.H2D(tool.device)
    C = product(tool, A, B)
    try:
        plan = mhspgemm.ValuesPlan(tool, A2, B, C)
        try:
            plan.run()
            gp, gc, gv = C.to_host()
        finally:
            plan.close()
    finally:
        C.release()
    Sp, Si, Sv = orc.spgemm(A2.ptr, A2.col, A2.val, B.ptr, B.col, B.val, B.N)
    assert Sp[-1] < gp[-1], "the case needs entries of C that A'*B does not reach"
    want, pos = scatter_into(gp, gc, B.N, Sp, Si, Sv)
    unreached = np.ones(len(gc), bool)
    unreached[pos] = False
    assert unreached.any() and np.all(gv[unreached] == 0.0), "unreached entries must be exactly 0.0"
    assert_values(gp, gc, want, gp, gc, gv)


@functools.lru_cache(maxsize=None)
def zoo_operands():
    At, Bt = bin_zoo()
    return csr_of(At), csr_of(Bt)


# 7. idempotence and a separate output (a missing zero fill shows here, above all in the global class)
def test_values_idempotent_and_separate_output(tool):
    A, B = zoo_operands()
    C = product(tool, A, B)
    try:
        plan = mhspgemm.ValuesPlan(tool, A, B, C)
        try:
            assert plan.info()["rows"][GLOBAL] > 0
            plan.run()
            p, c, v1 = C.to_host()
            plan.run()
            _, _, v2 = C.to_host()
            out = torch.full((C.nnz,), float("nan"), dtype=torch.float64, device=f"cuda:{tool.device}")
            torch.cuda.synchronize()
            plan.run(out=out)
            v3 = out.cpu().numpy()
            _, _, v2_after = C.to_host()
        finally:
            plan.close()
    finally:
        C.release()
    assert np.array_equal(v2, v2_after), "C.val untouched by a call with its own output"
    Cp, Ci, Cv = orc.spgemm(A.ptr, A.col, A.val, B.ptr, B.col, B.val, B.N)
    for v in (v1, v2, v3):
        assert_values(Cp, Ci, Cv, p, c, v)


# 8. stream order: MHS_OPT_SYNC 0 on torch's current stream, ms = None
def test_values_stream_ordered(tool):
    p, c, v = random_csr(2000, 2000, 8, 21)
    A = mhspgemm.CSR(2000, 2000, p, c, v)
    C = product(tool, A, A)
    av, bv = new_values(A.nnz, 31), new_values(A.nnz, 32)
    try:
        plan = mhspgemm.ValuesPlan(tool, A, A, C)
        dA, dB = upload(tool, av), upload(tool, bv)
        out = torch.full((C.nnz,), float("nan"), dtype=torch.float64, device=f"cuda:{tool.device}")
        tool.set_option(_lib.MHS_OPT_SYNC, 0)
        tool.set_stream(torch.cuda.current_stream(tool.device).cuda_stream)
        try:
            assert plan.run(dA, dB, out=out) is None
            torch.cuda.synchronize()
            gv = out.cpu().numpy()
        finally:
            tool.set_option(_lib.MHS_OPT_SYNC, 1)
            tool.set_stream(None)
            plan.close()
        gp, gc, _ = C.to_host()
    finally:
        C.release()
    Cp, Ci, Cv = orc.spgemm(p, c, av, p, c, bv, A.N)
    assert_values(Cp, Ci, Cv, gp, gc, gv)


# 9. a full product on the same context between two values calls
def test_values_interleaved_with_spgemm(tool):
    p, c, v = random_csr(2500, 2500, 9, 41)
    A = mhspgemm.CSR(2500, 2500, p, c, v)
    q, d, w = random_csr(1200, 900, 6, 42)
    X = mhspgemm.CSR(1200, 900, q, d, w)
    Yp, Yc, Yv = random_csr(900, 4000, 8, 43)
    Y = mhspgemm.CSR(900, 4000, Yp, Yc, Yv)
    C = product(tool, A, A)
    try:
        plan = mhspgemm.ValuesPlan(tool, A, A, C)
        try:
            a1, b1 = new_values(A.nnz, 51), new_values(A.nnz, 52)
            plan.run(upload(tool, a1), upload(tool, b1))
            gp, gc, g1 = C.to_host()
            Z = product(tool, X, Y)  # an unrelated pair through the same context (workspace, pool, streams)
            try:
                zp, zc, zv = Z.to_host()
            finally:
                Z.release()
            a2, b2 = new_values(A.nnz, 53), new_values(A.nnz, 54)
            plan.run(upload(tool, a2), upload(tool, b2))
            _, _, g2 = C.to_host()
        finally:
            plan.close()
    finally:
        C.release()
    assert_values(*orc.spgemm(p, c, a1, p, c, b1, A.N), gp, gc, g1)
    assert_values(*orc.spgemm(q, d, w, Yp, Yc, Yv, Y.N), zp, zc, zv)
    assert_values(*orc.spgemm(p, c, a2, p, c, b2, A.N), gp, gc, g2)


# 10. rejections at create; the context stays usable
def test_values_rejections_at_create(tool):
    p, c, v = random_csr(400, 300, 6, 61)
    Bp, Bc, Bv = random_csr(300, 2000, 8, 62)
    A, B = mhspgemm.CSR(400, 300, p, c, v), mhspgemm.CSR(300, 2000, Bp, Bc, Bv)
    A.H2D(tool.device)
    B.H2D(tool.device)
    Cp, Ci, Cv = orc.spgemm(p, c, v, Bp, Bc, Bv, B.N)
    row = int(np.argmax(np.diff(Cp) >= 3))  # a row with at least three entries, each reached by a product
    assert Cp[row + 1] - Cp[row] >= 3

    def on_device(ptr, col, M=A.M):
        X = mhspgemm.CSR(M, B.N, ptr, col, np.zeros(len(col)))
        X.H2D(tool.device)
        return X

    # (i) one column removed from a row that a product reaches
    k = Cp[row] + 1
    ptr1 = Cp.copy()
    ptr1[row + 1:] -= 1
    # (ii) two columns of one row swapped
    col2 = Ci.copy()
    col2[[k, k + 1]] = col2[[k + 1, k]]
    # (iii) C.M != A.M
    ptr3 = np.append(Cp, Cp[-1]).astype(np.int32)
    bad = [("misses a column", on_device(ptr1, np.delete(Ci, k))), ("ascending", on_device(Cp, col2)),
           ("C.M != A.M", on_device(ptr3, Ci, A.M + 1))]
    for word, X in bad:
        with pytest.raises(mhspgemm.MHSpGEMMError) as e:
            mhspgemm.ValuesPlan(tool, A, B, X)
        assert e.value.status == 3 and word in str(e.value), str(e.value)
        if word != "C.M != A.M":
            assert f"row {row}" in str(e.value), str(e.value)  # the first bad row is named
    good = on_device(Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, A, B, good)
    try:
        plan.run()
        torch.cuda.synchronize()
        gv = good.d_val.cpu().numpy()
    finally:
        plan.close()
    assert_values(Cp, Ci, Cv, Cp, Ci, gv)
