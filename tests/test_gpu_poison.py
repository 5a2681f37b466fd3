"""GPU tests of the promise that a call depends on nothing an earlier call left in device memory.

The workspace, the global-bin scratch and the value slots are cached across calls and never cleared, C's arrays
come out of a pool of released ones or fresh from hipMalloc, and a values plan keeps lists, B^T and (while it is
built) a sort scratch of its own.  A repeated call therefore finds the previous call's correct results already in
place -- the same row pointer, columns and values in the recycled C, the same bins, caches and offsets in the
workspace -- and a first call finds whatever fresh device memory holds, which the HIP runtime does not define.  A
kernel that skips rows, a launch left out although something reads its output, a table that is never cleared:
none of it shows in a suite whose memory is either right already or happens to be zero.

Contexts here are created with MHS_POISON=<byte> (include/mhspgemm.h, MHS_STAT_POISON_FILLS):
every buffer the library allocates for its own work, every buffer the pool hands out and, at the start of every
attempt of mhs_spgemm, the whole cached workspace, scratch and slots are filled with the byte.  Two bytes: 0xFF
(ints of -1, NaN doubles, bin bytes of 255) and 0x7F (ints of 0x7f7f7f7f, doubles of about 1.4e306) -- -1 is a
legal sentinel in places, a huge positive int nowhere.

a. the switch reaches what a caller can see; b. every full-call path three times in one context on the same
device arrays, the second and third call speculated hits on a recycled C; c. speculation under duress: values and
pattern changed in place, symbolic launches left out, a miss whose rerun runs them; d. values plans created and
run on a poisoned context, with a full call between two runs; e. the transpose and its radix sort's bit-count
edges.  Every result is held to the check its path has elsewhere in the suite: patterns bit-exact against the
oracle, FP64 values within 1.01 m 2^-53 S of long-double sums, semiring values and transposes bit-exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mhspgemm
from mhspgemm import _lib as L
from oracle import oracle as orc
from _util import assert_f64_bound, bin_zoo, device_csr, exact_forward, random_csr, with_hub_row
import test_gpu_semiring as sr
import test_gpu_subgrad as sub
import test_gpu_values_batched as vb
import test_gpu_witness as wit
from test_gpu_f64_bound import fresh_tool, masked_case, plain_case, plan_check, reference
from test_gpu_nonfinite import CALLS  # FULL_CALLS and perturbed_fem_row_chunked
from test_gpu_parity import test_device_transpose_bit_exact as _transpose_shapes
from test_gpu_spec_duress import overwrite

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x7F)
poisons = pytest.mark.parametrize("byte", POISONS, ids=["0xFF", "0x7F"])


@pytest.fixture(autouse=True)
def _no_switch_from_outside(monkeypatch):
    """The contexts of this file get MHS_POISON from fresh_tool or not at all."""
    monkeypatch.delenv("MHS_POISON", raising=False)


def poisoned_tool(tool, byte, env=None, options=None):
    return fresh_tool(tool, {**(env or {}), "MHS_POISON": str(byte)}, options or {})


def device_bytes(t, address, n):
    """n bytes at a device address, through mhs_memcpy (ordered on the context's stream)."""
    out = np.zeros(n, np.uint8)
    assert L.lib().mhs_memcpy(t.ctx, out.ctypes.data, ctypes.c_void_p(address), n, 1) == L.MHS_OK
    return out


def on_device(tool, *mats):
    for X in mats:
        if X.d_ptr is None:
            X.H2D(tool.device)


def released(*mats):
    for X in mats:
        X.d_release_csr()


class Since:
    """A context's counters since this object was made: the censuses of FULL_CALLS count the calls of a context
    that has made one call, and hold here for each call of several."""

    def __init__(self, t):
        self.t = t
        self.base = {k: t.stat(k) for k in t.STATS}

    def stat(self, name):
        return self.t.stat(name) - self.base[name]

    def chunked_calls(self):
        return self.stat("chunked")


def judged(t, A, B, Cp, Ci, exact, what, timing=True):
    """One full call judged as test_gpu_f64_bound.judged_call judges it -- row_ptr and col_idx the oracle's, the
    values within the bound, the timing's counts on a timed call -- with C released (recycled) before the return.
    Returns (timing, the three device addresses C had)."""
    C, tm = mhspgemm.spgemm(t, A, B, timing=timing)
    where = (C.c.ptr, C.c.col, C.c.val)
    try:
        p, c, v = C.to_host()
    finally:
        C.release()
    assert np.array_equal(p, Cp), f"{what}: row_ptr must be bit-exact"
    assert np.array_equal(c, Ci), f"{what}: col_idx must be bit-exact"
    assert_f64_bound(v, *exact, f"full call, {what}")
    if timing:
        assert tm.nnzC == Cp[-1] and tm.flop == exact[1].sum()  # (m sums to the products: the pattern is the product's own)
    return tm, where


# ------------------------------------------- a. the switch reaches what a caller can see ---
@poisons
def test_poison_reaches_fresh_and_pooled_c(tool, byte):
    """An all-empty A: C.col and C.val are alloc_c's 16 bytes each, which no kernel writes.  They hold the poison on
    the first call (fresh allocations) and again on the second, which takes them from the pool -- where the test has
    left zeros in them."""
    A = mhspgemm.CSR(5, 5, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0))
    A.H2D(tool.device)
    t2 = poisoned_tool(tool, byte)
    try:
        assert t2.stat("poison_fills") == 0
        zeros = np.zeros(16, np.uint8)
        firsts = None
        for call in range(2):
            C, _ = mhspgemm.spgemm(t2, A, A)
            try:
                assert (C.M, C.N, C.nnz) == (5, 5, 0)
                assert C.c.col and C.c.val
                for address in (C.c.col, C.c.val):
                    got = device_bytes(t2, address, 16)
                    assert np.all(got == byte), (call, got)
                    assert L.lib().mhs_memcpy(t2.ctx, ctypes.c_void_p(address), zeros.ctypes.data, 16, 0) == L.MHS_OK
                assert np.array_equal(C.to_host()[0], np.zeros(6, np.int32))
                if call == 0:
                    firsts = {C.c.ptr, C.c.col, C.c.val}
                else:
                    assert {C.c.col, C.c.val} <= firsts, "the second call's arrays come out of the pool"
            finally:
                C.release()
            assert t2.stat("poison_fills") > 0
    finally:
        t2.close()
        released(A)


@poisons
def test_poison_reaches_transpose_outputs(tool, byte):
    A = mhspgemm.CSR(3, 7, np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0))
    A.H2D(tool.device)
    t2 = poisoned_tool(tool, byte)
    try:
        T = mhspgemm.transpose(t2, A)
        try:
            assert (T.M, T.N, T.nnz) == (7, 3, 0)
            assert np.array_equal(T.dev.to_host()[0], np.zeros(8, np.int32))
            assert np.all(device_bytes(t2, T.dev.c.col, 4) == byte)
            assert np.all(device_bytes(t2, T.dev.c.val, 8) == byte)
        finally:
            T.d_release_csr()
        assert t2.stat("poison_fills") > 0
    finally:
        t2.close()
        released(A)


def test_no_poison_without_the_switch(tool):
    A, B, Cp, Ci, exact = reference("bin_zoo", "narrow")
    on_device(tool, A, B)
    t2 = fresh_tool(tool, {}, {})
    try:
        for call in range(2):
            judged(t2, A, B, Cp, Ci, exact, f"no switch, call {call}")
        T = mhspgemm.transpose(t2, A)
        T.d_release_csr()
        assert t2.stat("spec") == 1 and t2.stat("poison_fills") == 0
        assert L.lib().mhs_ctx_stat(t2.ctx, L.MHS_STAT_POISON_FILLS) == 0 and L.lib().mhs_ctx_stat(t2.ctx, 11) == -1
    finally:
        t2.close()
        released(A, B)


# --------------------------- b. every full-call path, three calls on the same arrays ---
@poisons
@pytest.mark.parametrize("case", list(CALLS))
def test_poisoned_full_call_three_times(tool, case, byte):
    """Call 1 timed, without a plan; call 2 timed; call 3 with MHS_OPT_SYNC 0 and untimed.  Each C is read and
    recycled before the next call, so calls 2 and 3 get call 1's three arrays back -- poisoned -- and a workspace
    poisoned at their start: wherever the path speculates they are hits, whose pattern outputs nothing else has
    put in place."""
    name, env, options, census = CALLS[case]
    A, B, Cp, Ci, exact = reference(name, "narrow")
    on_device(tool, A, B)
    t2 = poisoned_tool(tool, byte, env, options)
    chunked = L.MHS_OPT_MEM_BUDGET in options
    speculates = L.MHS_OPT_TINY_FIRST_ROWS not in options and not chunked  # (test_gpu_scale_edges.py's rule)
    try:
        first = None
        for call in (1, 2, 3):
            since = Since(t2)
            if call == 3:
                t2.set_option(L.MHS_OPT_SYNC, 0)
            tm, where = judged(t2, A, B, Cp, Ci, exact, f"{case}, poison {byte:#x}, call {call}", timing=call < 3)
            if call < 3:
                census(since, tm, A.M)
            if call == 1:
                first = where
                assert t2.stat("spec") == 0
            elif call == 2 and not chunked:  # (the row-chunked call frees the pool)
                assert set(where) == set(first), "call 2's C is not the three arrays call 1 released"
            assert since.stat("poison_fills") > 0
        assert (t2.stat("spec"), t2.stat("spec_miss")) == (2 * int(speculates), 0), (t2.stat("spec"), t2.stat("spec_miss"))
    finally:
        t2.close()
        released(A, B)


# ------------------------------------------------------- c. speculation under duress ---
@functools.lru_cache(maxsize=None)
def zoo_contents():
    """bin_zoo's operands as test_speculated_plan_miss_and_values changes them in place: the zoo, new values of A,
    then a new pattern of A with the same row lengths.  Each with the oracle's pattern and the exact sums."""
    (M, K, Ap, Ac, Av), (K2, N, Bp, Bc, Bv) = bin_zoo()
    Av2 = Av * 1.5 + 0.25
    rng = np.random.default_rng(3)
    Ac2 = Ac.copy()
    for r in range(M):
        a0, a1 = int(Ap[r]), int(Ap[r + 1])
        if a1 > a0:
            Ac2[a0:a1] = np.sort(rng.choice(K, a1 - a0, replace=False)).astype(np.int32)
    B = mhspgemm.CSR(K2, N, Bp, Bc, Bv)
    out = []
    for col, val in ((Ac, Av), (Ac, Av2), (Ac2, Av2)):
        A = mhspgemm.CSR(M, K, Ap, col, val)
        Cp, Ci, _ = orc.spgemm(A.ptr, A.col, A.val, B.ptr, B.col, B.val, N)
        out.append((A, Cp, Ci, exact_forward(A, B, Cp, Ci, A.val, B.val)))
    return B, out


@poisons
def test_poisoned_speculation_miss_and_values(tool, byte, monkeypatch):
    """test_speculated_plan_miss_and_values' sequence on a poisoned context: call, hit, new values in place (hit),
    new pattern in place (miss and rerun), hit -- each judged against the oracle of the contents then in the
    arrays, with that test's counts."""
    monkeypatch.setenv("MHS_SPEC_NSS", "4")
    Bh, contents = zoo_contents()
    A = mhspgemm.CSR(contents[0][0].M, contents[0][0].N, contents[0][0].ptr, contents[0][0].col, contents[0][0].val)
    B = mhspgemm.CSR(Bh.M, Bh.N, Bh.ptr, Bh.col, Bh.val)
    on_device(tool, A, B)
    t2 = poisoned_tool(tool, byte)
    try:
        counts = []
        for call, k in enumerate((0, 0, 1, 2, 2)):
            Ah, Cp, Ci, exact = contents[k]
            if call in (2, 3):
                A.d_val.copy_(torch.from_numpy(Ah.val))
                A.d_col.copy_(torch.from_numpy(Ah.col))
                torch.cuda.synchronize()
            tm, _ = judged(t2, A, B, Cp, Ci, exact, f"bin_zoo in place, poison {byte:#x}, call {call}")
            # both patterns have rows in the rare symbolic bins (1024-thread, global, 10 KiB wave)
            assert tm.sym_bins[3] + tm.sym_bins[4] + tm.sym_bins[11] > 0, tm.sym_bins
            counts.append((t2.stat("spec"), t2.stat("spec_miss")))
        assert counts == [(0, 0), (1, 0), (2, 0), (3, 1), (4, 1)], counts
        assert t2.stat("sym_fork") == 4 and t2.stat("spec_skipped") == 0, (t2.stat("sym_fork"), t2.stat("spec_skipped"))
    finally:
        t2.close()
        released(A, B)


SHORT_M, SHORT_PER, SHORT_SEED, HUB = 3000, 4, 21, 1500


@functools.lru_cache(maxsize=None)
def short_rows():
    """Rows of about 4 entries, whose speculated calls leave the rare symbolic launches out, and the same arrays
    with one hub row of 1500 columns (with_hub_row: the same M and nnz)."""
    p, c, v = random_csr(SHORT_M, SHORT_M, SHORT_PER, SHORT_SEED)
    out = []
    for ptr, col in ((p, c), with_hub_row(p, c, SHORT_M, HUB)):
        A = mhspgemm.CSR(SHORT_M, SHORT_M, ptr, col, v)
        Cp, Ci, _ = orc.spgemm(A.ptr, A.col, A.val, A.ptr, A.col, A.val, A.N)
        out.append((A, Cp, Ci, exact_forward(A, A, Cp, Ci, A.val, A.val)))
    return out


@poisons
def test_poisoned_speculation_leaves_launches_out(tool, byte):
    """Speculated calls that leave symbolic launches out (MHS_STAT_SPEC_SKIPPED) on a poisoned workspace and a
    poisoned, recycled C; then one hub row written into the same arrays: its bin was empty in the plan, so the
    launch that counts it was left out and its row pointer slot holds the poison -- the scan must reject the plan
    and the rerun run the bins the plan had empty."""
    (A0, Cp0, Ci0, exact0), (A1, Cp1, Ci1, exact1) = short_rows()
    A = mhspgemm.CSR(A0.M, A0.N, A0.ptr, A0.col, A0.val)
    A.H2D(tool.device)
    t2 = poisoned_tool(tool, byte)
    try:
        tm0 = None
        for call in range(3):
            tm, _ = judged(t2, A, A, Cp0, Ci0, exact0, f"short rows, poison {byte:#x}, call {call}")
            tm0 = tm0 or tm
            assert list(tm.sym_bins) == list(tm0.sym_bins) and list(tm.num_bins) == list(tm0.num_bins)
        assert (t2.stat("spec"), t2.stat("spec_miss")) == (2, 0)
        assert t2.stat("spec_skipped") >= 1, t2.stat("spec_skipped")
        overwrite(A, A1.ptr, A1.col)
        tm, _ = judged(t2, A, A, Cp1, Ci1, exact1, f"short rows with a hub row, poison {byte:#x}")
        assert (t2.stat("spec"), t2.stat("spec_miss")) == (3, 1)
        new = [b for b in range(1, 16) if tm0.sym_bins[b] == 0 and tm.sym_bins[b] > 0]
        print(f"sym_bins {list(tm0.sym_bins)} -> {list(tm.sym_bins)}: bins {new} were empty in the plan")
        assert new, "the hub row lands in a symbolic bin the plan had empty"
        judged(t2, A, A, Cp1, Ci1, exact1, f"short rows with a hub row, poison {byte:#x}, the call repeated")
        assert (t2.stat("spec"), t2.stat("spec_miss")) == (4, 1)
    finally:
        t2.close()
        released(A)


# ----------------------------- d. values plans created and run on a poisoned context ---
def full_call_between(t, A, B):
    """A full mhs_spgemm on the plan's context between two runs of the plan: it poisons and rewrites the workspace
    and takes C from the pool, none of which is the plan's."""
    def between():
        C, _ = mhspgemm.spgemm(t, A, B)
        C.release()
    return between


def info_on(tool, A, B, Cp, Ci, **kw):
    """info() of the same plan made on another context (the session's: no poison)."""
    on_device(tool, A, B)
    plan = mhspgemm.ValuesPlan(tool, A, B, device_csr(tool, A.M, B.N, Cp, Ci), **kw)
    try:
        return plan.info()
    finally:
        plan.close()


@poisons
def test_poisoned_plain_plan(tool, byte):
    A, B, (Cp, Ci) = plain_case("bin_zoo")
    t2 = poisoned_tool(tool, byte)
    try:
        on_device(tool, A, B)
        info = plan_check(t2, A, B, Cp, Ci, f"values plan on a poisoned context ({byte:#x}), bin_zoo", seed=3,
                          between=full_call_between(t2, A, B))
        assert t2.stat("poison_fills") > 0
        assert info == info_on(tool, A, B, Cp, Ci)
    finally:
        t2.close()
        released(A, B)


@poisons
@pytest.mark.parametrize("form", ["product", "dot", "auto"])
@pytest.mark.parametrize("case", ["triangle", "thinned_with_strangers"])
def test_poisoned_masked_plan(tool, case, form, byte):
    A, B, Mp, Mc = masked_case(case)
    t2 = poisoned_tool(tool, byte)
    try:
        on_device(tool, A, B)
        info = plan_check(t2, A, B, Mp, Mc, f"masked plan on a poisoned context ({byte:#x}), {form} form, {case}",
                          masked=True, form=form, seed=9, between=full_call_between(t2, A, B))
        assert 0 < info["kept_products"] < info["products"]
        if form != "auto":
            assert (info["rows"][7] > 0) == (form == "dot"), info
        assert info == info_on(tool, A, B, Mp, Mc, masked=True, form=form)
    finally:
        t2.close()
        released(A, B)


@poisons
def test_poisoned_f32_width_4_plan(tool, byte):
    A, B = vb.product_input("bin_zoo")[:2]
    t2 = poisoned_tool(tool, byte)
    try:
        on_device(tool, A, B)
        info = vb.run_every_set(t2, "bin_zoo", "f32", 4, between=full_call_between(t2, A, B))
        assert info == vb.every_set(tool, "bin_zoo", "f32", 4)
    finally:
        t2.close()
        released(A, B)


@poisons
def test_poisoned_min_plus_plan(tool, byte):
    A, B, Cp, Ci, pqs = sr.case("bin_zoo")
    t2 = poisoned_tool(tool, byte)
    dA, dB, dC = sr.on_device(tool, A, B, Cp, Ci)
    try:
        av, bv = sr.sr_values(A.nnz, 3), sr.sr_values(B.nnz, 1003)
        got, info = sr.run_plan(t2, dA, dB, dC, "min_plus", av, bv, calls=2, between=full_call_between(t2, dA, dB))
        want = sr.reference("min_plus", pqs, av, bv, len(Ci))
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
        plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, semiring="min_plus")
        try:
            assert info == plan.info()
        finally:
            plan.close()
    finally:
        t2.close()
        released(dA, dB, dC)


@poisons
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("semiring", sr.SEMIRINGS)
def test_poisoned_semiring_subgrad_and_witness(tool, semiring, dtype, byte):
    """The subgradient and the witness of a semiring plan created on a poisoned context -- its row lists and counters
    are allocated under poison, and the pre-fills of ties and wit are all that stands between the kernels and the
    poison byte -- twice each, a full call on the context ahead of every call after the first.  The exact regime of
    tests/test_gpu_subgrad.py: ties, dA, dB and wit equal the reference on every call."""
    A, B, Cp, Ci, pqs = sr.case("bin_zoo")
    nC = len(Ci)
    av, bv = sub.exact_values(semiring, A, B, 600)
    c = sr.reference(semiring, pqs, av, bv, nC, dtype)
    win, T = sub.winners(semiring, pqs, av, bv, c, dtype)
    assert (T == 0).any() and (T >= 2).any(), "entries the ties pre-fill alone writes, and entries with ties"
    g = np.random.default_rng(601).integers(-2, 3, nC).astype(np.float64)
    G = np.where(T > 0, T * g, np.nan)
    wA, wB = sub.exact_reference(semiring, pqs, win, T, av, bv, G, A.nnz, B.nnz, dtype)
    wW, _ = wit.witness_reference(semiring, A, pqs, av, bv, c, dtype)
    assert (wW == -1).any() and (wW >= 0).any(), "entries the wit pre-fill alone writes, and entries with a witness"
    t2 = poisoned_tool(tool, byte)
    dA, dB, dC = sr.on_device(tool, A, B, Cp, Ci)
    try:
        plan = mhspgemm.ValuesPlan(t2, dA, dB, dC, dtype=dtype, semiring=semiring)
        try:
            info = plan.info()
            between = full_call_between(t2, dA, dB)
            cdev = sub.forward_values(t2, plan, nC, dtype, av, bv)
            assert np.array_equal(cdev.cpu().numpy(), c), "the forward"
            for k in range(2):
                for what in ("subgrad", "witness"):
                    if k or what == "witness":
                        between()
                        assert plan.info() == info, "the plan after other work on its context"
                    if what == "subgrad":
                        _, gA, gB, ties = sub.call(t2, plan, A.nnz, B.nnz, nC, dtype, av, bv, G, cval=cdev)
                        assert np.array_equal(ties, T), f"ties, call {k}"
                        assert np.array_equal(gA, wA) and np.array_equal(gB, wB), f"dA and dB, call {k}"
                    else:
                        _, w = wit.call(t2, plan, nC, dtype, av, bv, cval=cdev)
                        assert np.array_equal(w, wW), f"wit, call {k}"
            assert t2.stat("poison_fills") > 0
        finally:
            plan.close()
        plain = mhspgemm.ValuesPlan(tool, dA, dB, dC, dtype=dtype, semiring=semiring)
        try:
            assert info == plain.info(), "info() is the unpoisoned context's"
        finally:
            plain.close()
    finally:
        t2.close()
        released(dA, dB, dC)


# ------------------------------------------------------------------ e. the transpose ---
def transposed_bit_exact(t, M, N, p, c, v, what):
    A = mhspgemm.CSR(M, N, p, c, v)
    A.H2D(t.device)
    try:
        T = mhspgemm.transpose(t, A)
        tp, tc, tv = T.dev.to_host()
        T.d_release_csr()
    finally:
        released(A)
    oM, oN, op, oc, ov = orc.transpose(M, N, p, c, v)
    assert (T.M, T.N) == (N, M) == (oM, oN), what
    assert np.array_equal(tp, op) and np.array_equal(tc, oc), what
    assert np.array_equal(tv.view(np.uint64), np.ascontiguousarray(ov, np.float64).view(np.uint64)), what


TRANSPOSE_SHAPES = [m.args[1] for m in _transpose_shapes.pytestmark if m.name == "parametrize"][0]


@poisons
@pytest.mark.parametrize("shape", TRANSPOSE_SHAPES)
def test_poisoned_transpose_shapes(tool, shape, byte):
    """The shapes of test_device_transpose_bit_exact on a poisoned context."""
    M, N, per = shape
    p, c, v = random_csr(M, N, per, seed=M + N)
    t2 = poisoned_tool(tool, byte)
    try:
        transposed_bit_exact(t2, M, N, p, c, v, f"{shape}, poison {byte:#x}")
    finally:
        t2.close()


@functools.lru_cache(maxsize=None)
def sort_edge_matrix(N, trailing):
    """700 rows by N columns: 70 leading and 50 trailing empty rows (and empty rows between), 37 leading and
    `trailing` trailing empty columns, columns unsorted within a row, and every fifth entry a duplicate of the one
    before it in its row.  trailing == 0: the last column, N - 1, is used -- with N = 2^k + 1 the one key that has
    the sort's top bit."""
    rng = np.random.default_rng(N + trailing)
    M, lead, trail, c0 = 700, 70, 50, 37
    lens = np.zeros(M, np.int64)
    lens[lead:M - trail] = rng.poisson(6, M - lead - trail)
    lens[[lead + 9, lead + 10, lead + 11, M // 2]] = 0
    ptr = np.zeros(M + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    col = rng.integers(c0, N - trailing, int(ptr[-1]))
    first = np.zeros(len(col), bool)
    first[ptr[:-1][lens > 0]] = True
    dup = (np.arange(len(col)) % 5 == 4) & ~first
    col[dup] = col[np.nonzero(dup)[0] - 1]
    if trailing == 0:
        col[len(col) // 2] = N - 1
    val = rng.uniform(0.1, 1.0, len(col)) * rng.choice([-1.0, 1.0], len(col))
    col = col.astype(np.int32)
    assert lens[:lead].sum() == 0 and lens[M - trail:].sum() == 0 and (lens[lead:M - trail] == 0).any()
    assert col.min() >= c0 and col.max() < N - trailing and (trailing > 0 or col.max() == N - 1)
    rows = np.repeat(np.arange(M), lens)
    assert len(np.unique(rows * N + col)) < len(col) - len(col) // 8, "duplicate entries"
    return M, ptr.astype(np.int32), col, val


@poisons
@pytest.mark.parametrize("trailing", [21, 0], ids=["empty_last_columns", "last_column_used"])
@pytest.mark.parametrize("N", [1024, 1025], ids=["N_2^10", "N_2^10+1"])
def test_poisoned_transpose_sort_edges(tool, N, trailing, byte):
    M, p, c, v = sort_edge_matrix(N, trailing)
    t2 = poisoned_tool(tool, byte)
    try:
        transposed_bit_exact(t2, M, N, p, c, v, f"N {N}, {trailing} empty last columns, poison {byte:#x}")
    finally:
        t2.close()
