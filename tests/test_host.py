"""CPU tests of the host layer: the C-ABI library loads and exports every
symbol include/mhspgemm.h declares, the product's Matrix Market reader agrees
with the golden fixtures and the oracle reader, the reference-mirroring Python
surface (Timing, CSR ==) behaves like the reference, synthetic generators are
well-formed.  No compute call reaches the GPU here."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mhspgemm
from mhspgemm import _lib, synth
from oracle import oracle as orc
from _util import GOLDEN, PRODUCT_CASES, READ_CASES, load_golden

ROOT = Path(__file__).resolve().parent.parent


def test_library_exports_every_declared_symbol():
    L = _lib.lib()
    names = _lib.declared_functions()
    assert len(names) >= 15
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(names) <= exported
    assert L.mhs_abi_version() == 10


def test_output_owner_under_sanitizers(tmp_path):
    # the owner of a call's C arrays (csrc/mhs_owner.hpp) has no HIP in it: tests/owner_check.cpp runs
    # commit, early exits with and without queued work, the miss hand-back and double release on the host
    exe = tmp_path / "owner_check"
    cc = subprocess.run(["c++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", str(ROOT / "tests" / "owner_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "owner ok", run.stdout + run.stderr


def test_numeric_plan_under_sanitizers(tmp_path):
    # the numeric launch plan (csrc/mhs_numplan.hpp) is a HIP-free function of the published Stats:
    # tests/numplan_check.cpp checks every bin's launch, the split and fused cases, the thresholds, the
    # speculation premise and the dealing rule against hand-computed literals on the host
    exe = tmp_path / "numplan_check"
    cc = subprocess.run(["c++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", str(ROOT / "tests" / "numplan_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "numplan ok", run.stdout + run.stderr


def test_front_plan_under_sanitizers(tmp_path):
    # the pre-numeric launch plans (csrc/mhs_frontplan.hpp) are HIP-free functions of the call's shape and a
    # speculated call's Stats: tests/frontplan_check.cpp checks the mask / analyze / scan geometry on both
    # sides of every edge, k_sym_common's roles, the skip rules, the forked order and the set of kernel
    # variants the rules reach against hand-computed literals on the host
    exe = tmp_path / "frontplan_check"
    cc = subprocess.run(["c++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", str(ROOT / "tests" / "frontplan_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "frontplan ok", run.stdout + run.stderr


def test_vendor_library_exports_every_declared_symbol():
    # rocSPARSE comparison row (include/mhs_vendor.h): loads without a GPU, exports its two entries
    V = _lib.vendor_lib()
    names = _lib.declared_functions(_lib.VENDOR_HEADER)
    assert names == ["mhs_vendor_free", "mhs_vendor_spgemm"]
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.VENDOR_PATH)], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(names) <= exported and all(hasattr(V, n) for n in names)


def test_library_is_gfx950_code_object():
    data = Path(_lib.lib_path()).read_bytes()
    # every offload-bundle target is gfx950 (rocPRIM's host-side tuning tables name other
    # architectures as strings; only the code-object targets count)
    targets = set(re.findall(rb"amdgcn-amd-amdhsa--(gfx\w+)", data))
    assert targets == {b"gfx950"}, targets


@pytest.mark.parametrize("name", READ_CASES)
def test_product_reader_matches_golden(name):
    d, p, c, v = load_golden(name)
    A = mhspgemm.CSR()
    assert mhspgemm.readMtxFile(A, str(GOLDEN / d["file"])) == 0
    assert (A.M, A.N) == (d["M"], d["N"])
    assert np.array_equal(A.ptr, p) and np.array_equal(A.col, c) and np.array_equal(A.val, v)
    assert A.isSymmetric == d["is_symmetric"]


@pytest.mark.parametrize("name", PRODUCT_CASES)
def test_product_reader_matches_oracle_reader(name):
    d, *_ = load_golden(name)
    for f in [d["A"]] + ([d["B"]] if d["B"] else []):
        A = mhspgemm.CSR()
        assert mhspgemm.readMtxFile(A, str(GOLDEN / f)) == 0
        M, N, p, c, v, s = orc.read_mtx(GOLDEN / f)
        assert (A.M, A.N) == (M, N)
        assert np.array_equal(A.ptr, p) and np.array_equal(A.col, c)
        assert np.array_equal(A.val.view(np.uint64), v.view(np.uint64))


def test_product_reader_large_parallel_parse(tmp_path):
    # > 1 MiB body: exercises the chunked parallel tokenizer; compared with the oracle reader
    rng = np.random.default_rng(1)
    M, N, nz = 5000, 4000, 120_000
    r = rng.integers(1, M + 1, nz)
    c = rng.integers(1, N + 1, nz)
    v = rng.standard_normal(nz)
    lines = ["%%MatrixMarket matrix coordinate real symmetric", "% big", f"{M} {N} {nz}"]
    lines += [f"{a} {b} {float(x)!r}" for a, b, x in zip(r, c, v)]
    f = tmp_path / "big.mtx"
    f.write_text("\n".join(lines) + "\n")
    A = mhspgemm.CSR()
    assert mhspgemm.readMtxFile(A, str(f)) == 0
    M2, N2, p, col, val, _ = orc.read_mtx(f)
    assert np.array_equal(A.ptr, p) and np.array_equal(A.col, col) and np.array_equal(A.val, val)


def test_binary_csr_cache(tmp_path):
    # the first cached read parses the text and writes <file>.mhscsr; the
    # second reads the cache (bit-identical); rewriting the .mtx invalidates it; a
    # corrupt cache is refused and re-parsed from the text.
    import os
    rng = np.random.default_rng(3)
    M, nz = 300, 2000
    lines = ["%%MatrixMarket matrix coordinate real symmetric", f"{M} {M} {nz}"]
    lines += [f"{a} {b} {float(x)!r}" for a, b, x in
              zip(rng.integers(1, M + 1, nz), rng.integers(1, M + 1, nz), rng.standard_normal(nz))]
    f = tmp_path / "m.mtx"
    f.write_text("\n".join(lines) + "\n")
    ref = mhspgemm.CSR()
    assert mhspgemm.readMtxFile(ref, str(f)) == 0

    def read():
        A = mhspgemm.CSR()
        assert mhspgemm.readMtxFile(A, str(f), cache=True) == 0
        assert (A.M, A.N, A.nnz, A.isSymmetric) == (ref.M, ref.N, ref.nnz, ref.isSymmetric)
        assert np.array_equal(A.ptr, ref.ptr) and np.array_equal(A.col, ref.col)
        assert np.array_equal(A.val.view(np.uint64), ref.val.view(np.uint64))
        return mhspgemm.readMtxFile.last_from_cache

    cache = tmp_path / "m.mtx.mhscsr"
    assert read() is False and cache.exists()
    assert read() is True
    # a changed .mtx (new mtime) is re-parsed, never served from the old cache
    st = os.stat(f)
    os.utime(f, ns=(st.st_atime_ns, st.st_mtime_ns + 10**9))
    assert read() is False
    assert read() is True
    # truncated / corrupt caches are refused by the binary reader, the text is parsed again
    data = cache.read_bytes()
    cache.write_bytes(data[: len(data) - 8])
    assert read() is False
    blob = bytearray(cache.read_bytes())
    col_off = 64 + 4 * (M + 1)
    blob[col_off:col_off + 4] = np.int32(M + 5).tobytes()  # column out of range
    cache.write_bytes(bytes(blob))
    h = _lib.mhs_host_csr()
    assert _lib.lib().mhs_read_csr_bin(str(cache).encode(), ctypes.byref(h), None, None) == _lib.MHS_ERR_IO
    assert read() is False
    # a cache directory instead of the file's own
    d = tmp_path / "cachedir"
    A = mhspgemm.CSR()
    assert mhspgemm.readMtxFile(A, str(f), cache=str(d)) == 0 and (d / "m.mtx.mhscsr").exists()
    assert mhspgemm.readMtxFile(A, str(f), cache=str(d)) == 0 and mhspgemm.readMtxFile.last_from_cache
    assert np.array_equal(A.col, ref.col)


def test_reader_errors(tmp_path):
    A = mhspgemm.CSR()
    assert mhspgemm.readMtxFile(A, str(tmp_path / "nope.mtx")) == -1
    bad = tmp_path / "bad.mtx"
    bad.write_text("%%MatrixMarket matrix coordinate real general\n2 2 3\n1 1 1.0\n")
    assert mhspgemm.readMtxFile(A, str(bad)) == -1  # truncated body
    oob = tmp_path / "oob.mtx"
    oob.write_text("%%MatrixMarket matrix coordinate real general\n2 2 1\n3 1 1.0\n")
    assert mhspgemm.readMtxFile(A, str(oob)) == -1


def test_flop_count_matches_reference_rule():
    A = synth.cage4_like()
    assert mhspgemm.flop_count(A, A) == orc.flop(A.col, A.ptr) == mhspgemm.flop_count_np(A.col, A.ptr)


def test_timing_gettotal_excludes_mask_formation():
    t = mhspgemm.Timing(mem_alloc=1, Form_mask_matrix_B=100, Calculate_C_nnz=2, Malloc_C_col_val=3,
                        Numeric=4, symbolic_binning=5, numeric_binning=6)
    assert t.getTotal() == 21
    t2 = mhspgemm.Timing()
    t2 += t
    t2 += t
    t2 /= 2
    assert t2.getTotal() == 21 and t2.Form_mask_matrix_B == 100


def test_csr_eq_reference_semantics():
    p = np.array([0, 2, 3], np.int32)
    c = np.array([0, 1, 1], np.int32)
    v = np.array([1.0, 2.0, 3.0])
    A = mhspgemm.CSR(2, 2, p, c, v)
    B = mhspgemm.CSR(2, 2, p.copy(), c.copy(), v + 1e-10)
    assert A == B
    C = mhspgemm.CSR(2, 2, p.copy(), c.copy(), v + 1e-3)
    assert not (A == C)
    D = mhspgemm.CSR(2, 2, np.array([0, 1, 2], np.int32), c[:2].copy(), v[:2].copy())
    with pytest.raises(RuntimeError):
        A == D  # nnz mismatch throws in the reference


@pytest.mark.parametrize("name", ["cage4", "cant"])
def test_synthetic_generators_well_formed(name):
    A = synth.SYNTH[name]()
    assert A.ptr[0] == 0 and A.ptr[-1] == A.nnz == len(A.col) == len(A.val)
    assert np.all(np.diff(A.ptr) >= 0)
    rows = np.repeat(np.arange(A.M), np.diff(A.ptr))
    key = rows.astype(np.int64) * A.N + A.col
    assert np.all(np.diff(key) > 0), "rows sorted, no duplicates"
    assert A.col.min() >= 0 and A.col.max() < A.N
    assert np.all(A.val >= 0.1) and np.all(A.val < 1.0)
    if name == "cant":
        assert A.M == 62451
        assert 60 <= A.nnz / A.M <= 75


def test_cant_like_matches_published_shape():
    # the real cant: 62,451 rows, ~4.0M nnz, nnz(A*A) ~1.74e7, flop ~2.7e8
    A = synth.cant_like()
    Cp = orc.spgemm_symbolic(A.ptr, A.col, A.ptr, A.col, A.N)
    assert 1.6e7 < Cp[-1] < 1.9e7
    assert 2.5e8 < orc.flop(A.col, A.ptr) < 3.5e8


def test_cli_binary_built():
    cli = ROOT / "mh-spgemm_amd" / "bin" / "spgemm"
    assert cli.exists()
    out = subprocess.run([str(cli)], capture_output=True, text=True)
    assert "Usage" in out.stdout


def test_product_never_imports_oracle():
    # the product package must not reference the test oracle
    pkg = ROOT / "mh-spgemm_amd"
    for f in list(pkg.rglob("*.py")) + list(pkg.rglob("*.cpp")) + list(pkg.rglob("*.hip")) + list(pkg.rglob("*.hpp")):
        assert "oracle" not in f.read_text(errors="ignore").lower().replace("oracle-free", ""), f


def test_mtx_cache_env_words(tmp_path, monkeypatch):
    # MHS_MTX_CACHE=0/false/no/off (any case) means off -- never a directory named
    # after the word; 1/true/yes/on caches next to the file; anything else is a directory
    from mhspgemm.core import _cache_setting
    for off in (None, "", "0", "false", "No", "OFF"):
        assert _cache_setting(off) is False
    for on in ("1", "true", "YES", "on"):
        assert _cache_setting(on) is True
    assert _cache_setting(str(tmp_path / "c")) == str(tmp_path / "c")
    f = tmp_path / "m.mtx"
    f.write_text("%%MatrixMarket matrix coordinate real general\n2 2 2\n1 1 1.0\n2 2 2.0\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("MHS_MTX_CACHE", "false")
    A = mhspgemm.CSR()
    assert mhspgemm.readMtxFile(A, str(f)) == 0 and A.nnz == 2
    assert not (tmp_path / "false").exists() and not (tmp_path / "m.mtx.mhscsr").exists()


@pytest.mark.parametrize("name", ["cant", "webbase-1M", "mac_econ_fwd500", "scircuit", "cop20k_A", "cage15"])
def test_standin_stats(name):
    """every BASELINE config's stand-in against SURVEY §8's
    SuiteSparse statistics -- the counts synth.ACHIEVED records hold (nnz(C) recounted by the
    oracle below 2 M rows; cage15-like's 9.3e8 by tools/standin_stats.py), and each is within its
    synth.CALIBRATED_TOL of synth.TARGETS."""
    from mhspgemm import synth
    A = synth.SYNTH[name]()
    bl = np.diff(A.ptr).astype(np.int64)
    got = dict(M=A.M, nnzA=A.nnz, flop=int(bl[A.col].sum()), max_row=int(bl.max()))
    rec, tgt = synth.ACHIEVED[name], synth.TARGETS[name]
    for k, v in got.items():
        assert k not in rec or v == rec[k], (k, v, rec[k])
    if A.M < 2_000_000:
        Cp, _, _ = orc.spgemm(A.ptr, A.col, A.val, A.ptr, A.col, A.val, A.N)
        assert int(Cp[-1]) == rec["nnzC"]
    tol = synth.CALIBRATED_TOL[name]
    for k in ("nnzA", "flop", "nnzC", "max_row"):
        if k in tgt:
            assert abs(rec[k] / tgt[k] - 1) <= tol, (k, rec[k], tgt[k])
