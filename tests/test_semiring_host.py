"""CPU tests of the semiring values plans' surface: the value-level part of the kernels' policy
(csrc/mhs_semiring.hpp) on the host under sanitizers, the two new entry points declared and bound, their argument
checks, which return before any HIP call, and the Python mirror's argument."""
import ctypes
import inspect
import subprocess
from pathlib import Path

import pytest

import mhspgemm
from mhspgemm import _lib

ROOT = Path(__file__).resolve().parent.parent


def test_semiring_policy_under_sanitizers(tmp_path):
    exe = tmp_path / "semiring_check"
    cc = subprocess.run(["c++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", str(ROOT / "tests" / "semiring_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "semiring ok", run.stdout + run.stderr


def test_semiring_symbols_declared_and_bound():
    L = _lib.lib()
    names = {"mhs_values_plan_create_semiring", "mhs_values_plan_semiring"}
    assert names <= set(_lib.declared_functions())
    assert all(hasattr(L, n) for n in names)
    assert L.mhs_values_plan_create_semiring.restype is ctypes.c_int and len(L.mhs_values_plan_create_semiring.argtypes) == 9
    assert L.mhs_values_plan_semiring.restype is ctypes.c_int and len(L.mhs_values_plan_semiring.argtypes) == 2
    assert L.mhs_abi_version() == 10  # additions only: the version stays
    assert (_lib.MHS_SR_PLUS_TIMES, _lib.MHS_SR_MIN_PLUS, _lib.MHS_SR_MAX_PLUS, _lib.MHS_SR_MAX_MIN) == (0, 1, 2, 3)
    header = _lib.HEADER.read_text()
    assert "MHS_SR_PLUS_TIMES = 0, MHS_SR_MIN_PLUS = 1, MHS_SR_MAX_PLUS = 2, MHS_SR_MAX_MIN = 3" in header
    assert "#define MHS_ABI_VERSION 10" in header


def test_semiring_bad_arguments_return_invalid_without_hip():
    L = _lib.lib()
    plan = ctypes.c_void_p()
    a = _lib.mhs_csr()
    ra = ctypes.byref(a)
    for semiring in (-1, 0, 1, 2, 3, 4):
        for dtype in (_lib.MHS_F64, _lib.MHS_F32):
            assert L.mhs_values_plan_create_semiring(None, ra, ra, ra, 0, 0, dtype, semiring, ctypes.byref(plan)) == 3  # a NULL ctx
            assert not plan.value
    assert L.mhs_values_plan_create_semiring(None, None, None, None, 0, 0, 0, 1, None) == 3
    sr = ctypes.c_int(-7)
    assert L.mhs_values_plan_semiring(None, ctypes.byref(sr)) == 3 and sr.value == -7
    assert L.mhs_values_plan_semiring(None, None) == 3


def test_values_plan_accepts_semiring():
    sig = inspect.signature(mhspgemm.ValuesPlan.__init__)
    assert sig.parameters["semiring"].default == "plus_times"
    assert list(sig.parameters)[-1] == "semiring"  # a trailing argument: positional callers keep their meaning
    assert mhspgemm.core.SEMIRINGS == {"plus_times": 0, "min_plus": 1, "max_plus": 2, "max_min": 3}
    assert isinstance(mhspgemm.ValuesPlan.semiring, property)
    for name in ("tropical", "MIN_PLUS", 1, None):  # refused before the library is called: nothing else is looked at
        with pytest.raises(ValueError, match="semiring"):
            mhspgemm.ValuesPlan(None, None, None, None, semiring=name)
    for width in (2, 4):  # a semiring plan has width 1
        with pytest.raises(ValueError, match="width"):
            mhspgemm.ValuesPlan(None, None, None, None, width=width, semiring="max_min")
