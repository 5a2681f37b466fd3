"""CPU tests of the soft semiring plans' surface: the value-level part of the smoothed kernels (csrc/mhs_smooth.hpp)
and a smoothed plan's launch plans (csrc/mhs_valplan.hpp at twice the value's bytes) on the host under sanitizers,
the four new entry points declared and bound, their argument checks, which return before any HIP call, and the
Python mirror's ``smooth=`` keyword."""
import ctypes
import inspect
import subprocess
from pathlib import Path

import pytest

import mhspgemm
from mhspgemm import _lib, core

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = {"mhs_values_plan_create_smooth": 10, "mhs_values_plan_smooth": 2, "mhs_spgemm_values_softgrad": 9,
           "mhs_spgemm_values_softgrad_f32": 9}


def build_and_run(tmp_path, name, says):
    exe = tmp_path / name
    cc = subprocess.run(["c++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", str(ROOT / "tests" / f"{name}.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == says, run.stdout + run.stderr


def test_smooth_policy_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "smooth_check", "smooth ok")


def test_smooth_plan_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "valplan_smooth_check", "valplan smooth ok")


def test_smooth_symbols_declared_and_bound():
    L = _lib.lib()
    declared = _lib.declared_functions()
    for name, nargs in SYMBOLS.items():
        assert name in declared
        assert hasattr(L, name)
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    assert L.mhs_abi_version() == 10  # additions only: the version stays
    assert (_lib.MHS_SMOOTH_NONE, _lib.MHS_SMOOTH_LSE) == (0, 1)
    header = _lib.HEADER.read_text()
    assert "typedef enum mhs_smooth { MHS_SMOOTH_NONE = 0, MHS_SMOOTH_LSE = 1 } mhs_smooth;" in header
    assert "MHS_SR_PLUS_TIMES = 0, MHS_SR_MIN_PLUS = 1, MHS_SR_MAX_PLUS = 2, MHS_SR_MAX_MIN = 3 } mhs_semiring;" in header
    assert "#define MHS_ABI_VERSION 10" in header


def test_smooth_bad_arguments_return_invalid_without_hip():
    L = _lib.lib()
    a = _lib.mhs_csr()
    ra = ctypes.byref(a)
    plan = ctypes.c_void_p(0x5a5a)
    for smooth in (-1, 0, 1, 2):
        for semiring in (-1, 0, 1, 2, 3, 4):
            for dtype in (_lib.MHS_F64, _lib.MHS_F32):
                assert L.mhs_values_plan_create_smooth(None, ra, ra, ra, 0, 0, dtype, semiring, smooth, ctypes.byref(plan)) == 3
                assert L.mhs_values_plan_create_smooth(None, None, None, None, 1, 0, dtype, semiring, smooth, None) == 3
    assert plan.value == 0x5a5a  # nothing written without a context
    sm = ctypes.c_int(-7)
    assert L.mhs_values_plan_smooth(None, ctypes.byref(sm)) == 3 and sm.value == -7
    assert L.mhs_values_plan_smooth(None, None) == 3
    for fn in (L.mhs_spgemm_values_softgrad, L.mhs_spgemm_values_softgrad_f32):
        assert fn(None, None, None, None, None, None, None, None, None) == 3  # a NULL ctx
    # (the checks that need a context -- the messages, the getter's values, the refusals by plan -- are in
    # tests/test_gpu_smooth.py::test_smooth_refusals)


def test_values_plan_accepts_smooth():
    assert core.values_smooth(None) is None and core.values_smooth("lse") == "lse"
    for bad in ("LSE", "softmax", "none", "", 1, True, 0.5):
        with pytest.raises(ValueError, match="smooth"):
            core.values_smooth(bad)
    # the constructor refuses before it touches the tool or the library
    for bad in ("LSE", "softmin", 1):
        with pytest.raises(ValueError, match="smooth"):
            mhspgemm.ValuesPlan(None, None, None, None, semiring="min_plus", smooth=bad)
    for semiring in ("plus_times", "max_min"):
        with pytest.raises(ValueError, match="smooth"):
            mhspgemm.ValuesPlan(None, None, None, None, semiring=semiring, smooth="lse")
    with pytest.raises(ValueError, match="smooth"):
        mhspgemm.ValuesPlan(None, None, None, None, smooth="lse")  # (the default semiring is plus_times)
    for semiring in ("min_plus", "max_plus"):
        with pytest.raises(ValueError, match="accum"):
            mhspgemm.ValuesPlan(None, None, None, None, dtype="float32", semiring=semiring, smooth="lse", accum="float64")
        with pytest.raises(ValueError, match="width"):
            mhspgemm.ValuesPlan(None, None, None, None, width=2, semiring=semiring, smooth="lse")
    # a keyword of the constructor call, None by default, next to accum; __init__'s own signature is as it was
    call = inspect.signature(type(mhspgemm.ValuesPlan).__call__).parameters
    assert call["smooth"].default is None and call["accum"].default is None
    sig = inspect.signature(mhspgemm.ValuesPlan.__init__)
    assert list(sig.parameters)[-1] == "semiring" and "smooth" not in sig.parameters
    assert mhspgemm.core.SEMIRINGS == {"plus_times": 0, "min_plus": 1, "max_plus": 2, "max_min": 3}
    for name in ("softgrad", "apply_soft"):
        assert callable(getattr(mhspgemm.ValuesPlan, name))
    assert list(inspect.signature(mhspgemm.ValuesPlan.softgrad).parameters) == [
        "self", "dC", "Cval", "Aval", "Bval", "need_A", "need_B", "out_A", "out_B", "timed"]
