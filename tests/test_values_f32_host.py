"""CPU tests of the FP32 values plans' surface: the four symbols (mhs_values_plan_create_typed,
mhs_values_plan_dtype, mhs_spgemm_values_f32, mhs_spgemm_values_grad_f32), their argument checks, which return
before any HIP call, the dtype argument of ValuesPlan, and the classes and launch plans as a function of the
value size (csrc/mhs_valplan.hpp) on the host under sanitizers."""
import ctypes
import inspect
import subprocess
from pathlib import Path

import pytest

import mhspgemm
from mhspgemm import _lib, core

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = {"mhs_values_plan_create_typed": 8, "mhs_values_plan_dtype": 2, "mhs_spgemm_values_f32": 6,
           "mhs_spgemm_values_grad_f32": 8}


def test_f32_symbols_declared_and_bound():
    L = _lib.lib()
    declared = _lib.declared_functions()
    for name, nargs in SYMBOLS.items():
        assert name in declared
        assert hasattr(L, name)
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    assert L.mhs_abi_version() == 10  # additions: the version stays
    assert (_lib.MHS_F64, _lib.MHS_F32) == (0, 1)
    header = (ROOT / "include" / "mhspgemm.h").read_text()
    assert "typedef enum mhs_dtype { MHS_F64 = 0, MHS_F32 = 1 } mhs_dtype;" in header
    assert "#define MHS_ABI_VERSION 10" in header


def test_f32_null_arguments_return_invalid_without_hip():
    L = _lib.lib()
    buf = (ctypes.c_float * 4)(7.0, 7.0, 7.0, 7.0)
    p = ctypes.addressof(buf)
    ms = ctypes.c_double(-1.0)
    # no context, with everything else null or in place
    assert L.mhs_spgemm_values_f32(None, None, None, None, None, None) == 3
    assert L.mhs_spgemm_values_f32(None, None, p, p, p, ctypes.byref(ms)) == 3
    assert L.mhs_spgemm_values_grad_f32(None, None, None, None, None, None, None, None) == 3
    assert L.mhs_spgemm_values_grad_f32(None, None, p, p, p, p, p, ctypes.byref(ms)) == 3
    assert ms.value == -1.0 and list(buf) == [7.0] * 4
    a = _lib.mhs_csr()
    plan = ctypes.c_void_p(0x5a5a)
    for dtype in (_lib.MHS_F64, _lib.MHS_F32, 2, -1):
        for masked in (0, 1):
            assert L.mhs_values_plan_create_typed(None, None, None, None, masked, 0, dtype, None) == 3
            assert L.mhs_values_plan_create_typed(None, ctypes.byref(a), ctypes.byref(a), ctypes.byref(a), masked, 0, dtype,
                                                  ctypes.byref(plan)) == 3
    assert plan.value == 0x5a5a  # nothing written without a context
    dt = ctypes.c_int(-7)
    assert L.mhs_values_plan_dtype(None, ctypes.byref(dt)) == 3 and dt.value == -7
    assert L.mhs_values_plan_dtype(None, None) == 3
    # (the checks that need a context and a plan -- a bad dtype, a call of the wrong type -- are in
    # tests/test_gpu_values_f32.py::test_f32_wrong_type_is_refused)


def test_f32_bad_dtype_is_refused_by_the_wrapper():
    assert core.values_dtype_name("float64") == "float64" and core.values_dtype_name("float32") == "float32"
    assert core.values_dtype_name("f32") == "float32" and core.values_dtype_name("f64") == "float64"
    import torch
    assert core.values_dtype_name(torch.float32) == "float32" and core.values_dtype_name(torch.float64) == "float64"
    for bad in ("float16", "bfloat16", torch.float16, torch.int32, 4, None):
        with pytest.raises(ValueError, match="dtype"):
            core.values_dtype_name(bad)
    # the constructor refuses it before it touches the tool or the library
    with pytest.raises(ValueError, match="dtype"):
        mhspgemm.ValuesPlan(None, None, None, None, dtype="float16")
    sig = inspect.signature(mhspgemm.ValuesPlan.__init__)
    assert sig.parameters["dtype"].default in ("float64", torch.float64)
    assert core.VALUES_DTYPES == {"float64": 0, "float32": 1}


def test_f32_plan_under_sanitizers(tmp_path):
    # the classes, caps, slice guards and both launch plans at vb = 4 against literals, and vb = 8 against
    # the signatures without vb: tests/valplan_f32_check.cpp, HIP-free
    exe = tmp_path / "valplan_f32_check"
    cc = subprocess.run(["c++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", str(ROOT / "tests" / "valplan_f32_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "valplan f32 ok", run.stdout + run.stderr
