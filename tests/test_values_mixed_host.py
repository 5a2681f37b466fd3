"""CPU tests of the mixed-precision values plans' surface (FP32 values summed in FP64): the two symbols
(mhs_values_plan_create_accum, mhs_values_plan_accum), their argument checks, which return before any HIP call, the
accum argument of ValuesPlan, and a mixed plan's launch plans against the float kernels' static LDS and slice guards
(csrc/mhs_valplan.hpp) on the host under sanitizers."""
import ctypes
import inspect
import subprocess
from pathlib import Path

import pytest

import mhspgemm
from mhspgemm import _lib, core

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = {"mhs_values_plan_create_accum": 10, "mhs_values_plan_accum": 2}


def test_mixed_symbols_declared_and_bound():
    L = _lib.lib()
    declared = _lib.declared_functions()
    for name, nargs in SYMBOLS.items():
        assert name in declared
        assert hasattr(L, name)
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    assert L.mhs_abi_version() == 10  # additions: the version stays
    assert (_lib.MHS_ACC_NATIVE, _lib.MHS_ACC_F64) == (0, 1)
    header = (ROOT / "include" / "mhspgemm.h").read_text()
    assert "typedef enum mhs_accum { MHS_ACC_NATIVE = 0, MHS_ACC_F64 = 1 } mhs_accum;" in header
    assert "typedef enum mhs_dtype { MHS_F64 = 0, MHS_F32 = 1 } mhs_dtype;" in header  # (no new dtype value)
    assert "#define MHS_ABI_VERSION 10" in header


def test_mixed_null_and_bad_accum_return_invalid_without_hip():
    L = _lib.lib()
    a = _lib.mhs_csr()
    plan = ctypes.c_void_p(0x5a5a)
    for accum in (_lib.MHS_ACC_NATIVE, _lib.MHS_ACC_F64, -1, 2, 7):
        for dtype in (_lib.MHS_F64, _lib.MHS_F32, 2):
            for width in (1, 2, 4, 3):
                for masked in (0, 1):
                    assert L.mhs_values_plan_create_accum(None, None, None, None, masked, 0, dtype, width, accum, None) == 3
                    assert L.mhs_values_plan_create_accum(None, ctypes.byref(a), ctypes.byref(a), ctypes.byref(a), masked, 0,
                                                          dtype, width, accum, ctypes.byref(plan)) == 3
    assert plan.value == 0x5a5a  # nothing written without a context
    acc = ctypes.c_int(-7)
    assert L.mhs_values_plan_accum(None, ctypes.byref(acc)) == 3 and acc.value == -7
    assert L.mhs_values_plan_accum(None, None) == 3
    assert L.mhs_values_plan_accum(ctypes.c_void_p(0), ctypes.byref(acc)) == 3 and acc.value == -7
    # (the checks that need a context -- a bad accum's message, the getter's values, the wrong-type refusal -- are in
    # tests/test_gpu_values_mixed.py::test_mixed_refusals)


def test_mixed_accum_argument_of_the_wrapper():
    import torch
    assert core.values_accum(None) is None
    assert core.values_accum("float64") == "float64" and core.values_accum("f64") == "float64"
    assert core.values_accum(torch.float64) == "float64"
    for bad in ("float32", "f32", "float16", "native", torch.float32, torch.float16, 1, 64, True):
        with pytest.raises(ValueError, match="accum"):
            core.values_accum(bad)
    # the constructor refuses both before it touches the tool or the library
    with pytest.raises(ValueError, match="accum"):
        mhspgemm.ValuesPlan(None, None, None, None, dtype="float32", accum="float16")
    for semiring in ("min_plus", "max_plus", "max_min"):
        with pytest.raises(ValueError, match="accum"):
            mhspgemm.ValuesPlan(None, None, None, None, dtype="float32", semiring=semiring, accum="float64")
        with pytest.raises(ValueError, match="accum"):
            mhspgemm.ValuesPlan(None, None, None, None, dtype="float32", semiring=semiring, accum=torch.float64)
    # a keyword of the constructor call, None by default; __init__'s own signature is as it was
    assert inspect.signature(type(mhspgemm.ValuesPlan).__call__).parameters["accum"].default is None
    assert list(inspect.signature(mhspgemm.ValuesPlan.__init__).parameters)[-1] == "semiring"


def test_mixed_plan_under_sanitizers(tmp_path):
    # a mixed plan's launch plans at sb = 8 W with a 4-byte value, the float backward's guards at 4 W against the
    # forward's at 8 W, the registered team launch: tests/valplan_mixed_check.cpp, HIP-free
    exe = tmp_path / "valplan_mixed_check"
    cc = subprocess.run(["c++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", str(ROOT / "tests" / "valplan_mixed_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "valplan mixed ok", run.stdout + run.stderr
