"""CPU tests of the batched values calls' surface: the four symbols (mhs_values_plan_create_batched,
mhs_values_plan_width, mhs_spgemm_values_batched, mhs_spgemm_values_batched_f32), the refusals that need no context,
which return before any HIP call, the width and shape validation of ValuesPlan, and the classes and launch plans as
a function of the sum bytes (csrc/mhs_valplan.hpp) on the host under sanitizers."""
import ctypes
import inspect
import subprocess
from pathlib import Path

import pytest

import mhspgemm
from mhspgemm import _lib, core

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = {"mhs_values_plan_create_batched": 9, "mhs_values_plan_width": 2, "mhs_spgemm_values_batched": 10,
           "mhs_spgemm_values_batched_f32": 10}


def test_batched_symbols_declared_and_bound():
    L = _lib.lib()
    declared = _lib.declared_functions()
    for name, nargs in SYMBOLS.items():
        assert name in declared
        assert hasattr(L, name)
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    for name in ("mhs_spgemm_values_batched", "mhs_spgemm_values_batched_f32"):  # the strides are 64-bit
        assert [getattr(L, name).argtypes[i] for i in (4, 6, 8)] == [ctypes.c_int64] * 3
    assert L.mhs_abi_version() == 10  # additions: the version stays
    header = (ROOT / "include" / "mhspgemm.h").read_text()
    assert "#define MHS_ABI_VERSION 10" in header
    assert "#define MHS_VAL_WIDTH_MAX 4" in header and _lib.MHS_VAL_WIDTH_MAX == 4


def test_batched_refusals_without_a_context_write_nothing():
    L = _lib.lib()
    buf = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    fbuf = (ctypes.c_float * 4)(7.0, 7.0, 7.0, 7.0)
    ms = ctypes.c_double(-1.0)
    for fn, b in ((L.mhs_spgemm_values_batched, buf), (L.mhs_spgemm_values_batched_f32, fbuf)):
        p = ctypes.addressof(b)
        assert fn(None, None, 1, None, 0, None, 0, None, 0, None) == 3
        for nb in (-1, 0, 1, 2, 5):
            for stride in (-3, 0, 1, 4, 1 << 40):
                assert fn(None, None, nb, p, stride, p, stride, p, stride, ctypes.byref(ms)) == 3
    assert ms.value == -1.0 and list(buf) == [7.0] * 4 and list(fbuf) == [7.0] * 4
    a = _lib.mhs_csr()
    plan = ctypes.c_void_p(0x5a5a)
    for width in (1, 2, 4, 0, 3, 8, -1):
        for dtype in (_lib.MHS_F64, _lib.MHS_F32, 2):
            for masked in (0, 1):
                assert L.mhs_values_plan_create_batched(None, None, None, None, masked, 0, dtype, width, None) == 3
                assert L.mhs_values_plan_create_batched(None, ctypes.byref(a), ctypes.byref(a), ctypes.byref(a), masked, 0,
                                                        dtype, width, ctypes.byref(plan)) == 3
    assert plan.value == 0x5a5a  # nothing written without a context
    w = ctypes.c_int(-7)
    assert L.mhs_values_plan_width(None, ctypes.byref(w)) == 3 and w.value == -7
    assert L.mhs_values_plan_width(None, None) == 3
    # (the refusals that need a context and a plan -- a bad width, nb, strides, the wrong type, the backward --
    # are in tests/test_gpu_values_batched.py::test_batched_refusals)


class _Untouchable:
    """Stands for the tool and the operands: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper touched .{name} before it refused the argument")


def test_batched_bad_width_is_refused_by_the_wrapper():
    for ok in (1, 2, 4):
        assert core.values_width(ok) == ok
    for bad in (0, 3, 8, -1, 5, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="width"):
            core.values_width(bad)
        with pytest.raises(ValueError, match="width"):  # before the tool or the library is touched
            mhspgemm.ValuesPlan(_Untouchable(), _Untouchable(), _Untouchable(), _Untouchable(), width=bad)
    sig = inspect.signature(mhspgemm.ValuesPlan.__init__)
    assert sig.parameters["width"].default == 1
    assert core.VALUES_WIDTHS == (1, 2, 4)
    assert list(inspect.signature(mhspgemm.ValuesPlan.run_batched).parameters) == ["self", "Aval", "Bval", "out", "timed"]


def test_batched_shapes_are_refused_by_the_wrapper(monkeypatch):
    import torch

    class NoLib:
        """The library as run_batched may see it while it validates: present, never called."""

        def __getattr__(self, name):
            def call(*a):
                raise AssertionError(f"{name} called: the shapes were to be refused first")
            return call

    monkeypatch.setattr(core.L, "lib", lambda: NoLib())
    plan = object.__new__(mhspgemm.ValuesPlan)  # (no library call: the fields run_batched's validation reads)
    plan.plan, plan.tool = ctypes.c_void_p(1), _Untouchable()
    plan.dtype_name, plan.f32, plan.width = "float64", False, 2
    plan.nnzA, plan.nnzB, plan.nnzC = 5, 7, 9
    try:
        A2, B2 = torch.zeros(3, 5, dtype=torch.float64), torch.zeros(3, 7, dtype=torch.float64)
        cases = [
            (torch.zeros(3, 5, dtype=torch.float32), B2, None, "Aval"),   # the other type
            (torch.zeros(3, 6, dtype=torch.float64), B2, None, "Aval"),   # not nnz(A) entries
            (torch.zeros(6, dtype=torch.float64), B2, None, "Aval"),
            (torch.zeros(2, 3, 5, dtype=torch.float64), B2, None, "Aval"),  # neither [nb, nnz] nor [nnz]
            (A2, torch.zeros(3, 14, dtype=torch.float64)[:, ::2], None, "Bval"),  # inner stride 2
            (torch.zeros(5, 3, dtype=torch.float64).t(), B2, None, "Aval"),       # row stride 1 < nnz
            (A2, torch.zeros(4, 7, dtype=torch.float64), None, "value sets"),     # nb 3 against nb 4
            (A2, [0.0] * 7, None, "Bval"),                                        # no tensor
            (A2, B2, None, "device"),                                             # host tensors
        ]
        for Aval, Bval, out, what in cases:
            with pytest.raises(ValueError, match=what):
                plan.run_batched(Aval, Bval, out=out)
    finally:
        plan.plan = ctypes.c_void_p()  # (nothing for __del__ to close)


def test_batched_plan_under_sanitizers(tmp_path):
    # the caps, classes, slice guards, launch plans and LDS totals at sb = 16 and 32 against literals, and sb = 4
    # and 8 against the existing signatures: tests/valplan_batched_check.cpp, HIP-free
    exe = tmp_path / "valplan_batched_check"
    cc = subprocess.run(["c++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", str(ROOT / "tests" / "valplan_batched_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "valplan batched ok", run.stdout + run.stderr
