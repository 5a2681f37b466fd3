"""CPU tests of the values backward's surface (mhs_spgemm_values_grad, ValuesPlan.grad / .apply): the
symbol, its argument checks, which return before any HIP call, and the backward's launch plan
(plan_grad, csrc/mhs_valplan.hpp) on the host under sanitizers."""
import ctypes
import subprocess
from pathlib import Path

import mhspgemm
from mhspgemm import _lib

ROOT = Path(__file__).resolve().parent.parent


def test_grad_symbol_declared_and_bound():
    L = _lib.lib()
    assert "mhs_spgemm_values_grad" in _lib.declared_functions()
    assert hasattr(L, "mhs_spgemm_values_grad")
    assert L.mhs_spgemm_values_grad.restype is ctypes.c_int and len(L.mhs_spgemm_values_grad.argtypes) == 8
    assert L.mhs_abi_version() == 10  # an addition: the version stays


def test_grad_null_arguments_return_invalid_without_hip():
    L = _lib.lib()
    buf = (ctypes.c_double * 4)()
    p = ctypes.addressof(buf)
    ms = ctypes.c_double(-1.0)
    # no context, with everything else null or in place
    assert L.mhs_spgemm_values_grad(None, None, None, None, None, None, None, None) == 3
    assert L.mhs_spgemm_values_grad(None, None, p, p, p, p, p, ctypes.byref(ms)) == 3
    assert ms.value == -1.0
    # (the checks that need a context and a plan -- null plan, null dCval, no output, a missing input -- are in
    # tests/test_gpu_values_grad.py::test_grad_argument_checks)
    assert "mhs_ctx_fence_default_stream" in _lib.declared_functions()
    assert L.mhs_ctx_fence_default_stream(None, 0) == 3 and L.mhs_ctx_fence_default_stream(None, 1) == 3


def test_grad_plan_under_sanitizers(tmp_path):
    # plan_grad is HIP-free: tests/gradplan_check.cpp checks its launches against literals, the dot rows of
    # a masked plan routed to the global-form kernel among them, and that plan_values returns what it did
    exe = tmp_path / "gradplan_check"
    cc = subprocess.run(["c++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", str(ROOT / "tests" / "gradplan_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "gradplan ok", run.stdout + run.stderr


def test_grad_methods_exist():
    for m in ("grad", "apply"):
        assert callable(getattr(mhspgemm.ValuesPlan, m))
