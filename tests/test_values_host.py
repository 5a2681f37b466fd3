"""CPU tests of the values-only SpGEMM surface: the row classes and the launch plan
(csrc/mhs_valplan.hpp) on the host under sanitizers, and the argument checks of the new
entry points, which return before any HIP call."""
import ctypes
import subprocess
from pathlib import Path

import mhspgemm
from mhspgemm import _lib

ROOT = Path(__file__).resolve().parent.parent


def test_values_plan_under_sanitizers(tmp_path):
    # the classes, their LDS needs and plan_values are HIP-free: tests/valplan_check.cpp checks rows
    # one below, at and one above every threshold and every class's launch against literals
    exe = tmp_path / "valplan_check"
    cc = subprocess.run(["c++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", str(ROOT / "tests" / "valplan_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "valplan ok", run.stdout + run.stderr


def test_values_symbols_declared_and_bound():
    L = _lib.lib()
    names = {"mhs_values_plan_create", "mhs_spgemm_values", "mhs_values_plan_info", "mhs_values_plan_destroy"}
    assert names <= set(_lib.declared_functions())
    assert all(hasattr(L, n) for n in names)
    assert L.mhs_abi_version() == 10  # additions only: the version stays


def test_values_null_arguments_return_invalid_without_hip():
    L = _lib.lib()
    plan = ctypes.c_void_p()
    a = _lib.mhs_csr()
    assert L.mhs_values_plan_create(None, ctypes.byref(a), ctypes.byref(a), ctypes.byref(a), ctypes.byref(plan)) == 3
    assert not plan.value
    assert L.mhs_values_plan_create(None, None, None, None, None) == 3
    assert L.mhs_spgemm_values(None, None, None, None, None, None) == 3
    info = _lib.mhs_values_info()
    assert L.mhs_values_plan_info(None, ctypes.byref(info)) == 3
    L.mhs_values_plan_destroy(None, None)  # a no-op


def test_values_plan_exported():
    assert "ValuesPlan" in mhspgemm.__all__
    assert mhspgemm.ValuesPlan is mhspgemm.core.ValuesPlan
    for m in ("run", "info", "close"):
        assert callable(getattr(mhspgemm.ValuesPlan, m))
