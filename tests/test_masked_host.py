"""CPU tests of the masked product's surface: the masked row rule and the dot launch
(csrc/mhs_valplan.hpp) on the host under sanitizers, and the argument checks of the two new entry
points, which return before any HIP call."""
import ctypes
import inspect
import subprocess
from pathlib import Path

import pytest

import mhspgemm
from mhspgemm import _lib

ROOT = Path(__file__).resolve().parent.parent


def test_masked_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "maskplan_check"
    cc = subprocess.run(["c++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", str(ROOT / "tests" / "maskplan_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "maskplan ok", run.stdout + run.stderr


def test_masked_symbols_declared_and_bound():
    L = _lib.lib()
    names = {"mhs_values_plan_create_masked", "mhs_values_plan_kept"}
    assert names <= set(_lib.declared_functions())
    assert all(hasattr(L, n) for n in names)
    assert L.mhs_values_plan_create_masked.restype is ctypes.c_int and len(L.mhs_values_plan_create_masked.argtypes) == 6
    assert len(L.mhs_values_plan_kept.argtypes) == 2
    assert L.mhs_abi_version() == 10  # additions only: the version stays
    assert (_lib.MHS_MASK_AUTO, _lib.MHS_MASK_PRODUCT, _lib.MHS_MASK_DOT) == (0, 1, 2)
    header = _lib.HEADER.read_text()
    assert "MHS_MASK_AUTO = 0, MHS_MASK_PRODUCT = 1, MHS_MASK_DOT = 2" in header and "#define MHS_ABI_VERSION 10" in header


def test_masked_bad_arguments_return_invalid_without_hip():
    L = _lib.lib()
    plan = ctypes.c_void_p()
    a = _lib.mhs_csr()
    ra = ctypes.byref(a)
    for form in (0, 1, 2, 3):
        assert L.mhs_values_plan_create_masked(None, ra, ra, ra, form, ctypes.byref(plan)) == 3  # a NULL ctx
        assert not plan.value
    assert L.mhs_values_plan_create_masked(None, None, None, None, 0, None) == 3
    kept = ctypes.c_int64(-5)
    assert L.mhs_values_plan_kept(None, ctypes.byref(kept)) == 3 and kept.value == -5
    assert L.mhs_values_plan_kept(None, None) == 3


def test_values_plan_accepts_masked_and_form():
    sig = inspect.signature(mhspgemm.ValuesPlan.__init__)
    assert sig.parameters["masked"].default is False and sig.parameters["form"].default == "auto"
    assert mhspgemm.core.VALUES_CLASSES[7] == "dot" and len(mhspgemm.core.VALUES_CLASSES) == 8
    assert mhspgemm.core.MASK_FORMS == {"auto": 0, "product": 1, "dot": 2}
    with pytest.raises(ValueError):  # a form by an unknown name is refused before the library is called
        mhspgemm.ValuesPlan(None, None, None, None, masked=True, form="inner")
