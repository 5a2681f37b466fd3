"""CPU tests of the semiring subgradient's surface: the value-level rule (csrc/mhs_semiring.hpp: wins, share_a,
share_b) on the host under sanitizers, the two entry points declared and bound, their argument checks, which return
before any HIP call, and the Python methods' signatures."""
import ctypes
import inspect
import subprocess
from pathlib import Path

import mhspgemm
from mhspgemm import _lib

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("mhs_spgemm_values_subgrad", "mhs_spgemm_values_subgrad_f32")


def test_subgrad_rule_under_sanitizers(tmp_path):
    exe = tmp_path / "subgrad_check"
    cc = subprocess.run(["c++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", str(ROOT / "tests" / "subgrad_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "subgrad ok", run.stdout + run.stderr


def test_subgrad_symbols_declared_and_bound():
    L = _lib.lib()
    assert set(NAMES) <= set(_lib.declared_functions())
    for name in NAMES:
        fn = getattr(L, name)
        # ctx, plan, Aval, Bval, Cval, dCval, ties, dAval, dBval, ms
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 10, name
        assert fn.argtypes[-1] == ctypes.POINTER(ctypes.c_double)
    assert L.mhs_abi_version() == 10  # additions only: the version stays
    header = _lib.HEADER.read_text()
    assert "#define MHS_ABI_VERSION 10" in header
    for name, t in zip(NAMES, ("double", "float")):
        decl = header[header.index(f"int {name}("):]
        decl = " ".join(decl[:decl.index(";")].split())
        assert decl == (f"int {name}(mhs_ctx *ctx, mhs_values_plan *plan, const {t} *Aval, const {t} *Bval, const {t} *Cval, "
                        f"const {t} *dCval, int32_t *ties, {t} *dAval, {t} *dBval, double *ms)"), decl


def test_subgrad_bad_arguments_return_invalid_without_hip():
    L = _lib.lib()
    buf = (ctypes.c_double * 4)()
    x = ctypes.addressof(buf)
    for name in NAMES:
        fn = getattr(L, name)
        assert fn(None, None, None, None, None, None, None, None, None, None) == 3  # everything NULL
        assert fn(None, None, x, x, x, x, x, x, x, None) == 3  # a NULL ctx and plan beside arrays: nothing is touched
        ms = ctypes.c_double(-7.0)
        assert fn(None, None, x, x, x, x, x, None, None, ctypes.byref(ms)) == 3 and ms.value == -7.0
    assert all(v == 0.0 for v in buf)
    # the four backward entry points still refuse without a context
    assert L.mhs_spgemm_values_grad(None, None, None, None, None, None, None, None) == 3
    assert L.mhs_spgemm_values_grad_f32(None, None, None, None, None, None, None, None) == 3


def test_values_plan_has_subgrad_methods():
    sig = inspect.signature(mhspgemm.ValuesPlan.subgrad)
    assert list(sig.parameters) == ["self", "dC", "Cval", "Aval", "Bval", "need_A", "need_B", "out_A", "out_B", "ties", "timed"]
    p = sig.parameters
    assert p["need_A"].default is True and p["need_B"].default is True and p["timed"].default is False
    assert p["out_A"].default is None and p["out_B"].default is None and p["ties"].default is None
    for name in ("dC", "Cval", "Aval", "Bval"):  # the winner test reads all four: none has a default
        assert p[name].default is inspect.Parameter.empty
    sig = inspect.signature(mhspgemm.ValuesPlan.apply_subgrad)
    assert list(sig.parameters) == ["self", "Aval", "Bval"]
    assert "subgrad" in mhspgemm.ValuesPlan.__doc__ and "apply_subgrad" in mhspgemm.ValuesPlan.__doc__
    # the existing backward methods keep their signatures
    assert list(inspect.signature(mhspgemm.ValuesPlan.grad).parameters)[:4] == ["self", "dC", "Aval", "Bval"]
    assert list(inspect.signature(mhspgemm.ValuesPlan.apply).parameters) == ["self", "Aval", "Bval"]
