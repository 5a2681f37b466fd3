"""CPU tests of the semiring witness's surface: the two entry points declared in the header, exported by the built
library and bound, the ABI version unchanged, the argument checks that return before any HIP call, and the Python
methods' signatures."""
import ctypes
import inspect

import mhspgemm
from mhspgemm import _lib

NAMES = ("mhs_spgemm_values_witness", "mhs_spgemm_values_witness_f32")


def test_witness_header_declares_both_entry_points():
    header = _lib.HEADER.read_text()
    assert set(NAMES) <= set(_lib.declared_functions())
    for name, t in zip(NAMES, ("double", "float")):
        decl = header[header.index(f"int {name}("):]
        decl = " ".join(decl[:decl.index(";")].split())
        assert decl == (f"int {name}(mhs_ctx *ctx, mhs_values_plan *plan, const {t} *Aval, const {t} *Bval, const {t} *Cval, "
                        f"int32_t *wit, double *ms)"), decl
    # its own section, after the subgradient's, with the rule by reference
    assert header.index("semiring subgradients") < header.index("semiring witnesses") < header.index(f"int {NAMES[0]}(")


def test_witness_library_exports_both_entry_points():
    L = ctypes.CDLL(str(_lib.lib_path()))  # the built file itself, not the bound object
    for name in NAMES:
        assert hasattr(L, name), name
    B = _lib.lib()
    for name in NAMES:
        fn = getattr(B, name)
        # ctx, plan, Aval, Bval, Cval, wit, ms
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 7, name
        assert fn.argtypes[-1] == ctypes.POINTER(ctypes.c_double)


def test_witness_abi_version_stays():
    assert _lib.lib().mhs_abi_version() == 10  # additions only
    assert "#define MHS_ABI_VERSION 10" in _lib.HEADER.read_text()


def test_witness_null_ctx_returns_invalid_without_hip():
    L = _lib.lib()
    buf = (ctypes.c_double * 4)()
    x = ctypes.addressof(buf)
    for name in NAMES:
        fn = getattr(L, name)
        assert fn(None, None, None, None, None, None, None) == _lib.MHS_ERR_INVALID == 3  # everything NULL
        assert fn(None, None, x, x, x, x, None) == 3  # a NULL ctx and plan beside arrays: nothing is touched
        ms = ctypes.c_double(-7.0)
        assert fn(None, None, x, x, x, x, ctypes.byref(ms)) == 3 and ms.value == -7.0
    assert all(v == 0.0 for v in buf)


def test_values_plan_has_witness_methods():
    sig = inspect.signature(mhspgemm.ValuesPlan.witness)
    assert list(sig.parameters) == ["self", "Cval", "Aval", "Bval", "out", "timed"]
    p = sig.parameters
    assert p["out"].default is None and p["timed"].default is False
    for name in ("Cval", "Aval", "Bval"):  # the winner test reads all three: none has a default
        assert p[name].default is inspect.Parameter.empty
    assert list(inspect.signature(mhspgemm.ValuesPlan.run_arg).parameters) == ["self", "Aval", "Bval"]
    assert "witness" in mhspgemm.ValuesPlan.__doc__ and "run_arg" in mhspgemm.ValuesPlan.__doc__
    # the subgradient's methods keep their signatures
    assert list(inspect.signature(mhspgemm.ValuesPlan.subgrad).parameters)[:5] == ["self", "dC", "Cval", "Aval", "Bval"]
