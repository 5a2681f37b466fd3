"""CPU tests of the batched values backward's surface (mhs_spgemm_values_grad_batched / _f32,
ValuesPlan.grad_batched / .apply_batched): the two symbols, the refusals that need no context, which return before
any HIP call, the shape validation of the wrapper with a library that must not be called, and the backward's launch
plan as a function of the sum bytes (plan_grad(counts, sb), csrc/mhs_valplan.hpp) on the host under sanitizers."""
import ctypes
import inspect
import subprocess
from pathlib import Path

import pytest

import mhspgemm
from mhspgemm import _lib, core

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("mhs_spgemm_values_grad_batched", "mhs_spgemm_values_grad_batched_f32")


def test_grad_batched_symbols_declared_and_bound():
    L = _lib.lib()
    declared = _lib.declared_functions()
    for name in SYMBOLS:
        assert name in declared
        assert hasattr(L, name)
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14
        assert [fn.argtypes[i] for i in (4, 6, 8, 10, 12)] == [ctypes.c_int64] * 5  # the five strides are 64-bit
        assert fn.argtypes[2] is ctypes.c_int
    assert L.mhs_abi_version() == 10  # additions: the version stays
    assert "#define MHS_ABI_VERSION 10" in (ROOT / "include" / "mhspgemm.h").read_text()
    # the unbatched entry points are what they were
    assert len(L.mhs_spgemm_values_grad.argtypes) == 8 and len(L.mhs_spgemm_values_grad_f32.argtypes) == 8


def test_grad_batched_refusals_without_a_context_write_nothing():
    L = _lib.lib()
    buf = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    fbuf = (ctypes.c_float * 4)(7.0, 7.0, 7.0, 7.0)
    ms = ctypes.c_double(-1.0)
    plan = ctypes.c_void_p(0x5a5a)  # (never dereferenced: the context is looked at first)
    for fn, b in ((L.mhs_spgemm_values_grad_batched, buf), (L.mhs_spgemm_values_grad_batched_f32, fbuf)):
        p = ctypes.addressof(b)
        assert fn(None, None, 1, None, 0, None, 0, None, 0, None, 0, None, 0, None) == 3
        for nb in (-1, 0, 1, 2, 5):
            for stride in (-3, 0, 1, 4, 1 << 40):
                assert fn(None, None, nb, p, stride, p, stride, p, stride, p, stride, p, stride, ctypes.byref(ms)) == 3
                assert fn(None, plan, nb, p, stride, p, stride, p, stride, p, stride, p, stride, ctypes.byref(ms)) == 3
                assert fn(None, plan, nb, None, stride, p, stride, p, stride, p, stride, None, stride, ctypes.byref(ms)) == 3
    assert ms.value == -1.0 and list(buf) == [7.0] * 4 and list(fbuf) == [7.0] * 4
    # (the refusals that need a context and a plan are in tests/test_gpu_values_grad_batched.py)


class _Untouchable:
    """Stands for the tool: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper touched .{name} before it refused the argument")


def test_grad_batched_signatures():
    sig = inspect.signature(mhspgemm.ValuesPlan.grad_batched)
    assert list(sig.parameters) == ["self", "dC", "Aval", "Bval", "need_A", "need_B", "out_A", "out_B", "timed"]
    assert [sig.parameters[k].default for k in ("need_A", "need_B", "out_A", "out_B", "timed")] == [True, True, None, None, False]
    assert list(inspect.signature(mhspgemm.ValuesPlan.apply_batched).parameters) == ["self", "Aval", "Bval"]
    # what was there stays as it was
    assert list(inspect.signature(mhspgemm.ValuesPlan.run_batched).parameters) == ["self", "Aval", "Bval", "out", "timed"]
    assert list(inspect.signature(mhspgemm.ValuesPlan.grad).parameters) == ["self", "dC", "Aval", "Bval", "need_A", "need_B",
                                                                            "out_A", "out_B", "timed"]
    assert list(inspect.signature(mhspgemm.ValuesPlan.apply).parameters) == ["self", "Aval", "Bval"]


def test_grad_batched_shapes_are_refused_by_the_wrapper(monkeypatch):
    import torch

    class NoLib:
        """The library as grad_batched may see it while it validates: present, never called."""

        def __getattr__(self, name):
            def call(*a):
                raise AssertionError(f"{name} called: the shapes were to be refused first")
            return call

    monkeypatch.setattr(core.L, "lib", lambda: NoLib())
    plan = object.__new__(mhspgemm.ValuesPlan)  # (no library call: the fields grad_batched's validation reads)
    plan.plan, plan.tool, plan._pad = ctypes.c_void_p(1), _Untouchable(), None
    plan.dtype_name, plan.f32, plan.width = "float64", False, 2
    plan.nnzA, plan.nnzB, plan.nnzC = 5, 7, 9
    f64 = torch.float64
    try:
        G, A2, B2 = torch.zeros(3, 9, dtype=f64), torch.zeros(3, 5, dtype=f64), torch.zeros(3, 7, dtype=f64)
        cases = [
            (dict(dC=torch.zeros(3, 9, dtype=torch.float32), Aval=A2, Bval=B2), "dC"),   # the other type
            (dict(dC=torch.zeros(9, dtype=f64), Aval=A2, Bval=B2), "dC"),                # a cotangent is never shared
            (dict(dC=torch.zeros(3, 8, dtype=f64), Aval=A2, Bval=B2), "dC"),             # not nnz(C) entries
            (dict(dC=torch.zeros(3, 18, dtype=f64)[:, ::2], Aval=A2, Bval=B2), "dC"),    # inner stride 2
            (dict(dC=torch.zeros(9, 3, dtype=f64).t(), Aval=A2, Bval=B2), "dC"),         # row stride 1 < nnz
            (dict(dC=[0.0] * 9, Aval=A2, Bval=B2), "dC"),                                # no tensor
            (dict(dC=G, Aval=torch.zeros(3, 6, dtype=f64), Bval=B2), "Aval"),
            (dict(dC=G, Aval=torch.zeros(2, 3, 5, dtype=f64), Bval=B2), "Aval"),
            (dict(dC=G, Aval=A2, Bval=torch.zeros(3, 7, dtype=torch.float32)), "Bval"),
            (dict(dC=G, Aval=torch.zeros(4, 5, dtype=f64), Bval=B2), "value sets"),      # nb 4 against dC's 3
            (dict(dC=G, Aval=A2, Bval=torch.zeros(2, 7, dtype=f64)), "value sets"),
            (dict(dC=G, Aval=None, Bval=B2), "Aval"),                                    # needed for dB
            (dict(dC=G, Aval=A2, Bval=None), "Bval"),                                    # needed for dA
            (dict(dC=G, Aval=A2, Bval=B2, out_A=torch.zeros(5, dtype=f64)), "out_A"),    # gradients come back per set
            (dict(dC=G, Aval=A2, Bval=B2, out_A=torch.zeros(2, 5, dtype=f64)), "value sets"),
            (dict(dC=G, Aval=A2, Bval=B2, out_B=torch.zeros(3, 8, dtype=f64)), "out_B"),
            (dict(dC=G, Aval=A2, Bval=B2, out_B=torch.zeros(3, 7, dtype=torch.float32)), "out_B"),
            (dict(dC=G, Aval=A2, Bval=B2, need_A=False, need_B=False), "need_A or need_B"),
            (dict(dC=G, Aval=A2, Bval=B2), "device"),                                    # host tensors
            (dict(dC=G, Aval=torch.zeros(5, dtype=f64), Bval=torch.zeros(7, dtype=f64)), "device"),  # shared, host
        ]
        for kw, what in cases:
            with pytest.raises(ValueError, match=what):
                plan.grad_batched(**kw)
        # a side that is not asked for does not have its operand looked at
        with pytest.raises(ValueError, match="device"):
            plan.grad_batched(G, None, B2, need_B=False)
        with pytest.raises(ValueError, match="device"):
            plan.grad_batched(G, A2, None, need_A=False)
    finally:
        plan.plan = ctypes.c_void_p()  # (nothing for __del__ to close)


def test_grad_batched_plan_under_sanitizers(tmp_path):
    # plan_grad(counts, sb) at sb = 16 and 32 against literals, the dot rows routed to the global-form kernel with
    # the list unchanged, static + dynamic LDS within a workgroup for every launch, type and width, the sb = 32
    # team launch of 73,728 B, and sb = 4 / 8 against what gradplan_check.cpp holds: HIP-free
    exe = tmp_path / "gradplan_batched_check"
    cc = subprocess.run(["c++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", str(ROOT / "tests" / "gradplan_batched_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "gradplan batched ok", run.stdout + run.stderr
