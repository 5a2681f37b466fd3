"""Host-side mirror of the reference's SpGEMM interface, over the C-ABI.

Names, argument meaning and error behaviour follow the reference
(yyssys/MH-SpGEMM):

  * ``CSR``            inc/CSR.h:4-44, src/CSR.cu -- host arrays (numpy) plus device
                       arrays, ``H2D()``, ``D2H()``, ``==`` (src/CSR.cu:48-96: raises
                       on an nnz mismatch or more than 10 errors, like the C++ throws).
  * ``Timing``         inc/Timing.h, src/Timing.cpp -- the 7 phase fields, ``getTotal()``
                       (without Form_mask_matrix_B), ``print_step_time()``.
  * ``Tool``           inc/Tool.h -- here it owns the C-ABI context (stream, workspace).
  * ``MH_spgemm``      src/main.cu:12-72 -- C = A * B on device-resident A, B.
  * ``readMtxFile``    inc/mmio_read.h:34-159.

Device memory for A and B comes from PyTorch (HIP allocations on ``cuda:N``);
C is allocated by the library.  No torch type crosses the ABI: only pointers.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L


class MHSpGEMMError(RuntimeError):
    """A C-ABI call returned a non-zero mhs_status (the reference throws std::exception)."""

    def __init__(self, status: int, msg: str):
        super().__init__(f"{L.STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


def _check(ctx, rc: int, what: str):
    if rc != L.MHS_OK:
        msg = L.lib().mhs_last_error(ctx).decode() if ctx else what
        raise MHSpGEMMError(rc, f"{what}: {msg}")


def _torch():
    import torch
    return torch


# ----------------------------------------------------------------- context ---

class Tool:
    """The reference's Tool (inc/Tool.h): here the C-ABI context of one device."""

    def __init__(self, device: int = 0):
        self.device = device
        self.ctx = ctypes.c_void_p()
        _check(None, L.lib().mhs_ctx_create(ctypes.byref(self.ctx), device), "mhs_ctx_create")

    def set_stream(self, hip_stream: int | None):
        _check(self.ctx, L.lib().mhs_ctx_set_stream(self.ctx, hip_stream or None), "mhs_ctx_set_stream")

    def fence_default_stream(self, after: bool):
        """mhs_ctx_fence_default_stream: order the context stream against the device's default (null) stream,
        whose handle 0 ``set_stream`` cannot take (0 selects the context's own, non-blocking stream).
        ``after=False``, before a call: the context stream waits for what is queued on the null stream;
        ``after=True``, after it: the null stream waits for what is queued on the context stream."""
        _check(self.ctx, L.lib().mhs_ctx_fence_default_stream(self.ctx, 1 if after else 0), "mhs_ctx_fence_default_stream")

    def set_option(self, option: int, value: int):
        """mhs_ctx_set_option: MHS_OPT_SYNC (0: return once the numeric phase is
        queued) or MHS_OPT_NUMERIC_EVENTS (ring size of numeric-phase events)."""
        _check(self.ctx, L.lib().mhs_ctx_set_option(self.ctx, option, value), "mhs_ctx_set_option")

    def numeric_ms(self, n: int) -> list[float]:
        """Numeric-phase durations (ms) of the last n calls (hipEvents on the stream)."""
        buf = (ctypes.c_float * max(1, n))()
        k = L.lib().mhs_ctx_numeric_ms(self.ctx, buf, n)
        if k < 0:
            _check(self.ctx, -k, "mhs_ctx_numeric_ms")
        return [float(buf[i]) for i in range(k)]

    def probe_conflicts(self) -> int:
        """Hash probe conflicts since the last query (the reference's HASH_CONFLICT count,
        src/main.cu:68-71); needs the diagnostic library (MHS_LIB=.../libmhspgemm_probe.so)."""
        v = ctypes.c_uint64()
        _check(self.ctx, L.lib().mhs_probe_conflicts(self.ctx, ctypes.byref(v)), "mhs_probe_conflicts")
        return int(v.value)

    def chunked_calls(self) -> int:
        """Calls that ran row-chunked (the out-of-memory fallback)."""
        return int(L.lib().mhs_ctx_chunked_calls(self.ctx))

    STATS = {"chunked": 0, "split": 1, "sym_fork": 2, "nft": 3, "near": 4, "multi_stream": 5,
             "spec": 6, "spec_miss": 7, "spec_skipped": 8, "wide_offsets": 9, "poison_fills": 10}

    def stat(self, name: str) -> int:
        """Calls of this context that took a path (mhs_ctx_stat: 'split', 'sym_fork', 'nft',
        'near', 'multi_stream', 'chunked', 'spec', 'spec_miss', 'spec_skipped', 'wide_offsets'), and
        'poison_fills': the buffers a context created under MHS_POISON=<byte> has filled with that byte."""
        return int(L.lib().mhs_ctx_stat(self.ctx, self.STATS[name]))

    def hbm_peak(self, nbytes: int = 2 << 30, iters: int = 10) -> dict:
        """Measured HBM bandwidth of this device (GB/s): copy (read + write bytes), read,
        write streaming kernels over `nbytes` buffers (mhs_hbm_peak)."""
        out = (ctypes.c_double * 3)()
        _check(self.ctx, L.lib().mhs_hbm_peak(self.ctx, nbytes, iters, out), "mhs_hbm_peak")
        return {"copy_GBps": round(out[0], 1), "read_GBps": round(out[1], 1), "write_GBps": round(out[2], 1),
                "buffer_bytes": int(nbytes), "iters": int(iters)}

    def allocate(self, B=None, C=None):  # src/Tool.cu:4 -- workspace grows on demand
        return None

    def release(self):
        if self.ctx:
            L.lib().mhs_ctx_trim(self.ctx)

    def close(self):
        if self.ctx:
            L.lib().mhs_ctx_destroy(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class Timing:
    """Reference Timing (inc/Timing.h:3-20), ms; plus the e2e total and run stats."""
    mem_alloc: float = 0.0
    Form_mask_matrix_B: float = 0.0
    Calculate_C_nnz: float = 0.0
    Malloc_C_col_val: float = 0.0
    Numeric: float = 0.0
    symbolic_binning: float = 0.0
    numeric_binning: float = 0.0
    total_e2e: float = 0.0
    flop: int = 0
    nnzC: int = 0
    sym_bins: list = field(default_factory=lambda: [0] * 16)
    num_bins: list = field(default_factory=lambda: [0] * 16)

    PHASES = ("mem_alloc", "Form_mask_matrix_B", "Calculate_C_nnz", "Malloc_C_col_val",
              "Numeric", "symbolic_binning", "numeric_binning", "total_e2e")

    def getTotal(self) -> float:  # src/Timing.cpp:39-41: Form_mask_matrix_B excluded
        return (self.Calculate_C_nnz + self.Malloc_C_col_val + self.Numeric + self.symbolic_binning
                + self.numeric_binning + self.mem_alloc)

    def __iadd__(self, t: "Timing"):
        for k in self.PHASES:
            setattr(self, k, getattr(self, k) + getattr(t, k))
        return self

    def __itruediv__(self, x: float):
        for k in self.PHASES:
            setattr(self, k, getattr(self, k) / x)
        return self

    def print_step_time(self):
        print("  -------------time-------------")
        print(f"    mem_alloc: \t\t{self.mem_alloc:.3f}ms")
        print(f"    form_mask_matrix_B: {self.Form_mask_matrix_B:.3f}ms")
        print(f"    symbolic_binning: \t{self.symbolic_binning:.3f}ms")
        print(f"    calculate_C_nnz: \t{self.Calculate_C_nnz:.3f}ms")
        print(f"    malloc_C_col_val: \t{self.Malloc_C_col_val:.3f}ms")
        print(f"    numeric_binning: \t{self.numeric_binning:.3f}ms")
        print(f"    numeric: \t\t{self.Numeric:.3f}ms")
        print("  ------------------------------")

    @classmethod
    def from_c(cls, t: L.mhs_timing) -> "Timing":
        return cls(mem_alloc=t.mem_alloc, Form_mask_matrix_B=t.Form_mask_matrix_B,
                   Calculate_C_nnz=t.Calculate_C_nnz, Malloc_C_col_val=t.Malloc_C_col_val,
                   Numeric=t.Numeric, symbolic_binning=t.symbolic_binning,
                   numeric_binning=t.numeric_binning, total_e2e=t.total_e2e, flop=int(t.flop),
                   nnzC=int(t.nnzC), sym_bins=list(t.sym_bins), num_bins=list(t.num_bins))


# --------------------------------------------------------------------- CSR ---

class DeviceCSR:
    """A device CSR produced by the library (hipMalloc'ed); recycled into the
    context's output pool when released (the reference frees with cudaFree)."""

    def __init__(self, tool: Tool, c: L.mhs_csr):
        self.tool = tool
        self.c = c

    @property
    def M(self):
        return self.c.M

    @property
    def N(self):
        return self.c.N

    @property
    def nnz(self):
        return self.c.nnz

    def to_host(self):
        M, nnz = self.c.M, self.c.nnz
        ptr = np.empty(M + 1, np.int32)
        col = np.empty(nnz, np.int32)
        val = np.empty(nnz, np.float64)
        lib, ctx = L.lib(), self.tool.ctx
        _check(ctx, lib.mhs_memcpy(ctx, ptr.ctypes.data, self.c.ptr, ptr.nbytes, 1), "D2H ptr")
        if nnz:
            _check(ctx, lib.mhs_memcpy(ctx, col.ctypes.data, self.c.col, col.nbytes, 1), "D2H col")
            _check(ctx, lib.mhs_memcpy(ctx, val.ctypes.data, self.c.val, val.nbytes, 1), "D2H val")
        return ptr, col, val

    def to_torch(self, device=None):
        """Copy into torch tensors on the context's device (D2D)."""
        torch = _torch()
        dev = device or f"cuda:{self.tool.device}"
        ptr = torch.empty(self.c.M + 1, dtype=torch.int32, device=dev)
        col = torch.empty(self.c.nnz, dtype=torch.int32, device=dev)
        val = torch.empty(self.c.nnz, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        lib, ctx = L.lib(), self.tool.ctx
        _check(ctx, lib.mhs_memcpy(ctx, ptr.data_ptr(), self.c.ptr, 4 * (self.c.M + 1), 2), "D2D ptr")
        if self.c.nnz:
            _check(ctx, lib.mhs_memcpy(ctx, col.data_ptr(), self.c.col, 4 * self.c.nnz, 2), "D2D col")
            _check(ctx, lib.mhs_memcpy(ctx, val.data_ptr(), self.c.val, 8 * self.c.nnz, 2), "D2D val")
        return ptr, col, val

    def release(self):
        if self.c.ptr or self.c.col or self.c.val:
            if self.tool.ctx:
                L.lib().mhs_ctx_recycle(self.tool.ctx, ctypes.byref(self.c))
            else:
                L.lib().mhs_csr_free(ctypes.byref(self.c))

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class CSR:
    """Reference CSR (inc/CSR.h): host arrays ptr/col/val (numpy), device arrays
    d_ptr/d_col/d_val (torch tensors, or a DeviceCSR for library outputs)."""

    def __init__(self, M=0, N=0, ptr=None, col=None, val=None, isSymmetric=0):
        self.M, self.N = int(M), int(N)
        self.ptr = None if ptr is None else np.ascontiguousarray(ptr, dtype=np.int32)
        self.col = None if col is None else np.ascontiguousarray(col, dtype=np.int32)
        self.val = None if val is None else np.ascontiguousarray(val, dtype=np.float64)
        self.nnz = 0 if self.col is None else int(self.col.shape[0])
        self.isSymmetric = int(isSymmetric)
        self.d_ptr = self.d_col = self.d_val = None
        self.dev: DeviceCSR | None = None

    # --- reference methods -------------------------------------------------
    def alloc(self, r, c, n):
        self.M, self.N, self.nnz = r, c, n
        self.ptr = np.zeros(r + 1, np.int32)
        self.col = np.zeros(n, np.int32)
        self.val = np.zeros(n, np.float64)

    def copy(self) -> "CSR":  # operator= (deep host copy, src/CSR.cu:34-47)
        return CSR(self.M, self.N, self.ptr.copy(), self.col.copy(), self.val.copy(), self.isSymmetric)

    def H2D(self, device: int = 0):
        torch = _torch()
        dev = f"cuda:{device}"
        self.d_ptr = torch.from_numpy(self.ptr).to(dev)
        self.d_col = torch.from_numpy(self.col).to(dev)
        self.d_val = torch.from_numpy(self.val).to(dev)
        torch.cuda.synchronize(dev)

    def D2H(self):
        if self.dev is not None:
            self.ptr, self.col, self.val = self.dev.to_host()
        else:
            self.ptr = self.d_ptr.cpu().numpy()
            self.col = self.d_col.cpu().numpy()
            self.val = self.d_val.cpu().numpy()
        self.nnz = int(self.col.shape[0])

    def d_release_csr(self):
        if self.dev is not None:
            self.dev.release()
            self.dev = None
        self.d_ptr = self.d_col = self.d_val = None

    def release(self):
        self.d_release_csr()
        self.ptr = self.col = self.val = None

    def c_view(self) -> L.mhs_csr:
        """mhs_csr over the device arrays (for the C-ABI)."""
        if self.dev is not None:
            return self.dev.c
        def p(t):
            return None if t is None or t.numel() == 0 else t.data_ptr()
        return L.mhs_csr(self.M, self.N, self.nnz, p(self.d_ptr), p(self.d_col), p(self.d_val))

    def __eq__(self, other: "CSR") -> bool:
        """CSR::operator== (src/CSR.cu:48-96), vectorised.  Raises RuntimeError
        where the reference throws (nnz mismatch, > 10 errors, ptr[M] mismatch)."""
        if self.nnz != other.nnz:
            print(f"nnz not equal {self.nnz} {other.nnz}")
            raise RuntimeError("nnz not equal")
        assert self.M == other.M and self.N == other.N, "dimension not same"
        return compare_ref(self.ptr, self.col, self.val, other.ptr, other.col, other.val)

    __hash__ = None


def compare_ref(p, c, v, p2, c2, v2, verbose=True) -> bool:
    """The reference comparison rule: ptr and col exact; val accepted when
    |d| < 1e-9 or |d| < 1e-9*|v| (v is the left operand)."""
    M = len(p) - 1
    eps = 1e-9
    if p[M] != p2[M]:
        raise RuntimeError("matrix compare: error num exceed threshold")
    bad_ptr = np.nonzero(p[:M] != p2[:M])[0]
    errs = len(bad_ptr)
    if errs == 0:
        bad_col = np.nonzero(c != c2)[0]
        d = np.abs(v - v2)
        bad_val = np.nonzero(~((d < eps) | (d < eps * np.abs(v))))[0]
        errs += len(bad_col) + len(bad_val)
        if verbose:
            for j in bad_col[:11]:
                print(f"col not equal at index {j}, {c[j]} != {c2[j]}")
            for j in bad_val[:11]:
                print(f"val not eqaul at index {j}, value {v[j]:.18e} != {v2[j]:.18e}")
    elif verbose:
        for i in bad_ptr[:11]:
            print(f"ptr not equal at {i} rows, {p[i]} != {p2[i]}")
    if errs > 10:
        raise RuntimeError("matrix compare: error num exceed threshold")
    return errs == 0


def compare_tol(p_ref, c_ref, v_ref, p, c, v, rtol=1e-6, atol=1e-12):
    """North-star parity: ptr and col bit-exact, |dv| <= rtol*|ref| or <= atol.
    Returns (ok, n_bad_ptr, n_bad_col, n_bad_val, max_rel)."""
    if len(p_ref) != len(p) or p_ref[-1] != p[-1]:
        return False, -1, -1, -1, float("inf")
    bp = int(np.count_nonzero(p_ref != p))
    bc = int(np.count_nonzero(c_ref != c))
    d = np.abs(v_ref - v)
    ok_v = (d <= atol) | (d <= rtol * np.abs(v_ref))
    bv = int(np.count_nonzero(~ok_v))
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(np.abs(v_ref) > 0, d / np.abs(v_ref), d)
    mr = float(rel.max()) if rel.size else 0.0
    return (bp == 0 and bc == 0 and bv == 0), bp, bc, bv, mr


# ------------------------------------------------------------- entry points ---

def spgemm(tool: Tool, A: CSR, B: CSR, timing: bool = True):
    """C = A * B with A, B device-resident (H2D done).  Returns (DeviceCSR, Timing|None)."""
    a, b = A.c_view(), B.c_view()
    c = L.mhs_csr()
    t = L.mhs_timing() if timing else None
    rc = L.lib().mhs_spgemm(tool.ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                            ctypes.byref(t) if t is not None else None)
    _check(tool.ctx, rc, "mhs_spgemm")
    return DeviceCSR(tool, c), (Timing.from_c(t) if t is not None else None)


VALUES_CLASSES = ("none", "team", "wave_direct", "wave_search", "block_direct", "block_search", "global", "dot")
MASK_FORMS = {"auto": L.MHS_MASK_AUTO, "product": L.MHS_MASK_PRODUCT, "dot": L.MHS_MASK_DOT}
VALUES_DTYPES = {"float64": L.MHS_F64, "float32": L.MHS_F32}
VALUES_WIDTHS = (1, 2, 4)
SEMIRINGS = {"plus_times": L.MHS_SR_PLUS_TIMES, "min_plus": L.MHS_SR_MIN_PLUS, "max_plus": L.MHS_SR_MAX_PLUS,
             "max_min": L.MHS_SR_MAX_MIN}


def values_width(width) -> int:
    """A values plan's ``width`` argument as an int: 1, 2 or 4.  ValueError for anything else."""
    if isinstance(width, bool) or not isinstance(width, int) or width not in VALUES_WIDTHS:
        raise ValueError(f"width: one of {VALUES_WIDTHS}, not {width!r}")
    return int(width)


def values_dtype_name(dtype) -> str:
    """``"float64"`` or ``"float32"`` for a values plan's ``dtype`` argument: one of those names (also ``"f64"`` /
    ``"f32"``) or the torch dtype.  ValueError for anything else."""
    name = {"f64": "float64", "f32": "float32"}.get(dtype, dtype) if isinstance(dtype, str) else str(dtype).replace("torch.", "")
    if name not in VALUES_DTYPES:
        raise ValueError(f"dtype: torch.float64 or torch.float32 (or their names), not {dtype!r}")
    return name


def values_accum(accum):
    """A values plan's ``accum`` argument as ``None`` (sums in the plan's value type) or ``"float64"``: ``None``,
    ``"float64"`` / ``"f64"`` or ``torch.float64``.  ValueError for anything else."""
    if accum is None:
        return None
    name = {"f64": "float64"}.get(accum, accum) if isinstance(accum, str) else str(accum).replace("torch.", "")
    if name != "float64":
        raise ValueError(f"accum: None (the plan's value type) or torch.float64 (or its name), not {accum!r}")
    return name


SMOOTHS = {"lse": L.MHS_SMOOTH_LSE}


def values_smooth(smooth):
    """A values plan's ``smooth`` argument as ``None`` (the hard reduce) or ``"lse"`` (log-sum-exp).  ValueError for
    anything else."""
    if smooth is None:
        return None
    if not isinstance(smooth, str) or smooth not in SMOOTHS:
        raise ValueError(f"smooth: None or one of {sorted(SMOOTHS)}, not {smooth!r}")
    return smooth


class _AccumKeyword(type):
    """``ValuesPlan(..., accum=...)``: the sum type is taken here, as a keyword only, checked, and left on the instance
    for ``__init__``, whose own signature stays as released -- ``semiring`` is its trailing argument, so positional
    callers keep their meaning (tests/test_semiring_host.py pins it).  What follows from that: ``accum`` reaches a plan only
    through the constructor call ``ValuesPlan(...)`` -- a direct ``ValuesPlan.__init__`` or ``super().__init__`` makes a
    plan of native sums -- ``inspect.signature(ValuesPlan)`` does not list it, and a subclass that needs a metaclass of
    its own derives it from this one.  Once the pin may move, ``accum`` becomes an ordinary trailing parameter."""

    def __call__(cls, *args, accum=None, smooth=None, **kw):
        self = cls.__new__(cls)
        self.accum = values_accum(accum)
        self.smooth = values_smooth(smooth)  # (``smooth=`` travels the same way, for the same reason)
        self.__init__(*args, **kw)
        return self


class ValuesPlan(metaclass=_AccumKeyword):
    """Values-only SpGEMM on a kept pattern (mhs_values_plan_create / mhs_spgemm_values).

    ``A`` and ``B`` are device-resident ``CSR``; ``C`` is a ``DeviceCSR`` (what ``spgemm``
    returns) or a ``CSR`` with device arrays, whose ``ptr`` / ``col`` hold a pattern containing
    the pattern of A*B.  The plan borrows the six pattern arrays and keeps Python references
    to their owners, so they cannot be collected under it; they must not change while the
    plan lives.  Creation validates the patterns on the device (``MHSpGEMMError`` with status
    3 otherwise); ``run`` does not validate again.

    ``masked=True`` (mhs_values_plan_create_masked): C's pattern is a mask and may be smaller than
    the product's -- products outside it are dropped, mask entries no product reaches get 0.0.
    ``form`` then says how rows are computed: ``"product"`` (walk the products, drop the misses),
    ``"dot"`` (per mask entry, A's row against B's column, through B^T's pattern kept in the plan)
    or ``"auto"`` (per row, the cheaper).  An integer ``form`` is passed to the library as it is.

    ``grad`` is the backward of ``run`` on the same plan (mhs_spgemm_values_grad) and ``apply`` the pair as a
    ``torch.autograd.Function``, for products inside a differentiable program.

    ``dtype`` (``torch.float64``, the default, or ``torch.float32``; also by name) is the plan's value type,
    fixed at creation (mhs_values_plan_create_typed): rows are classified for its size, every tensor of
    ``run``, ``grad`` and ``apply`` must have it (``ValueError`` otherwise) and outputs are allocated in it.
    On a float32 plan ``Aval`` and ``Bval`` must be given: the operands' own ``d_val`` is FP64.

    ``width`` (1, the default, 2 or 4; mhs_values_plan_create_batched) is the number of value sets one walk of the
    patterns sums in ``run_batched``: rows are classified for ``width`` sums per C entry, so ``info()`` differs
    from the width-1 plan's.  Any plan runs any batch.  ``grad_batched`` is the backward of ``run_batched``
    (mhs_spgemm_values_grad_batched) and ``apply_batched`` the pair as a ``torch.autograd.Function``, both on a plan
    of any width; the unbatched ``grad`` and ``apply`` serve width-1 plans only.

    ``semiring`` (``"plus_times"``, the default, ``"min_plus"``, ``"max_plus"`` or ``"max_min"``;
    mhs_values_plan_create_semiring) is what the kept products are reduced with: ``C(i,j) = min_k A(i,k) + B(k,j)``
    and its kin.  Such a plan has width 1 (``ValueError`` otherwise), classifies its rows as the plus-times plan
    does, gives entries no kept product reaches the identity (+Inf, -Inf, -Inf) and results that are bit-identical to
    a sequential evaluation; ``run`` and ``run_batched`` serve it, ``grad``, ``grad_batched``, ``apply`` and
    ``apply_batched`` raise the library's refusal (min and max have subgradients only).  Its backward is ``subgrad``
    (mhs_spgemm_values_subgrad): every product that attains its C entry's value shares the entry's cotangent evenly
    (``torch.amin`` / ``torch.amax``'s split, ``torch.minimum``'s inside max_min), with the tie counts as a third
    result; ``apply_subgrad`` is the pair as a ``torch.autograd.Function``.  Both raise the library's refusal on a
    plus_times plan.  Its arg is ``witness`` (mhs_spgemm_values_witness): the smallest inner index ``k`` among the
    products that attain each C entry, -1 where there is none; ``run_arg`` is the forward and the witness together.
    They raise the library's refusal on a plus_times plan too (a sum has no witness).

    ``accum`` (``None``, the default: sums in the plan's value type; or ``torch.float64``, also by name;
    mhs_values_plan_create_accum) is the plan's sum type.  ``dtype="float32", accum="float64"`` is a mixed plan: float32
    tensors in and out, products and sums in double (an entry is the double sum of exact products, rounded to float
    once), rows classified as the float64 plan's of the same width -- for float32 callers on patterns where the slow
    LDS float add carries the forward.  Rows of the global class and the backward keep float sums.  With
    ``dtype="float64"`` it is the plain float64 plan.  It is refused with another semiring than plus_times
    (``ValueError``).  ``run``, ``run_batched``, ``grad``, ``grad_batched``, ``apply`` and ``apply_batched`` serve a
    mixed plan as they serve a float32 plan.  ``accum`` is a keyword of the constructor call only, taken by the
    metaclass and not by ``__init__`` (see ``_AccumKeyword`` for what that means for subclasses and direct calls).

    ``smooth`` (``None``, the default, or ``"lse"``; mhs_values_plan_create_smooth) smooths a min_plus or max_plus plan:
    ``C(i,j) = log sum_k exp(A(i,k) + B(k,j))`` under max_plus and its negated twin under min_plus, at unit temperature
    (for a temperature tau scale the values by 1 / tau and the result by tau).  ``ValueError`` with another semiring or
    with ``accum``.  Such a plan holds a max and a sum per C entry, so its rows are classified as the width-2 plus_times
    plan's; ``run`` and ``run_batched`` serve it, its backward is ``softgrad`` (mhs_spgemm_values_softgrad: the true
    gradient, softmax weights over the products, no ties) and ``apply_soft`` the pair as a ``torch.autograd.Function``;
    ``subgrad``, ``apply_subgrad``, ``witness`` and ``run_arg`` raise the library's refusal on it, and ``softgrad`` and
    ``apply_soft`` on every other plan.  ``plan.smooth`` and ``info()["smooth"]`` say ``None`` or ``"lse"``.  Like
    ``accum`` it is a keyword of the constructor call only."""

    _semiring = "plus_times"
    smooth = None

    def __init__(self, tool: Tool, A: CSR, B: CSR, C, masked: bool = False, form="auto", dtype="float64", width=1,
                 semiring="plus_times"):
        self.width = values_width(width)
        self.accum = getattr(self, "accum", None)  # (the keyword ``accum``, checked: _AccumKeyword)
        if not isinstance(semiring, str) or semiring not in SEMIRINGS:
            raise ValueError(f"semiring: one of {sorted(SEMIRINGS)}, not {semiring!r}")
        self._semiring = semiring
        if semiring != "plus_times" and self.width != 1:
            raise ValueError(f"width: a {semiring} plan has width 1, not {self.width}")
        if semiring != "plus_times" and self.accum is not None:
            raise ValueError(f"accum: a {semiring} plan sums nothing (min and max are exact in any type): accum must be None, "
                             f"not {self.accum!r}")
        self.smooth = getattr(self, "smooth", None)  # (the keyword ``smooth``, checked: _AccumKeyword)
        if self.smooth is not None and semiring not in ("min_plus", "max_plus"):
            raise ValueError(f"smooth: {self.smooth!r} smooths a min_plus or max_plus plan, not a {semiring} one")
        if self.smooth is not None and self.accum is not None:
            raise ValueError(f"smooth: a smoothed plan sums in its value type: accum must be None, not {self.accum!r}")
        if not hasattr(L.lib(), "mhs_values_plan_create"):
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "this libmhspgemm.so has no values-only entry points")
        if self.smooth is not None and not hasattr(L.lib(), "mhs_values_plan_create_smooth"):
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "this libmhspgemm.so has no soft semiring entry points")
        if masked and not hasattr(L.lib(), "mhs_values_plan_create_masked"):
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "this libmhspgemm.so has no masked entry points")
        self.dtype_name = values_dtype_name(dtype)
        self.f32 = self.dtype_name == "float32"
        if self.width > 1 and not hasattr(L.lib(), "mhs_values_plan_create_batched"):
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "this libmhspgemm.so has no batched values entry points")
        if self.f32 and not hasattr(L.lib(), "mhs_values_plan_create_typed"):
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "this libmhspgemm.so has no FP32 values entry points")
        if semiring != "plus_times" and not hasattr(L.lib(), "mhs_values_plan_create_semiring"):
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "this libmhspgemm.so has no semiring values entry points")
        if self.accum is not None and not hasattr(L.lib(), "mhs_values_plan_create_accum"):
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "this libmhspgemm.so has no mixed-precision values entry points")
        if isinstance(form, str):
            if form not in MASK_FORMS:
                raise ValueError(f"form: one of {sorted(MASK_FORMS)}, not {form!r}")
            form = MASK_FORMS[form]
        self.masked, self.form = bool(masked), int(form)
        self.tool, self.A, self.B, self.C = tool, A, B, C
        # (tensors can be rebound on the CSR objects: hold the arrays themselves too)
        self._keep = (A.d_ptr, A.d_col, A.dev, B.d_ptr, B.d_col, B.dev,
                      getattr(C, "d_ptr", None), getattr(C, "d_col", None), getattr(C, "dev", None))
        a, b = A.c_view(), B.c_view()
        c = C.c if isinstance(C, DeviceCSR) else C.c_view()
        self._c = c
        self.nnzA, self.nnzB, self.nnzC = int(a.nnz), int(b.nnz), int(c.nnz)
        self.plan = ctypes.c_void_p()
        self._pad = None
        if self.smooth is not None:
            rc = L.lib().mhs_values_plan_create_smooth(tool.ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                                       int(self.masked), self.form, VALUES_DTYPES[self.dtype_name],
                                                       SEMIRINGS[semiring], SMOOTHS[self.smooth], ctypes.byref(self.plan))
            _check(tool.ctx, rc, "mhs_values_plan_create_smooth")
        elif semiring != "plus_times":
            rc = L.lib().mhs_values_plan_create_semiring(tool.ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                                         int(self.masked), self.form, VALUES_DTYPES[self.dtype_name],
                                                         SEMIRINGS[semiring], ctypes.byref(self.plan))
            _check(tool.ctx, rc, "mhs_values_plan_create_semiring")
        elif self.accum is not None:
            rc = L.lib().mhs_values_plan_create_accum(tool.ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                                      int(self.masked), self.form, VALUES_DTYPES[self.dtype_name],
                                                      self.width, L.MHS_ACC_F64, ctypes.byref(self.plan))
            _check(tool.ctx, rc, "mhs_values_plan_create_accum")
        elif self.width > 1:
            rc = L.lib().mhs_values_plan_create_batched(tool.ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                                        int(self.masked), self.form, VALUES_DTYPES[self.dtype_name],
                                                        self.width, ctypes.byref(self.plan))
            _check(tool.ctx, rc, "mhs_values_plan_create_batched")
        elif self.f32:
            rc = L.lib().mhs_values_plan_create_typed(tool.ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                                      int(self.masked), self.form, L.MHS_F32, ctypes.byref(self.plan))
            _check(tool.ctx, rc, "mhs_values_plan_create_typed")
        elif masked:
            rc = L.lib().mhs_values_plan_create_masked(tool.ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                                       self.form, ctypes.byref(self.plan))
            _check(tool.ctx, rc, "mhs_values_plan_create_masked")
        else:
            rc = L.lib().mhs_values_plan_create(tool.ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                                ctypes.byref(self.plan))
            _check(tool.ctx, rc, "mhs_values_plan_create")

    @property
    def dtype(self):
        """The plan's value type as a torch dtype."""
        return getattr(_torch(), self.dtype_name)

    @property
    def semiring(self) -> str:
        """The plan's semiring by name (a key of ``SEMIRINGS``)."""
        return self._semiring

    def _refuse_backward(self, what):
        """The library's refusal of a backward call on a plan of another semiring than plus-times, before anything
        runs or is written."""
        if self._semiring != "plus_times":
            call = L.lib().mhs_spgemm_values_grad_f32 if self.f32 else L.lib().mhs_spgemm_values_grad
            _check(self.tool.ctx, call(self.tool.ctx, self.plan, None, None, None, None, None, None), what)

    def _ptr(self, t, n, what):
        if t is None:
            return None
        torch = _torch()
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == self.dtype and t.is_contiguous()
                and t.numel() == n):
            got = f" (got {t.dtype})" if isinstance(t, torch.Tensor) and t.dtype != self.dtype else ""
            raise ValueError(f"{what}: a {self.dtype_name} plan needs a contiguous {self.dtype_name} device tensor of {n} "
                             f"entries{got}")
        return t.data_ptr() if n else None

    def _own(self, X, given, n, what):
        """The value pointer of an operand: the tensor given, or (FP64 plans) the operand's own ``d_val``."""
        if given is not None:
            return self._ptr(given, n, what)
        if self.f32:
            raise ValueError(f"{what}: a float32 plan needs the values as a tensor (the operand's own d_val is float64)")
        return X.c_view().val

    def run(self, Aval=None, Bval=None, out=None, timed: bool = False):
        """C's values of A*B for the values ``Aval`` / ``Bval`` (torch device tensors of the plan's dtype,
        nnz(A) / nnz(B) entries; default, FP64 plans only: the operands' own ``d_val``) into ``out`` (nnz(C)
        entries; default, FP64 plans only: C's own ``val``).  Returns the call's hipEvent time in ms when
        ``timed``, else None (the call then follows MHS_OPT_SYNC)."""
        if not self.plan:
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "ValuesPlan.run: the plan is closed")
        av = self._own(self.A, Aval, self.nnzA, "Aval")
        bv = self._own(self.B, Bval, self.nnzB, "Bval")
        if out is None and self.f32:
            raise ValueError("out: a float32 plan needs an output tensor (C's own val is float64)")
        cv = self._c.val if out is None else self._ptr(out, self.nnzC, "out")
        ms = ctypes.c_double(0.0)
        call = L.lib().mhs_spgemm_values_f32 if self.f32 else L.lib().mhs_spgemm_values
        rc = call(self.tool.ctx, self.plan, av, bv, cv, ctypes.byref(ms) if timed else None)
        _check(self.tool.ctx, rc, "mhs_spgemm_values_f32" if self.f32 else "mhs_spgemm_values")
        return float(ms.value) if timed else None

    def _sets(self, t, nnz, what):
        """A batched operand: ``[nb, nnz]`` (inner stride 1, row stride >= nnz) or ``[nnz]`` (shared by all sets).
        Returns (pointer, stride in elements, nb or None)."""
        torch = _torch()
        if not (isinstance(t, torch.Tensor) and t.dtype == self.dtype and t.dim() in (1, 2)):
            got = f" (got {t.dtype})" if isinstance(t, torch.Tensor) and t.dtype != self.dtype else ""
            raise ValueError(f"{what}: a {self.dtype_name} tensor of shape [nb, {nnz}] or [{nnz}]{got}")
        if t.shape[-1] != nnz or (nnz > 1 and t.stride(-1) != 1):
            raise ValueError(f"{what}: {nnz} entries per set with inner stride 1, not shape {tuple(t.shape)} "
                             f"stride {tuple(t.stride())}")
        if t.dim() == 1:
            return (t.data_ptr() if nnz else None), 0, None
        nb = int(t.shape[0])
        if nb < 1:
            raise ValueError(f"{what}: at least one value set")
        stride = int(t.stride(0)) if nb > 1 else max(int(t.stride(0)), nnz)
        if stride < nnz:
            raise ValueError(f"{what}: a row stride of at least {nnz}, not {stride}")
        return (t.data_ptr() if nnz else None), stride, nb

    def run_batched(self, Aval, Bval, out=None, timed: bool = False):
        """C's values for ``nb`` value sets in one call (mhs_spgemm_values_batched): ``Aval`` / ``Bval`` are device
        tensors of the plan's dtype shaped ``[nb, nnz]`` (any row stride >= nnz, inner stride 1) or ``[nnz]`` (one
        array shared by all sets); ``nb`` comes from whichever is 2-D (both 1-D: 1).  ``out``: ``[nb, nnz(C)]``, row
        stride >= nnz(C); allocated when not given.  Returns ``out``, or ``(out, ms)`` when ``timed``.  The plan's
        width sets share each walk of the patterns; a width-1 plan runs the unbatched kernels ``nb`` times."""
        if not self.plan:
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "ValuesPlan.run_batched: the plan is closed")
        if not hasattr(L.lib(), "mhs_spgemm_values_batched"):
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "this libmhspgemm.so has no batched values entry points")
        torch = _torch()
        av, sa, na = self._sets(Aval, self.nnzA, "Aval")
        bv, sb, nb_ = self._sets(Bval, self.nnzB, "Bval")
        if na is not None and nb_ is not None and na != nb_:
            raise ValueError(f"Aval has {na} value sets, Bval {nb_}")
        nb = na if na is not None else nb_ if nb_ is not None else 1
        if out is None:
            if not (Aval.is_cuda and Bval.is_cuda):
                raise ValueError("Aval, Bval: device tensors")
            out = torch.empty((nb, self.nnzC), dtype=self.dtype, device=Aval.device)
        if not (isinstance(out, torch.Tensor) and out.dim() == 2):
            raise ValueError(f"out: a {self.dtype_name} tensor of shape [{nb}, {self.nnzC}]")
        cv, sc, nc = self._sets(out, self.nnzC, "out")
        if nc != nb:
            raise ValueError(f"out has {nc} value sets, the inputs {nb}")
        for t, what in ((Aval, "Aval"), (Bval, "Bval"), (out, "out")):
            if not t.is_cuda:
                raise ValueError(f"{what}: a device tensor")
        ms = ctypes.c_double(0.0)
        name = "mhs_spgemm_values_batched_f32" if self.f32 else "mhs_spgemm_values_batched"
        rc = getattr(L.lib(), name)(self.tool.ctx, self.plan, nb, av, sa, bv, sb, cv, sc, ctypes.byref(ms) if timed else None)
        _check(self.tool.ctx, rc, name)
        return (out, float(ms.value)) if timed else out

    def grad(self, dC, Aval=None, Bval=None, need_A: bool = True, need_B: bool = True, out_A=None, out_B=None,
             timed: bool = False):
        """The backward of ``run`` (mhs_spgemm_values_grad): for the cotangent ``dC`` on C's pattern (nnz(C)
        entries) the gradients of ``Aval`` and ``Bval`` (default: the operands' own ``d_val``), into ``out_A`` /
        ``out_B`` (nnz(A) / nnz(B) entries; allocated with torch when not given).  Tensors as in ``run``.
        Returns ``(dA, dB)`` with None for a side not asked for -- that side's buffer is not touched and the
        other operand's values are not read -- and ``(dA, dB, ms)`` when ``timed``.  When one tensor is both
        ``Aval`` and ``Bval`` (A*A) the two gradients still come back apart: the caller (autograd) adds them."""
        if not self.plan:
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "ValuesPlan.grad: the plan is closed")
        if not hasattr(L.lib(), "mhs_spgemm_values_grad"):
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "this libmhspgemm.so has no mhs_spgemm_values_grad")
        if not (need_A or need_B):
            raise ValueError("ValuesPlan.grad: need_A or need_B")
        self._refuse_backward("ValuesPlan.grad")
        torch = _torch()
        dev = f"cuda:{self.tool.device}"
        gp = self._ptr(dC, self.nnzC, "dC")
        # (an empty array has no address; the library wants one for every array it is given: nothing reads it)
        if self._pad is None:
            self._pad = torch.zeros(1, dtype=self.dtype, device=dev)
        pad = self._pad.data_ptr()
        av = bv = pa = pb = None
        dA = dB = None
        if need_A:
            bv = self._own(self.B, Bval, self.nnzB, "Bval") or pad
            dA = torch.empty(self.nnzA, dtype=self.dtype, device=dev) if out_A is None else out_A
            pa = self._ptr(dA, self.nnzA, "out_A") or pad
        if need_B:
            av = self._own(self.A, Aval, self.nnzA, "Aval") or pad
            dB = torch.empty(self.nnzB, dtype=self.dtype, device=dev) if out_B is None else out_B
            pb = self._ptr(dB, self.nnzB, "out_B") or pad
        ms = ctypes.c_double(0.0)
        call = L.lib().mhs_spgemm_values_grad_f32 if self.f32 else L.lib().mhs_spgemm_values_grad
        rc = call(self.tool.ctx, self.plan, av, bv, gp or pad, pa, pb, ctypes.byref(ms) if timed else None)
        _check(self.tool.ctx, rc, "mhs_spgemm_values_grad_f32" if self.f32 else "mhs_spgemm_values_grad")
        return (dA, dB, float(ms.value)) if timed else (dA, dB)

    def apply(self, Aval, Bval):
        """C's values of A*B as a differentiable function of ``Aval`` and ``Bval`` (a ``torch.autograd.Function``):
        the forward is ``run`` into a fresh nnz(C) tensor, the backward ``grad`` for the inputs that need it
        (once differentiable).  Both are ordered on torch's current stream, also with MHS_OPT_SYNC 0: a stream
        of torch's making is handed to the tool; torch's default stream (the null stream, handle 0) cannot be,
        so there the calls run on the tool's own stream between two fences (``Tool.fence_default_stream``)."""
        self._refuse_backward("ValuesPlan.apply")
        if self.width > 1:  # no backward on a batched plan: the library's refusal, before the forward runs
            call = L.lib().mhs_spgemm_values_grad_f32 if self.f32 else L.lib().mhs_spgemm_values_grad
            _check(self.tool.ctx, call(self.tool.ctx, self.plan, None, None, None, None, None, None), "ValuesPlan.apply")
        return _values_function().apply(self, Aval, Bval)

    def grad_batched(self, dC, Aval, Bval, need_A: bool = True, need_B: bool = True, out_A=None, out_B=None,
                     timed: bool = False):
        """The backward of ``run_batched`` (mhs_spgemm_values_grad_batched), on a plan of any width: ``dC`` is the
        cotangent ``[nb, nnz(C)]``, ``Aval`` / ``Bval`` are ``[nb, nnz]`` or ``[nnz]`` (shared by all sets) as in
        ``run_batched``; a side's operand that is not needed (``Bval`` with ``need_A=False``, ``Aval`` with
        ``need_B=False``) may be None.  Returns ``(dA, dB)``, each ``[nb, nnz]`` -- one gradient per set also for a
        shared operand, whose gradient is their sum over the sets -- into ``out_A`` / ``out_B`` (row stride >= nnz;
        allocated when not given), with None for a side not asked for, whose buffer is not touched; and
        ``(dA, dB, ms)`` when ``timed``.  The plan's width sets share each walk of the patterns; a width-1 plan runs
        the unbatched backward kernels ``nb`` times."""
        if not self.plan:
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "ValuesPlan.grad_batched: the plan is closed")
        if not hasattr(L.lib(), "mhs_spgemm_values_grad_batched"):
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "this libmhspgemm.so has no batched backward entry points")
        if not (need_A or need_B):
            raise ValueError("ValuesPlan.grad_batched: need_A or need_B")
        self._refuse_backward("ValuesPlan.grad_batched")
        torch = _torch()
        if not (isinstance(dC, torch.Tensor) and dC.dim() == 2):
            raise ValueError(f"dC: a {self.dtype_name} tensor of shape [nb, {self.nnzC}]")
        gp, sg, nb = self._sets(dC, self.nnzC, "dC")
        used = [(dC, "dC")]
        av = bv = pa = pb = None
        sa = sb = sda = sdb = 0
        dA = dB = None

        def operand(t, nnz, what):
            ptr, stride, n = self._sets(t, nnz, what)
            if n is not None and n != nb:
                raise ValueError(f"{what} has {n} value sets, dC {nb}")
            used.append((t, what))
            return ptr, stride

        def output(t, nnz, what):
            if t is None:  # (beside dC, which the device check below looks at first)
                t = torch.empty((nb, nnz), dtype=self.dtype, device=dC.device)
            if not (isinstance(t, torch.Tensor) and t.dim() == 2):
                raise ValueError(f"{what}: a {self.dtype_name} tensor of shape [{nb}, {nnz}]")
            ptr, stride, n = self._sets(t, nnz, what)
            if n != nb:
                raise ValueError(f"{what} has {n} value sets, dC {nb}")
            used.append((t, what))
            return t, ptr, stride

        if need_B:
            av, sa = operand(Aval, self.nnzA, "Aval")
        if need_A:
            bv, sb = operand(Bval, self.nnzB, "Bval")
            dA, pa, sda = output(out_A, self.nnzA, "out_A")
        if need_B:
            dB, pb, sdb = output(out_B, self.nnzB, "out_B")
        for t, what in used:
            if not t.is_cuda:
                raise ValueError(f"{what}: a device tensor")
        # (an empty array has no address; the library wants one for every array it is given: nothing reads it)
        if self._pad is None:
            self._pad = torch.zeros(1, dtype=self.dtype, device=dC.device)
        pad = self._pad.data_ptr()
        if need_A:
            bv, pa = bv or pad, pa or pad
        if need_B:
            av, pb = av or pad, pb or pad
        ms = ctypes.c_double(0.0)
        name = "mhs_spgemm_values_grad_batched_f32" if self.f32 else "mhs_spgemm_values_grad_batched"
        rc = getattr(L.lib(), name)(self.tool.ctx, self.plan, nb, av, sa, bv, sb, gp or pad, sg, pa, sda, pb, sdb,
                                    ctypes.byref(ms) if timed else None)
        _check(self.tool.ctx, rc, name)
        return (dA, dB, float(ms.value)) if timed else (dA, dB)

    def apply_batched(self, Aval, Bval):
        """``run_batched`` as a differentiable function of ``Aval`` and ``Bval`` (a ``torch.autograd.Function``), on
        a plan of any width: the forward is ``run_batched`` into a fresh ``[nb, nnz(C)]`` tensor, the backward
        ``grad_batched`` for the inputs that need it (once differentiable), both ordered on torch's current stream
        as in ``apply``.  The gradient of a 1-D (shared) operand is the per-set gradients summed over the sets."""
        self._refuse_backward("ValuesPlan.apply_batched")
        return _values_batched_function().apply(self, Aval, Bval)

    def _refuse_subgrad(self, what):
        """The library's refusal of a subgradient call on a plus-times plan, before anything runs or is written."""
        if not hasattr(L.lib(), "mhs_spgemm_values_subgrad"):
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "this libmhspgemm.so has no semiring subgradient entry points")
        if self._semiring == "plus_times" or self.smooth is not None:  # (a smoothed plan has a gradient: softgrad)
            call = L.lib().mhs_spgemm_values_subgrad_f32 if self.f32 else L.lib().mhs_spgemm_values_subgrad
            _check(self.tool.ctx, call(self.tool.ctx, self.plan, None, None, None, None, None, None, None, None), what)

    def subgrad(self, dC, Cval, Aval, Bval, need_A: bool = True, need_B: bool = True, out_A=None, out_B=None, ties=None,
                timed: bool = False):
        """The backward of ``run`` on a min_plus, max_plus or max_min plan (mhs_spgemm_values_subgrad): for the
        cotangent ``dC`` on C's pattern and ``Cval``, the forward's result for ``Aval`` and ``Bval`` (all device
        tensors of the plan's dtype; all four are always needed), the subgradients of ``Aval`` and ``Bval`` into
        ``out_A`` / ``out_B`` (allocated when not given) and the winners per C entry into ``ties`` (an int32 device
        tensor of nnz(C) entries; allocated when not given).  A product is a winner of its C entry when it equals
        ``Cval`` there and that is not the identity; each winner of an entry carries ``dC / ties``, handed to both
        operands under the _plus semirings and to the smaller one under max_min (half each when equal).  Returns
        ``(dA, dB, ties)`` with None for a side not asked for, whose buffer is not touched, and
        ``(dA, dB, ties, ms)`` when ``timed``.  A plus_times plan raises the library's refusal."""
        if not self.plan:
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "ValuesPlan.subgrad: the plan is closed")
        if not (need_A or need_B):
            raise ValueError("ValuesPlan.subgrad: need_A or need_B")
        self._refuse_subgrad("ValuesPlan.subgrad")
        torch = _torch()
        dev = f"cuda:{self.tool.device}"
        # (an empty array has no address; the library wants one for every array it is given: nothing reads it)
        if self._pad is None:
            self._pad = torch.zeros(1, dtype=self.dtype, device=dev)
        pad = self._pad.data_ptr()
        gp = self._ptr(dC, self.nnzC, "dC") or pad
        cp = self._ptr(Cval, self.nnzC, "Cval") or pad
        av = self._ptr(Aval, self.nnzA, "Aval") or pad
        bv = self._ptr(Bval, self.nnzB, "Bval") or pad
        if ties is None:
            ties = torch.empty(self.nnzC, dtype=torch.int32, device=dev)
        if not (isinstance(ties, torch.Tensor) and ties.is_cuda and ties.dtype == torch.int32 and ties.is_contiguous()
                and ties.numel() == self.nnzC):
            raise ValueError(f"ties: a contiguous int32 device tensor of {self.nnzC} entries")
        pa = pb = None
        dA = dB = None
        if need_A:
            dA = torch.empty(self.nnzA, dtype=self.dtype, device=dev) if out_A is None else out_A
            pa = self._ptr(dA, self.nnzA, "out_A") or pad
        if need_B:
            dB = torch.empty(self.nnzB, dtype=self.dtype, device=dev) if out_B is None else out_B
            pb = self._ptr(dB, self.nnzB, "out_B") or pad
        ms = ctypes.c_double(0.0)
        name = "mhs_spgemm_values_subgrad_f32" if self.f32 else "mhs_spgemm_values_subgrad"
        rc = getattr(L.lib(), name)(self.tool.ctx, self.plan, av, bv, cp, gp, ties.data_ptr() if self.nnzC else pad, pa, pb,
                                    ctypes.byref(ms) if timed else None)
        _check(self.tool.ctx, rc, name)
        return (dA, dB, ties, float(ms.value)) if timed else (dA, dB, ties)

    def apply_subgrad(self, Aval, Bval):
        """C's values on a min_plus, max_plus or max_min plan as a differentiable function of ``Aval`` and ``Bval`` (a
        ``torch.autograd.Function``): the forward is ``run`` into a fresh nnz(C) tensor, saved with both inputs, the
        backward ``subgrad`` for the inputs that need it (once differentiable).  Both are ordered on torch's current
        stream as in ``apply``.  A plus_times plan raises the library's refusal (``apply`` serves it)."""
        self._refuse_subgrad("ValuesPlan.apply_subgrad")
        return _values_subgrad_function().apply(self, Aval, Bval)

    def _refuse_softgrad(self, what):
        """The library's refusal of a soft gradient call on a plan that is not smoothed, before anything runs or is
        written."""
        if not hasattr(L.lib(), "mhs_spgemm_values_softgrad"):
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "this libmhspgemm.so has no soft semiring entry points")
        if self.smooth is None:
            call = L.lib().mhs_spgemm_values_softgrad_f32 if self.f32 else L.lib().mhs_spgemm_values_softgrad
            _check(self.tool.ctx, call(self.tool.ctx, self.plan, None, None, None, None, None, None, None), what)

    def softgrad(self, dC, Cval, Aval, Bval, need_A: bool = True, need_B: bool = True, out_A=None, out_B=None,
                 timed: bool = False):
        """The backward of ``run`` on a smoothed plan (``smooth="lse"``; mhs_spgemm_values_softgrad): for the cotangent
        ``dC`` on C's pattern and ``Cval``, the forward's result for ``Aval`` and ``Bval`` (all device tensors of the
        plan's dtype; all four are always needed), the gradients of ``Aval`` and ``Bval`` into ``out_A`` / ``out_B``
        (allocated when not given).  Every kept product carries ``dC * exp(v - Cval)`` (max_plus; min_plus:
        ``exp(Cval - v)``) -- its softmax weight -- to both operands; an entry whose ``Cval`` is not finite passes
        nothing.  Returns ``(dA, dB)`` with None for a side not asked for, whose buffer is not touched, and
        ``(dA, dB, ms)`` when ``timed``.  A plan that is not smoothed raises the library's refusal."""
        if not self.plan:
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "ValuesPlan.softgrad: the plan is closed")
        if not (need_A or need_B):
            raise ValueError("ValuesPlan.softgrad: need_A or need_B")
        self._refuse_softgrad("ValuesPlan.softgrad")
        torch = _torch()
        dev = f"cuda:{self.tool.device}"
        # (an empty array has no address; the library wants one for every array it is given: nothing reads it)
        if self._pad is None:
            self._pad = torch.zeros(1, dtype=self.dtype, device=dev)
        pad = self._pad.data_ptr()
        gp = self._ptr(dC, self.nnzC, "dC") or pad
        cp = self._ptr(Cval, self.nnzC, "Cval") or pad
        av = self._ptr(Aval, self.nnzA, "Aval") or pad
        bv = self._ptr(Bval, self.nnzB, "Bval") or pad
        pa = pb = None
        dA = dB = None
        if need_A:
            dA = torch.empty(self.nnzA, dtype=self.dtype, device=dev) if out_A is None else out_A
            pa = self._ptr(dA, self.nnzA, "out_A") or pad
        if need_B:
            dB = torch.empty(self.nnzB, dtype=self.dtype, device=dev) if out_B is None else out_B
            pb = self._ptr(dB, self.nnzB, "out_B") or pad
        ms = ctypes.c_double(0.0)
        name = "mhs_spgemm_values_softgrad_f32" if self.f32 else "mhs_spgemm_values_softgrad"
        rc = getattr(L.lib(), name)(self.tool.ctx, self.plan, av, bv, cp, gp, pa, pb, ctypes.byref(ms) if timed else None)
        _check(self.tool.ctx, rc, name)
        return (dA, dB, float(ms.value)) if timed else (dA, dB)

    def apply_soft(self, Aval, Bval):
        """C's values on a smoothed plan as a differentiable function of ``Aval`` and ``Bval`` (a
        ``torch.autograd.Function``): the forward is ``run`` into a fresh nnz(C) tensor, saved with both inputs, the
        backward ``softgrad`` for the inputs that need it (once differentiable).  Both are ordered on torch's current
        stream as in ``apply_subgrad``.  A plan that is not smoothed raises the library's refusal."""
        self._refuse_softgrad("ValuesPlan.apply_soft")
        return _values_soft_function().apply(self, Aval, Bval)

    def _refuse_witness(self, what):
        """The library's refusal of a witness call on a plus-times plan, before anything runs or is written."""
        if not hasattr(L.lib(), "mhs_spgemm_values_witness"):
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "this libmhspgemm.so has no semiring witness entry points")
        if self._semiring == "plus_times" or self.smooth is not None:  # (a soft reduce has no witness)
            call = L.lib().mhs_spgemm_values_witness_f32 if self.f32 else L.lib().mhs_spgemm_values_witness
            _check(self.tool.ctx, call(self.tool.ctx, self.plan, None, None, None, None, None), what)

    def witness(self, Cval, Aval, Bval, out=None, timed: bool = False):
        """The arg of ``run`` on a min_plus, max_plus or max_min plan (mhs_spgemm_values_witness): for ``Cval``, the
        forward's result for ``Aval`` and ``Bval`` (device tensors of the plan's dtype; all three are always needed),
        the inner index ``k`` through which each C entry got its value -- the predecessor on the shortest path, the
        Viterbi back-pointer -- into ``out`` (an int32 device tensor of nnz(C) entries; allocated when not given).  A
        product is a winner of its C entry by ``subgrad``'s rule; an entry's witness is the smallest ``k`` (A's
        column, B's row) among its winners, and -1 where it has none: no product reaches it, it is the identity ("no
        path"), or it is NaN.  Returns ``wit``, and ``(wit, ms)`` when ``timed``.  A plus_times plan raises the
        library's refusal."""
        if not self.plan:
            raise MHSpGEMMError(L.MHS_ERR_INVALID, "ValuesPlan.witness: the plan is closed")
        self._refuse_witness("ValuesPlan.witness")
        torch = _torch()
        dev = f"cuda:{self.tool.device}"
        # (an empty array has no address; the library wants one for every array it is given: nothing reads it)
        if self._pad is None:
            self._pad = torch.zeros(1, dtype=self.dtype, device=dev)
        pad = self._pad.data_ptr()
        cp = self._ptr(Cval, self.nnzC, "Cval") or pad
        av = self._ptr(Aval, self.nnzA, "Aval") or pad
        bv = self._ptr(Bval, self.nnzB, "Bval") or pad
        wit = torch.empty(self.nnzC, dtype=torch.int32, device=dev) if out is None else out
        if not (isinstance(wit, torch.Tensor) and wit.is_cuda and wit.dtype == torch.int32 and wit.is_contiguous()
                and wit.numel() == self.nnzC):
            raise ValueError(f"out: a contiguous int32 device tensor of {self.nnzC} entries")
        ms = ctypes.c_double(0.0)
        name = "mhs_spgemm_values_witness_f32" if self.f32 else "mhs_spgemm_values_witness"
        rc = getattr(L.lib(), name)(self.tool.ctx, self.plan, av, bv, cp, wit.data_ptr() if self.nnzC else pad,
                                    ctypes.byref(ms) if timed else None)
        _check(self.tool.ctx, rc, name)
        return (wit, float(ms.value)) if timed else wit

    def run_arg(self, Aval, Bval):
        """C's values on a min_plus, max_plus or max_min plan together with their witnesses: ``(Cval, wit)``, the
        forward ``run`` into a fresh nnz(C) tensor and then ``witness`` on it.  Both are ordered on torch's current
        stream as in ``apply``.  A plus_times plan raises the library's refusal."""
        self._refuse_witness("ValuesPlan.run_arg")
        torch = _torch()
        out = torch.empty(self.nnzC, dtype=self.dtype, device=f"cuda:{self.tool.device}")

        def both():
            self.run(Aval, Bval, out=out)
            return out, self.witness(out, Aval, Bval)

        return self._ordered_on_current_stream(both)

    def _ordered_on_current_stream(self, call):
        """Run ``call()`` with its library work ordered after what torch's current stream holds, and before
        what it is given next."""
        torch = _torch()
        handle = torch.cuda.current_stream(self.tool.device).cuda_stream
        self.tool.set_stream(handle)
        if handle:
            return call()
        self.tool.fence_default_stream(after=False)
        try:
            return call()
        finally:
            self.tool.fence_default_stream(after=True)

    def info(self) -> dict:
        """Rows per class (by name and as the ``rows`` list indexed by class id), products, nnzC, plan_bytes,
        kept_products: the products that land in C's pattern (all of them unless the plan is masked), dtype:
        the plan's value type by name, width: its value sets per walk, semiring: its semiring by name, and accum: its
        sum type -- ``"float64"`` on a mixed plan (float32 values summed in double), ``None`` where the sums have the
        value type -- and smooth: ``"lse"`` on a smoothed min_plus or max_plus plan, else ``None`` (all five as the
        library reports them)."""
        i = L.mhs_values_info()
        _check(self.tool.ctx, L.lib().mhs_values_plan_info(self.plan, ctypes.byref(i)), "mhs_values_plan_info")
        rows = [int(x) for x in i.rows]
        d = {"rows": rows, "products": int(i.products), "nnzC": int(i.nnzC), "plan_bytes": int(i.plan_bytes)}
        d.update({name: rows[k] for k, name in enumerate(VALUES_CLASSES)})
        d["kept_products"] = d["products"]
        if hasattr(L.lib(), "mhs_values_plan_kept"):
            kept = ctypes.c_int64(0)
            _check(self.tool.ctx, L.lib().mhs_values_plan_kept(self.plan, ctypes.byref(kept)), "mhs_values_plan_kept")
            d["kept_products"] = int(kept.value)
        d["dtype"] = "float64"
        if hasattr(L.lib(), "mhs_values_plan_dtype"):
            dt = ctypes.c_int(0)
            _check(self.tool.ctx, L.lib().mhs_values_plan_dtype(self.plan, ctypes.byref(dt)), "mhs_values_plan_dtype")
            d["dtype"] = {v: k for k, v in VALUES_DTYPES.items()}[int(dt.value)]
        d["width"] = 1
        if hasattr(L.lib(), "mhs_values_plan_width"):
            w = ctypes.c_int(0)
            _check(self.tool.ctx, L.lib().mhs_values_plan_width(self.plan, ctypes.byref(w)), "mhs_values_plan_width")
            d["width"] = int(w.value)
        d["semiring"] = "plus_times"
        if hasattr(L.lib(), "mhs_values_plan_semiring"):
            sr = ctypes.c_int(0)
            _check(self.tool.ctx, L.lib().mhs_values_plan_semiring(self.plan, ctypes.byref(sr)), "mhs_values_plan_semiring")
            d["semiring"] = {v: k for k, v in SEMIRINGS.items()}[int(sr.value)]
        d["accum"] = None
        if hasattr(L.lib(), "mhs_values_plan_accum"):
            acc = ctypes.c_int(0)
            _check(self.tool.ctx, L.lib().mhs_values_plan_accum(self.plan, ctypes.byref(acc)), "mhs_values_plan_accum")
            d["accum"] = "float64" if int(acc.value) == L.MHS_ACC_F64 else None
        d["smooth"] = None
        if hasattr(L.lib(), "mhs_values_plan_smooth"):
            sm = ctypes.c_int(0)
            _check(self.tool.ctx, L.lib().mhs_values_plan_smooth(self.plan, ctypes.byref(sm)), "mhs_values_plan_smooth")
            d["smooth"] = {v: k for k, v in SMOOTHS.items()}.get(int(sm.value))
        return d

    def close(self):
        if self.plan:
            L.lib().mhs_values_plan_destroy(self.tool.ctx, self.plan)
            self.plan = ctypes.c_void_p()
        self._keep = ()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_VALUES_FUNCTION = None


def _values_function():
    """The autograd function behind ``ValuesPlan.apply`` (made on first use: torch is imported lazily)."""
    global _VALUES_FUNCTION
    if _VALUES_FUNCTION is not None:
        return _VALUES_FUNCTION
    torch = _torch()
    from torch.autograd.function import once_differentiable

    class ValuesProduct(torch.autograd.Function):
        @staticmethod
        def forward(ctx, plan, Aval, Bval):
            out = torch.empty(plan.nnzC, dtype=plan.dtype, device=f"cuda:{plan.tool.device}")
            plan._ordered_on_current_stream(lambda: plan.run(Aval, Bval, out=out))
            ctx.plan = plan
            ctx.save_for_backward(Aval, Bval)
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, dC):
            Aval, Bval = ctx.saved_tensors
            _, need_A, need_B = ctx.needs_input_grad
            if not (need_A or need_B):
                return None, None, None
            plan, dC = ctx.plan, dC.contiguous()
            dA, dB = plan._ordered_on_current_stream(lambda: plan.grad(dC, Aval, Bval, need_A=need_A, need_B=need_B))
            return None, dA, dB

    _VALUES_FUNCTION = ValuesProduct
    return ValuesProduct


_VALUES_SUBGRAD_FUNCTION = None


def _values_subgrad_function():
    """The autograd function behind ``ValuesPlan.apply_subgrad`` (made on first use, as ``_values_function``)."""
    global _VALUES_SUBGRAD_FUNCTION
    if _VALUES_SUBGRAD_FUNCTION is not None:
        return _VALUES_SUBGRAD_FUNCTION
    torch = _torch()
    from torch.autograd.function import once_differentiable

    class SemiringProduct(torch.autograd.Function):
        @staticmethod
        def forward(ctx, plan, Aval, Bval):
            out = torch.empty(plan.nnzC, dtype=plan.dtype, device=f"cuda:{plan.tool.device}")
            plan._ordered_on_current_stream(lambda: plan.run(Aval, Bval, out=out))
            ctx.plan = plan
            ctx.save_for_backward(Aval, Bval, out)
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, dC):
            Aval, Bval, Cval = ctx.saved_tensors
            _, need_A, need_B = ctx.needs_input_grad
            if not (need_A or need_B):
                return None, None, None
            plan, dC = ctx.plan, dC.contiguous()
            dA, dB, _ = plan._ordered_on_current_stream(
                lambda: plan.subgrad(dC, Cval, Aval, Bval, need_A=need_A, need_B=need_B))
            return None, dA, dB

    _VALUES_SUBGRAD_FUNCTION = SemiringProduct
    return SemiringProduct


_VALUES_SOFT_FUNCTION = None


def _values_soft_function():
    """The autograd function behind ``ValuesPlan.apply_soft`` (made on first use, as ``_values_function``)."""
    global _VALUES_SOFT_FUNCTION
    if _VALUES_SOFT_FUNCTION is not None:
        return _VALUES_SOFT_FUNCTION
    torch = _torch()
    from torch.autograd.function import once_differentiable

    class SoftSemiringProduct(torch.autograd.Function):
        @staticmethod
        def forward(ctx, plan, Aval, Bval):
            out = torch.empty(plan.nnzC, dtype=plan.dtype, device=f"cuda:{plan.tool.device}")
            plan._ordered_on_current_stream(lambda: plan.run(Aval, Bval, out=out))
            ctx.plan = plan
            ctx.save_for_backward(Aval, Bval, out)
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, dC):
            Aval, Bval, Cval = ctx.saved_tensors
            _, need_A, need_B = ctx.needs_input_grad
            if not (need_A or need_B):
                return None, None, None
            plan, dC = ctx.plan, dC.contiguous()
            dA, dB = plan._ordered_on_current_stream(
                lambda: plan.softgrad(dC, Cval, Aval, Bval, need_A=need_A, need_B=need_B))
            return None, dA, dB

    _VALUES_SOFT_FUNCTION = SoftSemiringProduct
    return SoftSemiringProduct


_VALUES_BATCHED_FUNCTION = None


def _values_batched_function():
    """The autograd function behind ``ValuesPlan.apply_batched`` (made on first use, as ``_values_function``)."""
    global _VALUES_BATCHED_FUNCTION
    if _VALUES_BATCHED_FUNCTION is not None:
        return _VALUES_BATCHED_FUNCTION
    torch = _torch()
    from torch.autograd.function import once_differentiable

    class ValuesBatchedProduct(torch.autograd.Function):
        @staticmethod
        def forward(ctx, plan, Aval, Bval):
            out = plan._ordered_on_current_stream(lambda: plan.run_batched(Aval, Bval))
            ctx.plan = plan
            ctx.save_for_backward(Aval, Bval)
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, dC):
            Aval, Bval = ctx.saved_tensors
            _, need_A, need_B = ctx.needs_input_grad
            if not (need_A or need_B):
                return None, None, None
            plan, dC = ctx.plan, dC.contiguous()
            dA, dB = plan._ordered_on_current_stream(
                lambda: plan.grad_batched(dC, Aval, Bval, need_A=need_A, need_B=need_B))
            # a shared (1-D) operand took part in every set: its gradient is the sets' summed
            if dA is not None and Aval.dim() == 1:
                dA = dA.sum(0)
            if dB is not None and Bval.dim() == 1:
                dB = dB.sum(0)
            return None, dA, dB

    _VALUES_BATCHED_FUNCTION = ValuesBatchedProduct
    return ValuesBatchedProduct


def transpose(tool: Tool, A: CSR) -> CSR:
    """A^T on the device (mhs_transpose): the AAT operand B = transpose(A)
    (src/main.cu:98-99, host version src/utils.cpp:20-46).  A must be device-
    resident; the result's device arrays are a library-owned DeviceCSR."""
    a = A.c_view()
    t = L.mhs_csr()
    _check(tool.ctx, L.lib().mhs_transpose(tool.ctx, ctypes.byref(a), ctypes.byref(t)), "mhs_transpose")
    out = CSR(t.M, t.N)
    out.nnz = t.nnz
    out.dev = DeviceCSR(tool, t)
    return out


def matrix_transposition(A: CSR, B: CSR, tool: Tool | None = None) -> None:
    """src/utils.cpp:20-46 (B = A^T, host arrays) computed on the device: A is
    uploaded if needed, transposed with mhs_transpose, and B gets host arrays."""
    own = tool is None
    tool = tool or Tool(0)
    try:
        if A.dev is None and A.d_ptr is None:
            A.H2D(tool.device)
        T = transpose(tool, A)
        B.M, B.N, B.nnz = T.M, T.N, T.nnz
        B.ptr, B.col, B.val = T.dev.to_host()
        B.isSymmetric = 0
        T.d_release_csr()
    finally:
        if own:
            tool.close()


def vendor_spgemm(tool: Tool, A: CSR, B: CSR, warmup: int = 0):
    """rocSPARSE C = A * B (include/mhs_vendor.h; the reference's cusparse_spgemm,
    inc/cusparse_spgemm.cuh:94-105).  `warmup` untimed calls first (rocSPARSE loads its
    code objects on first use).  Returns (DeviceCSR, ms over the reference's span)."""
    V = L.vendor_lib()
    a, b = A.c_view(), B.c_view()
    for i in range(warmup + 1):
        c = L.mhs_csr()
        ms = ctypes.c_double(0.0)
        err = ctypes.create_string_buffer(256)
        rc = V.mhs_vendor_spgemm(tool.device, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                 ctypes.byref(ms), err, 256)
        if rc != L.MHS_OK:
            raise MHSpGEMMError(rc, f"rocSPARSE SpGEMM: {err.value.decode(errors='replace')}")
        if i < warmup:
            V.mhs_vendor_free(ctypes.byref(c))
    return DeviceCSR(tool, c), float(ms.value)


def MH_spgemm(A: CSR, B: CSR, C: CSR, timing: Timing, tools: Tool):
    """src/main.cu:12-72: C.M = A.M, C.N = B.N, C.nnz and C's device arrays set;
    phase times written into `timing`.  Raises MHSpGEMMError on failure."""
    if tools.device is not None:
        try:
            torch = _torch()
            tools.set_stream(torch.cuda.current_stream(tools.device).cuda_stream)
        except Exception:
            tools.set_stream(None)
    dev, t = spgemm(tools, A, B, timing=True)
    C.d_release_csr()
    C.dev = dev
    C.M, C.N, C.nnz = dev.M, dev.N, dev.nnz
    for k in Timing.PHASES + ("flop", "nnzC", "sym_bins", "num_bins"):
        setattr(timing, k, getattr(t, k))
    print(f"C.nnz = {C.nnz}")


def _cache_setting(v):
    """$MHS_MTX_CACHE: unset, "", "0", "false", "no", "off" -> off; "1", "true", "yes", "on" ->
    next to the file; anything else -> a cache directory."""
    if v is None or v.strip().lower() in ("", "0", "false", "no", "off"):
        return False
    if v.strip().lower() in ("1", "true", "yes", "on"):
        return True
    return v


def readMtxFile(A: CSR, filename: str, cache=None) -> int:
    """inc/mmio_read.h:34-159 through the library's parallel reader.

    ``cache`` (default ``$MHS_MTX_CACHE``: unset = off, "1" = next to the file,
    else a directory): read a binary CSR cache stamped with the .mtx's size and
    mtime instead of the text, writing it on a miss."""
    h = L.mhs_host_csr()
    if cache is None:
        cache = _cache_setting(os.environ.get("MHS_MTX_CACHE"))
    if cache and cache is not True and str(cache).lower() not in ("1", "true", "yes", "on"):
        d = os.fspath(cache)
        os.makedirs(d, exist_ok=True)
        cpath = os.path.join(d, os.path.basename(str(filename)) + ".mhscsr").encode()
    else:
        cpath = None
    if cache:
        hit = ctypes.c_int(0)
        rc = L.lib().mhs_read_mtx_cached(str(filename).encode(), cpath, ctypes.byref(h), ctypes.byref(hit))
        readMtxFile.last_from_cache = bool(hit.value)
    else:
        rc = L.lib().mhs_read_mtx(str(filename).encode(), ctypes.byref(h))
        readMtxFile.last_from_cache = False
    if rc != L.MHS_OK:
        print(f"Could not read Matrix Market file {filename}.")
        return -1
    try:
        M, nnz = h.M, h.nnz
        ptr = np.ctypeslib.as_array(ctypes.cast(h.ptr, ctypes.POINTER(ctypes.c_int32)), (M + 1,)).copy()
        if nnz:
            col = np.ctypeslib.as_array(ctypes.cast(h.col, ctypes.POINTER(ctypes.c_int32)), (nnz,)).copy()
            val = np.ctypeslib.as_array(ctypes.cast(h.val, ctypes.POINTER(ctypes.c_double)), (nnz,)).copy()
        else:
            col = np.zeros(0, np.int32)
            val = np.zeros(0, np.float64)
        A.M, A.N, A.nnz = h.M, h.N, nnz
        A.ptr, A.col, A.val = ptr, col, val
        A.isSymmetric = h.is_symmetric
    finally:
        L.lib().mhs_host_csr_free(ctypes.byref(h))
    return 0


def flop_count(A: CSR, B: CSR) -> int:
    """int_result of src/main.cu:102-107 (sum of B row lengths over A's nonzeros)."""
    return int(L.lib().mhs_flop_count(A.nnz, A.col.ctypes.data, B.ptr.ctypes.data))


def flop_count_np(Acol: np.ndarray, Bptr: np.ndarray) -> int:
    blen = np.diff(Bptr.astype(np.int64))
    return int(blen[Acol].sum()) if len(Acol) else 0
