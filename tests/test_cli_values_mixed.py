"""`spgemm --f32 --acc64`: after each --f32 line the mode once more on a mixed plan -- float values, FP64 sums
(mhs_values_plan_create_accum) -- with one more line ("FP32, FP64 sums") and, with --check, the forward held to the
mixed plan's bound against the FP64 plan on the same float-rounded values, the backward to the FP32 bound.  Without
--acc64 the driver prints what it printed before."""
import re
import subprocess
from pathlib import Path

import pytest

from _util import GOLDEN

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "mh-spgemm_amd" / "bin" / "spgemm"
MTX = GOLDEN / "cage4_like_A.mtx"
MODES = ("values-only (pattern reused)", "masked (A's pattern)", "values backward (both gradients)")


def test_cli_acc64_is_a_modifier_of_f32():
    for args in (["--acc64"], ["--reuse", "2", "--acc64", str(MTX)]):  # no file; --acc64 without --f32
        r = subprocess.run([str(CLI)] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 255 and "Invalid Arguments." in r.stdout and "[--acc64]" in r.stdout, args


@pytest.mark.gpu
def test_cli_acc64_check():
    args = [str(CLI), "--f32", "--reuse", "3", "--masked", "3", "--grad", "3", "--check"]
    r = subprocess.run(args + ["--acc64", str(MTX)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    for mode in MODES:
        m = re.search(r"^MH-SpGEMM " + re.escape(mode) + r" FP32, FP64 sums median of 3 calls is (\d+\.\d+) ms, "
                      r"FP64 on the same rounded values (\d+\.\d+) ms$", out, re.M)
        assert m and float(m.group(1)) > 0 and float(m.group(2)) > 0, out
    for tag in ("values", "masked", "grad"):
        assert f"\n{tag} f32 acc64 pass\n" in out and f"\n{tag} f32 pass\n" in out, out
    assert "acc64 error" not in out and "f32 error" not in out
    # without --acc64: the same lines but the mixed ones (times aside)
    r0 = subprocess.run(args + [str(MTX)], capture_output=True, text=True, timeout=120)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    assert "FP64 sums" not in r0.stdout and "acc64" not in r0.stdout
    strip = lambda text: [re.sub(r"\d+\.\d+", "#", ln) for ln in text.splitlines()]  # noqa: E731
    kept = [ln for ln in strip(out) if "FP64 sums" not in ln and " acc64 " not in ln]
    assert kept == strip(r0.stdout)


@pytest.mark.gpu
def test_cli_acc64_batched():
    args = [str(CLI), "--f32", "--acc64", "--reuse", "2", "--grad", "2", "--batch", "5", "--width", "2", "--check", str(MTX)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    for what in ("values batched", "values grad batched"):
        m = re.search(r"^MH-SpGEMM " + what + r" FP32, FP64 sums \(5 sets, width 2\) median of 2 calls is (\d+\.\d+) ms, "
                      r"5 unbatched calls (\d+\.\d+) ms$", out, re.M)
        assert m and float(m.group(1)) > 0 and float(m.group(2)) > 0, out
    for tag in ("batched f32 acc64", "grad batched f32 acc64", "batched f32", "grad batched f32", "values f32 acc64", "grad f32 acc64"):
        assert f"\n{tag} pass\n" in out, out
    assert "acc64 error" not in out and "f32 error" not in out
