"""`spgemm --f32`, a modifier of --reuse, --masked and --grad: each chosen mode once more with an FP32 plan on
the operands' values rounded to float, beside an FP64 plan on the same rounded values -- one more line per
mode, and with --check every FP32 entry within 1.01 m 2^-24 S of the FP64 call's.  Without --f32 the driver
prints what it printed before."""
import re
import subprocess
from pathlib import Path

import pytest

from _util import GOLDEN

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "mh-spgemm_amd" / "bin" / "spgemm"
MTX = GOLDEN / "cage4_like_A.mtx"
MODES = ("values-only (pattern reused)", "masked (A's pattern)", "values backward (both gradients)")


def test_cli_f32_is_a_flag():
    r = subprocess.run([str(CLI), "--f32"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 255 and "Invalid Arguments." in r.stdout and "[--f32]" in r.stdout


@pytest.mark.gpu
def test_cli_f32_check():
    args = [str(CLI), "--reuse", "2", "--grad", "2", "--masked", "2"]
    r = subprocess.run(args + ["--f32", "--check", str(MTX)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    for mode in MODES:
        m = re.search(r"^MH-SpGEMM " + re.escape(mode) + r" FP32 median of 2 calls is (\d+\.\d+) ms, "
                      r"FP64 on the same rounded values (\d+\.\d+) ms$", out, re.M)
        assert m and float(m.group(1)) > 0 and float(m.group(2)) > 0, out
    for tag in ("values", "masked", "grad"):
        assert f"\n{tag} f32 pass\n" in out, out
    assert "f32 error" not in out
    # the FP64 modes' own lines stay, before the FP32 ones
    assert "\nvalues pass\n" in out and "\nmasked pass\n" in out and "\ngrad pass\n" in out and "\npass\n" in out, out
    assert out.index("\ngrad pass\n") < out.index("FP32 median") < out.index("SpGEMM   End!!!")
    # without --f32: the same lines but the FP32 ones (times aside)
    r0 = subprocess.run(args + ["--check", str(MTX)], capture_output=True, text=True, timeout=120)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    assert "FP32" not in r0.stdout and "f32" not in r0.stdout
    strip = lambda text: [re.sub(r"\d+\.\d+", "#", ln) for ln in text.splitlines()]  # noqa: E731
    kept = [ln for ln in strip(out) if "FP32" not in ln and " f32 " not in ln]
    assert kept == strip(r0.stdout)
