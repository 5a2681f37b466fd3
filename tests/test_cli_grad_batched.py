"""`spgemm --reuse N --grad N --batch NB [--width W]`: beside the batched values lines, NB seeded cotangent sets in N
calls of mhs_spgemm_values_grad_batched on the plan of width W and N x NB unbatched backward calls on a width-1 plan
-- one more line per type, and with --check every set of both gradients against the unbatched backward on that set.
Every new line contains "batched"; without --batch the driver prints what it printed before."""
import re
import subprocess
from pathlib import Path

import pytest

from _util import GOLDEN

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "mh-spgemm_amd" / "bin" / "spgemm"
MTX = GOLDEN / "cage4_like_A.mtx"


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("width", [2, 4])
def test_cli_grad_batch_check(width, f32):
    base = [str(CLI), "--reuse", "2", "--grad", "3"] + (["--f32"] if f32 else [])
    r = subprocess.run(base + ["--batch", "5", "--width", str(width), "--check", str(MTX)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    for typ, tag in (("FP64", "grad batched"), ("FP32", "grad batched f32"))[: 2 if f32 else 1]:
        m = re.search(r"^MH-SpGEMM values grad batched " + typ + rf" \(5 sets, width {width}\) median of 3 calls is (\d+\.\d+) ms, "
                      r"5 unbatched calls (\d+\.\d+) ms$", out, re.M)
        assert m and float(m.group(1)) > 0 and float(m.group(2)) > 0, out
        assert f"\n{tag} pass\n" in out, out
    assert "batched error" not in out and "batched f32 error" not in out
    assert ("grad batched FP32" in out) == f32
    # the modes' own lines stay, before the batched ones; the backward's batched lines follow the forward's
    assert "\nvalues pass\n" in out and "\ngrad pass\n" in out and "\nbatched pass\n" in out, out
    assert out.index("\ngrad pass\n") < out.index("values batched") < out.index("values grad batched") < out.index("SpGEMM   End!!!")
    # without --batch: the same lines but the batched ones (times aside)
    r0 = subprocess.run(base + ["--check", str(MTX)], capture_output=True, text=True, timeout=120)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    assert "batched" not in r0.stdout
    strip = lambda text: [re.sub(r"\d+\.\d+(e[+-]\d+)?", "#", ln) for ln in text.splitlines()]  # noqa: E731
    assert [ln for ln in strip(out) if "batched" not in ln] == strip(r0.stdout)
    # without --grad: no backward line among the batched ones
    r1 = subprocess.run([str(CLI), "--reuse", "2", "--batch", "5", "--width", str(width), "--check", str(MTX)], capture_output=True,
                        text=True, timeout=120)
    assert r1.returncode == 0 and "values batched" in r1.stdout and "grad batched" not in r1.stdout, r1.stdout
