"""`spgemm --reuse N --batch NB [--width W]`: NB seeded value sets in N batched calls on a plan of width W beside
N x NB unbatched calls on a width-1 plan -- one more line, and with --check every set of the batched call against
the unbatched call on the same values.  --batch is a modifier of --reuse and --width one of --batch; a bad NB or W
prints the usage message.  Without --batch the driver prints what it printed before."""
import re
import subprocess
from pathlib import Path

import pytest

from _util import GOLDEN

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "mh-spgemm_amd" / "bin" / "spgemm"
MTX = GOLDEN / "cage4_like_A.mtx"


@pytest.mark.parametrize("args", [
    ["--reuse", "2", "--batch"],                          # no NB
    ["--reuse", "2", "--batch", "0", str(MTX)],           # NB < 1
    ["--reuse", "2", "--batch", "-3", str(MTX)],
    ["--batch", "3", str(MTX)],                           # a modifier of --reuse
    ["--reuse", "2", "--width", "2", str(MTX)],           # a modifier of --batch
    ["--reuse", "2", "--batch", "3", "--width", "3", str(MTX)],  # not 1, 2 or 4
    ["--reuse", "2", "--batch", "3", "--width", "8", str(MTX)],
    ["--reuse", "2", "--batch", "3", "--width"],
], ids=lambda a: " ".join(x for x in a if x.startswith("-") or x.lstrip("-").isdigit()))
def test_cli_batch_argument_errors_print_usage(args):
    r = subprocess.run([str(CLI)] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 255 and "Invalid Arguments." in r.stdout, r.stdout
    assert "Usage:" in r.stdout and "[--batch NB] [--width W]" in r.stdout
    assert "SpGEMM Start" not in r.stdout  # refused before anything runs


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_cli_batch_check(f32):
    base = [str(CLI), "--reuse", "2"] + (["--f32"] if f32 else [])
    r = subprocess.run(base + ["--batch", "3", "--width", "2", "--check", str(MTX)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    for typ, tag in (("FP64", "batched"), ("FP32", "batched f32"))[: 2 if f32 else 1]:
        m = re.search(r"^MH-SpGEMM values batched " + typ + r" \(3 sets, width 2\) median of 2 calls is (\d+\.\d+) ms, "
                      r"3 unbatched calls (\d+\.\d+) ms$", out, re.M)
        assert m and float(m.group(1)) > 0 and float(m.group(2)) > 0, out
        assert f"\n{tag} pass\n" in out, out
    assert "batched error" not in out and "batched f32 error" not in out
    assert ("batched FP32" in out) == f32
    assert "\nvalues pass\n" in out and "\npass\n" in out, out  # the modes' own lines stay, before the batched ones
    assert out.index("\nvalues pass\n") < out.index("values batched") < out.index("SpGEMM   End!!!")
    # without --batch: the same lines but the batched ones (times aside)
    r0 = subprocess.run(base + ["--check", str(MTX)], capture_output=True, text=True, timeout=120)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    assert "batched" not in r0.stdout
    strip = lambda text: [re.sub(r"\d+\.\d+", "#", ln) for ln in text.splitlines()]  # noqa: E731
    assert [ln for ln in strip(out) if "batched" not in ln] == strip(r0.stdout)
