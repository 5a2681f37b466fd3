"""`spgemm --reuse N`: after the product, a values plan on C's pattern and N values-only calls;
their mean time on a line of its own, with --check the recomputed values against the product's
own (the reference 1e-9 rule of CSR::operator==).  The driver's other lines stay."""
import re
import subprocess
from pathlib import Path

import pytest

from _util import GOLDEN

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "mh-spgemm_amd" / "bin" / "spgemm"


def test_cli_reuse_needs_a_count():
    r = subprocess.run([str(CLI), "--reuse", str(GOLDEN / "cage4_like_A.mtx")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 255 and "Invalid Arguments." in r.stdout and "--reuse N" in r.stdout


@pytest.mark.gpu
def test_cli_reuse_check():
    r = subprocess.run([str(CLI), "--reuse", "3", "--check", str(GOLDEN / "cage4_like_A.mtx")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    m = re.search(r"^MH-SpGEMM values-only \(pattern reused\) mean of 3 calls is (\d+\.\d+)ms, Gflops is \d+\.\d+$", out, re.M)
    assert m and float(m.group(1)) > 0, out
    assert "\nvalues pass\n" in out, out
    # the lines tests/test_cli.py looks for
    assert "SpGEMM Start!!!" in out and "SpGEMM   End!!!" in out
    assert "MH-SpGEMM runtime is" in out and "rocsparse:" in out
    assert "\npass\n" in out, out
    assert out.index("MH-SpGEMM e2e") < out.index("values-only") < out.index("SpGEMM   End!!!")
