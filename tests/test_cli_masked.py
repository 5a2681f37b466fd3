"""`spgemm --masked N`: after the product, a masked plan (AUTO) of A*A on A's own pattern and N calls;
their mean time, the kept products and the dot rows on a line of its own, with --check the values
against the product's C filtered to A's pattern (the reference 1e-9 rule).  The driver's other lines stay."""
import re
import subprocess
from pathlib import Path

import pytest

from _util import GOLDEN

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "mh-spgemm_amd" / "bin" / "spgemm"


def test_cli_masked_needs_a_count():
    r = subprocess.run([str(CLI), "--masked", str(GOLDEN / "cage4_like_A.mtx")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 255 and "Invalid Arguments." in r.stdout and "--masked N" in r.stdout
    assert "--reuse N" in r.stdout


@pytest.mark.gpu
def test_cli_masked_check():
    r = subprocess.run([str(CLI), "--masked", "3", "--check", str(GOLDEN / "cage4_like_A.mtx")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    m = re.search(r"^MH-SpGEMM masked \(A's pattern\) mean of 3 calls is (\d+\.\d+) ms, kept (\d+) of (\d+) products, "
                  r"dot rows (\d+)$", out, re.M)
    assert m and float(m.group(1)) > 0, out
    assert 0 < int(m.group(2)) <= int(m.group(3))
    assert re.search(r"^SpGEMM intermediate result = %s$" % m.group(3), out, re.M), out
    assert "\nmasked pass\n" in out, out
    # the lines tests/test_cli.py looks for
    assert "SpGEMM Start!!!" in out and "SpGEMM   End!!!" in out
    assert "MH-SpGEMM runtime is" in out and "rocsparse:" in out
    assert "\npass\n" in out, out
    assert out.index("MH-SpGEMM e2e") < out.index("MH-SpGEMM masked") < out.index("SpGEMM   End!!!")
