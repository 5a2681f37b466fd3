"""`spgemm --grad N`: after the product, a values plan on C's pattern and, with a seeded cotangent, N
values calls and N backward calls; the two median times on a line of its own, with --check the adjoint
identities <G, C> = <dA, Aval> = <dB, Bval> on host-computed sums.  The driver's other lines stay."""
import re
import subprocess
from pathlib import Path

import pytest

from _util import GOLDEN

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "mh-spgemm_amd" / "bin" / "spgemm"


def test_cli_grad_needs_a_count():
    r = subprocess.run([str(CLI), "--grad", str(GOLDEN / "cage4_like_A.mtx")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 255 and "Invalid Arguments." in r.stdout and "--grad N" in r.stdout
    r = subprocess.run([str(CLI), "--grad", "-1", str(GOLDEN / "cage4_like_A.mtx")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 255 and "Invalid Arguments." in r.stdout


@pytest.mark.gpu
def test_cli_grad_check():
    r = subprocess.run([str(CLI), "--grad", "3", "--check", str(GOLDEN / "cage4_like_A.mtx")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    m = re.search(r"^MH-SpGEMM values backward \(both gradients\) median of 3 calls is (\d+\.\d+) ms, "
                  r"the values call's (\d+\.\d+) ms$", out, re.M)
    assert m and float(m.group(1)) > 0 and float(m.group(2)) > 0, out
    s = re.search(r"^<G,C> = (\S+), <dA,A> = (\S+), <dB,B> = (\S+)$", out, re.M)
    assert s, out
    gc, ga, gb = (float(x) for x in s.groups())
    assert gc != 0.0 and abs(gc - ga) <= 1e-9 * abs(gc) and abs(gc - gb) <= 1e-9 * abs(gc), out
    assert "\ngrad pass\n" in out, out
    # the lines tests/test_cli.py looks for
    assert "SpGEMM Start!!!" in out and "SpGEMM   End!!!" in out
    assert "MH-SpGEMM runtime is" in out and "rocsparse:" in out
    assert "\npass\n" in out, out
    assert out.index("MH-SpGEMM e2e") < out.index("values backward") < out.index("SpGEMM   End!!!")
