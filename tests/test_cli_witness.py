"""`spgemm --witness N`: a modifier of --semiring NAME (not plus_times) with --reuse or --masked, like --subgrad N.
After each semiring values line it runs N witness calls on seeded values that tie: one more line per mode and type, and
with --check the call against a sequential host loop of the rule -- the smallest inner index among equal products."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "mh-spgemm_amd" / "bin" / "spgemm"


def write_mtx(path, n=300, per_row=6, seed=17):
    """A small square general matrix with a full diagonal (so that A*A on A's pattern keeps products)."""
    rng = np.random.default_rng(seed)
    key = np.unique(np.concatenate([np.arange(n) * n + np.arange(n), rng.integers(0, n * n, n * per_row)]))
    val = rng.uniform(0.5, 2.0, len(key))
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write(f"{n} {n} {len(key)}\n")
        for k, v in zip(key, val):
            f.write(f"{k // n + 1} {k % n + 1} {v:.17g}\n")
    return str(path)


def run(mtx, *args, timeout=120):
    return subprocess.run([str(CLI), *args, mtx], capture_output=True, text=True, timeout=timeout)


def test_cli_witness_usage_errors(tmp_path):
    mtx = write_mtx(tmp_path / "w.mtx", n=20, per_row=2)
    for args in (("--reuse", "2", "--witness", "2"),                               # no semiring to modify
                 ("--reuse", "2", "--semiring", "plus_times", "--witness", "2"),   # a sum has no witness
                 ("--semiring", "min_plus", "--witness", "2"),                     # no mode
                 ("--reuse", "2", "--semiring", "min_plus", "--witness", "0"),     # no calls
                 ("--reuse", "2", "--semiring", "min_plus", "--witness")):         # no count
        r = run(mtx, *args, timeout=60)
        assert r.returncode == 255 and "Invalid Arguments." in r.stdout and "[--witness N]" in r.stdout, args
        assert "[--subgrad N]" in r.stdout and "SpGEMM Start" not in r.stdout


@pytest.mark.gpu
def test_cli_witness_check(tmp_path):
    mtx = write_mtx(tmp_path / "w.mtx")
    r = run(mtx, "--reuse", "2", "--masked", "2", "--semiring", "min_plus", "--witness", "2", "--f32", "--check")
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    for label, tag in (("values-only (pattern reused)", "values"), ("masked (A's pattern)", "masked")):
        for ty, suffix in (("FP64", ""), ("FP32", " f32")):
            m = re.search(r"^MH-SpGEMM %s min_plus witness %s median of 2 calls is (\d+\.\d+) ms$" % (re.escape(label), ty),
                          out, re.M)
            assert m and float(m.group(1)) > 0, out
            assert f"\n{tag} min_plus{suffix} witness pass\n" in out, out
            assert f"\n{tag} min_plus{suffix} pass\n" in out, out  # the mode it follows
            assert out.index(f"\n{tag} min_plus{suffix} pass\n") < out.index(f"\n{tag} min_plus{suffix} witness pass\n")
    assert out.count("witness pass") == 4 and "error" not in out, out
