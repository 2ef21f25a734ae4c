"""CPU: the per-sample bin function of binned mutual information (correrender_amd/csrc/crf_binned_bins.h), which the
native binned-MI kernel on narrow members evaluates -- for u8 once per code into a 256-entry table -- gives, for every u8,
u16 and f16 code and a list of extrema and bin counts, the bin of the reference's lines evaluated step by step; its
reciprocal form agrees with its division form wherever a launcher may choose it; exactly the f16 NaN codes are skipped
under finite extrema (tests/native/narrow_bins.cpp, built with g++ -ffp-contract=off)."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_narrow_bins_every_code(tmp_path):
    exe = tmp_path / "narrow_bins"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror",
                    f"-I{ROOT / 'correrender_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "narrow_bins.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("OK narrow bins"), r.stdout
    assert "u8: 256 codes, 0 NaN" in r.stdout and "u16: 65536 codes, 0 NaN" in r.stdout
    assert "f16: 65536 codes, 2046 NaN" in r.stdout
