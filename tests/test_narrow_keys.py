"""CPU: the order keys of the narrow member formats (correrender_amd/csrc/crf_narrow_keys.h), which the native Kendall
kernel sorts instead of the converted values, agree with the float order, float equality and NaN-ness of the converted
values for every u8, u16 and f16 code; the pad key lies above them all (tests/native/narrow_keys.cpp, built with g++)."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_narrow_keys_every_code(tmp_path):
    exe = tmp_path / "narrow_keys"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{ROOT / 'correrender_amd' / 'csrc'}",
                    str(ROOT / "tests" / "native" / "narrow_keys.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("OK narrow keys"), r.stdout
    assert "f16: 65536 codes, 2046 NaN" in r.stdout
