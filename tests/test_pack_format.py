"""CPU: the packed member format (correrender_amd/csrc/crf_internal.h) round-trips exhaustively -- every 2^32 bit
pattern against one base, every exponent against every base (tests/native/pack_roundtrip.cpp, built with g++)."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_pack_format_roundtrip(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "pack_roundtrip"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include",
                    f"-I{ROOT / 'correrender_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "pack_roundtrip.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK 268435456 fitting patterns"), r.stdout
