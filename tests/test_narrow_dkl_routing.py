"""CPU: the routing table of native DKL on narrow members.  dkl_narrow_routed (correrender_amd/csrc/crf_internal.h, constexpr)
decides in api.cpp whether a DKL call reads uint8 / uint16 / float16 members as stored; tests/test_gpu_narrow_dkl.py asserts
the kernel that ran against its own routed_native.  A small host program (tests/native/dkl_narrow_routing.cpp, built with g++
against the HIP headers, no GPU) prints the C++ table over formats x 1..2048 members x estimators x k, and this test
compares it with the Python one line by line, so the two cannot drift apart."""
import os
import subprocess
from pathlib import Path

from test_gpu_narrow_dkl import routed_native

ROOT = Path(__file__).resolve().parent.parent
FORMAT_NAMES = {0: "f32", 1: "u8", 2: "u16", 3: "f16", 4: "unknown"}


def test_cpp_and_python_routing_tables_agree(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "dkl_narrow_routing"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include",
                    f"-I{ROOT / 'correrender_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "dkl_narrow_routing.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == 5 * 2048 * 2 * 5
    native = 0
    for line in lines:
        fmt, cs, estimator, k, routed = map(int, line.split())
        assert bool(routed) == bool(routed_native(FORMAT_NAMES[fmt], cs, estimator, k)), line
        native += routed
    assert native > 0  # something is routed native
    assert not any(line.startswith(("0 ", "4 ")) and line.endswith(" 1") for line in lines)  # never fp32 / an unknown id
