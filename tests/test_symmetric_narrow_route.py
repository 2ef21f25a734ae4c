"""CPU: at which (member format, member count) the symmetric Pearson field reads two narrow fields as stored.
symmetric_narrow_routed (correrender_amd/csrc/symmetric_narrow_route.h, no HIP in it) decides it for api.cpp and for the
launcher; a small host program (tests/native/symmetric_narrow_route.cpp, plain g++, no GPU) prints the table over formats
-1..5 x 0..300 members, and this test compares it line by line with the rule below, which states the table on its own and
does not call the C++.  tests/test_gpu_narrow_secondary.py asserts the kernel that actually ran against the same table."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

F32, U8, U16, F16 = range(4)
# 65..128 members: the N = members rounded up to 16 that profiles/narrow_symmetric_ab.md measured no slower than the copy route
ROUTED_ABOVE_64 = {U8: {80, 96, 112, 128}, U16: {80, 96, 112, 128}, F16: {80, 96, 112, 128}}


def routed_rule(fmt, cs):
    if fmt not in (U8, U16, F16) or cs < 2 or cs > 128:
        return False
    return cs <= 64 or (cs + 15) // 16 * 16 in ROUTED_ABOVE_64[fmt]


def test_cpp_table_matches_the_documented_rule(tmp_path):
    exe = tmp_path / "symmetric_narrow_route"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'correrender_amd' / 'csrc'}",
                    str(ROOT / "tests" / "native" / "symmetric_narrow_route.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == 7 * 301
    table = {}
    for line in lines:
        fmt, cs, routed = (int(v) for v in line.split())
        table[fmt, cs] = bool(routed)
        assert bool(routed) == routed_rule(fmt, cs), line
    # what every later change of the measured part of the table has to keep
    for fmt in (U8, U16, F16):
        assert all(table[fmt, cs] for cs in range(2, 65)), "every narrow format is routed at 2..64 members"
        assert not table[fmt, 0] and not table[fmt, 1] and not any(table[fmt, cs] for cs in range(129, 301))
    for fmt in (-1, F32, 4, 5):
        assert not any(table[fmt, cs] for cs in range(0, 301)), "fp32 and unknown formats are never routed"
