"""CPU: the Kraskov dispatch (correrender_amd/csrc/kraskov_plan.h) -- which kernel family and instantiation runs for a
member count, a k and the six CRF_KRASKOV_* switches.  The header is plain C++17: a small program compiled with g++
prints the plan for every case given on its standard input, and the expected plans below were derived from the launchers
as they were before the plan function existed (the thresholds are measured ones)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

MAIN = r"""
#include <cstdio>
#include "kraskov_plan.h"
int main() {  // per line: entry (0 field, 1 field beyond 128 members, 2 symmetric) cs k sorted direct tile dxt ti4 stage
    int entry, cs, k;
    crf::KraskovSwitches s;
    while (std::scanf("%d %d %d %d %d %d %d %d %d", &entry, &cs, &k, &s.sorted, &s.direct, &s.tile, &s.dxt, &s.ti4, &s.stage) == 9) {
        crf::KraskovPlan p{};
        const bool ok = entry == 2 ? crf::kraskov_symmetric_plan(cs, k, &p) : crf::kraskov_field_plan(cs, k, entry == 1, s, &p);
        const char* family = p.family == crf::KraskovFamily::Column ? "Column" : p.family == crf::KraskovFamily::Direct ? "Direct" : "Sorted";
        if (!ok) std::printf("unsupported\n");
        else if (p.NS) std::printf("%s K%d NS%d\n", family, p.K, p.NS);
        else std::printf("%s K%d TI%d%s%s\n", family, p.K, p.TI, p.dxt ? " dxt" : "", p.stage ? " stage" : "");
    }
}
"""

FIELD, BEYOND_128, SYMMETRIC = 0, 1, 2
SWITCHES = ("sorted", "direct", "tile", "dxt", "ti4", "stage")  # -1 unset, 0, 1, 2 = any other first character


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kraskov_plan")
    (tmp / "main.cpp").write_text(MAIN)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'correrender_amd' / 'csrc'}", str(tmp / "main.cpp"),
                    "-o", str(tmp / "plan")], check=True)

    def run(cases):
        lines = "".join(f"{entry} {cs} {k} " + " ".join(str(sw.get(name, -1)) for name in SWITCHES) + "\n"
                        for entry, cs, k, sw in cases)
        out = subprocess.run([str(tmp / "plan")], input=lines, capture_output=True, text=True, check=True).stdout
        result = out.splitlines()
        assert len(result) == len(cases)
        return result
    return run


DIRECT = dict(direct=1)
TILE = dict(tile=1)
SORTED = dict(sorted=1)
CASES = [
    # defaults: the LDS-column kernel at few members, the tile-free kernel beyond the measured crossovers
    (FIELD, 32, 3, {}, "Column K3 TI8 dxt"),
    (FIELD, 40, 3, {}, "Column K3 TI8"),
    (FIELD, 41, 3, {}, "Direct K3 TI4 dxt stage"),
    (FIELD, 64, 3, {}, "Direct K3 TI4 dxt stage"),
    (FIELD, 65, 3, {}, "Direct K3 TI4 dxt"),
    (FIELD, 44, 2, {}, "Column K2 TI8"),
    (FIELD, 45, 2, {}, "Direct K2 TI8 dxt"),
    (FIELD, 64, 2, {}, "Direct K2 TI8 dxt"),
    (FIELD, 28, 4, {}, "Column K4 TI4 dxt"),
    (FIELD, 30, 4, {}, "Direct K4 TI4 dxt stage"),
    (FIELD, 36, 4, {}, "Column K4 TI4"),
    (FIELD, 37, 4, {}, "Direct K4 TI4 dxt stage"),
    # the x-distance table: up to 112 members for every k, up to 128 for k = 2, 4, never beyond
    (FIELD, 112, 3, {}, "Direct K3 TI4 dxt"),
    (FIELD, 113, 3, {}, "Direct K3 TI8"),
    (FIELD, 113, 4, {}, "Direct K4 TI4 dxt"),
    (FIELD, 128, 2, {}, "Direct K2 TI8 dxt"),
    (BEYOND_128, 129, 4, {}, "Direct K4 TI4"),
    (BEYOND_128, 129, 1, {}, "Direct K1 TI8"),
    (FIELD, 129, 4, {}, "Direct K4 TI4"),
    # k beyond 4 rounds up to the next instantiated K; min(k, cs - 1) counts
    (FIELD, 64, 5, {}, "Direct K8 TI4"),
    (FIELD, 64, 12, {}, "Direct K16 TI2"),
    (FIELD, 20, 20, {}, "Direct K32 TI1"),
    (FIELD, 100, 40, {}, "Direct K64 TI1"),
    (BEYOND_128, 160, 70, {}, "Direct K128 TI1"),
    (BEYOND_128, 200, 150, {}, "unsupported"),
    # the three tables of cs doubles beside the 20480 bytes of partial sums: 61424 bytes at 1706 members, 61448 at 1707,
    # against 60 KiB = 61440
    (BEYOND_128, 1706, 3, {}, "Direct K3 TI8"),
    (BEYOND_128, 1706, 128, {}, "Direct K128 TI1"),
    (BEYOND_128, 1707, 3, {}, "unsupported"),
    (BEYOND_128, 1707, 128, {}, "unsupported"),
    # CRF_KRASKOV_DIRECT=1 with _STAGE, _DXT, _TI4
    (FIELD, 20, 3, DIRECT, "Direct K3 TI4 dxt stage"),
    (FIELD, 20, 1, dict(DIRECT, stage=0), "Direct K1 TI8 dxt"),
    (FIELD, 20, 1, dict(DIRECT, stage=1), "Direct K1 TI4 dxt stage"),
    (FIELD, 48, 3, dict(DIRECT, dxt=0, ti4=1), "Direct K3 TI4"),
    (FIELD, 48, 4, dict(DIRECT, dxt=0, ti4=0), "Direct K4 TI8"),
    (FIELD, 48, 2, dict(DIRECT, dxt=1, ti4=1), "Direct K2 TI4 dxt"),
    # a first character other than 0 or 1: _TI4 and _STAGE count as set and not 1, _DXT as unset
    (FIELD, 48, 4, dict(DIRECT, dxt=0, ti4=2), "Direct K4 TI8"),
    (FIELD, 48, 3, dict(DIRECT, stage=2), "Direct K3 TI4 dxt"),
    (FIELD, 113, 3, dict(dxt=2), "Direct K3 TI8"),
    # CRF_KRASKOV_TILE=1: 16 points per sweep beyond 56 members where they fill the last sweep
    (FIELD, 64, 3, TILE, "Column K3 TI16"),
    (FIELD, 57, 2, TILE, "Column K2 TI16"),
    (FIELD, 63, 3, TILE, "Column K3 TI16"),
    (FIELD, 72, 3, TILE, "Column K3 TI8"),
    (FIELD, 64, 1, TILE, "Column K1 TI8"),
    (FIELD, 48, 3, dict(TILE, dxt=1), "Column K3 TI8 dxt"),
    (FIELD, 64, 3, dict(TILE, dxt=1), "Column K3 TI16"),
    (FIELD, 81, 3, TILE, "Direct K3 TI4 dxt"),
    # CRF_KRASKOV_SORTED=1: up to 64 members and k <= 4 only, and CRF_KRASKOV_DIRECT=1 wins
    (FIELD, 32, 3, SORTED, "Sorted K3 NS32"),
    (FIELD, 33, 3, SORTED, "Sorted K3 NS48"),
    (FIELD, 64, 4, SORTED, "Sorted K4 NS64"),
    (FIELD, 65, 3, SORTED, "Direct K3 TI4 dxt"),
    (FIELD, 48, 3, dict(SORTED, direct=1), "Direct K3 TI4 dxt stage"),
    (FIELD, 64, 5, SORTED, "Direct K8 TI4"),
    (FIELD, 48, 3, dict(sorted=0), "Direct K3 TI4 dxt stage"),
    # symmetric field mode: no table, 8 points per sweep up to k = 4, k <= 64
    (SYMMETRIC, 64, 3, {}, "Direct K3 TI8"),
    (SYMMETRIC, 64, 4, {}, "Direct K4 TI8"),
    (SYMMETRIC, 100, 20, {}, "Direct K32 TI1"),
    (SYMMETRIC, 100, 64, {}, "Direct K64 TI1"),
    (SYMMETRIC, 100, 70, {}, "unsupported"),
    (SYMMETRIC, 1706, 3, {}, "Direct K3 TI8"),
    (SYMMETRIC, 1707, 3, {}, "unsupported"),
]


def test_plan_table(plans):
    got = plans([case[:4] for case in CASES])
    wrong = [f"{case[:4]}: {g}, expected {case[4]}" for case, g in zip(CASES, got) if g != case[4]]
    assert not wrong, "\n".join(wrong)


def test_default_plans_up_to_130_members(plans):
    """Without switches, through the entry that the member count takes: K = min(k, cs - 1) exactly up to 4, a staged tile
    only together with the distance table, the LDS-column kernel only up to 80 members, every plan supported."""
    cases = [(FIELD if cs <= 128 else BEYOND_128, cs, k, {}) for cs in range(2, 131) for k in range(1, 9)]
    for (_, cs, k, _), plan in zip(cases, plans(cases)):
        what = f"cs={cs} k={k}: {plan}"
        family, K, TI, *flags = plan.split()
        K, kk = int(K[1:]), min(k, cs - 1)
        assert family in ("Column", "Direct"), what
        assert K == (kk if kk <= 4 else 8), what  # never the K = 0 any-k form, which is gone
        assert "stage" not in flags or "dxt" in flags, what
        assert family != "Column" or cs <= 80, what
