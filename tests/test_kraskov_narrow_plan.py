"""CPU: which Kraskov field calls on narrow members (uint8, uint16, float16) run on the members as stored --
kraskov_narrow_plan in correrender_amd/csrc/kraskov_plan.h.  The header is plain C++17: a small program compiled with g++
prints, for every case on its standard input, the narrow plan next to the field plan.  A native call must add its fp64
partial sums in the fp32 call's order, so whenever the narrow plan says yes its family, K, TI and dxt are the field
plan's, under every CRF_KRASKOV_* switch; and the routed set is the "within rule" column of
profiles/narrow_kraskov_ab.md, written out again below."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

MAIN = r"""
#include <cstdio>
#include "kraskov_plan.h"
static void print(bool ok, const crf::KraskovPlan& p) {
    const char* family = p.family == crf::KraskovFamily::Column ? "Column" : p.family == crf::KraskovFamily::Direct ? "Direct" : "Sorted";
    if (!ok) std::printf("no");
    else std::printf("%s K%d TI%d%s", family, p.K, p.TI, p.dxt ? " dxt" : "");
}
int main() {  // per line: format cs k sorted direct tile dxt ti4 stage -> "<narrow plan> | <field plan>"
    int format, cs, k;
    crf::KraskovSwitches s;
    while (std::scanf("%d %d %d %d %d %d %d %d %d", &format, &cs, &k, &s.sorted, &s.direct, &s.tile, &s.dxt, &s.ti4, &s.stage) == 9) {
        crf::KraskovPlan narrow{}, field{};
        const bool native = crf::kraskov_narrow_plan(format, cs, k, s, &narrow);
        const bool ok = cs >= 2 && crf::kraskov_field_plan(cs, k, false, s, &field);
        print(native, narrow);
        std::printf(" | ");
        print(ok, field);
        std::printf("\n");
    }
}
"""

F32, U8, U16, F16 = 0, 1, 2, 3  # crf_member_format
FORMATS = {"u8": U8, "u16": U16, "f16": F16}
SWITCH_NAMES = ("sorted", "direct", "tile", "dxt", "ti4", "stage")  # -1 unset, 0, 1
SWITCH_SETTINGS = [{}, dict(direct=1), dict(tile=1), dict(dxt=0), dict(dxt=1), dict(ti4=0), dict(ti4=1), dict(stage=0),
                   dict(stage=1), dict(direct=1, dxt=0, ti4=1), dict(direct=1, stage=1, ti4=0), dict(tile=1, dxt=1)]

# The routed cells of profiles/narrow_kraskov_ab.md ("Routing"): per format, kernel family and K, the member counts
# rounded up to a multiple of 16 that run native.  K = min(k, members - 1) up to 4, and 8 for 5..8; K = 16 uses scratch,
# K = 32, 64, 128 were not measured: they stay on the copy, like every (family, K) that is not listed.
ROUTED = {
    "u8": {("Column", 2): {48}, ("Column", 3): {48},
           ("Direct", 2): {64}, ("Direct", 3): {64, 80, 96}, ("Direct", 4): {128}, ("Direct", 8): {64, 128}},
    "u16": {("Direct", 2): {64}, ("Direct", 3): {64}, ("Direct", 4): {128}, ("Direct", 8): {128}},
    "f16": {("Direct", 2): {64}, ("Direct", 3): {64, 128}, ("Direct", 4): {128}, ("Direct", 8): {64, 128}},
}


def routed(fmt, cs, field_plan):
    """What the profile's table says of a field plan ("Column K3 TI8 dxt", ...) at cs members of format fmt."""
    family, K = field_plan.split()[0], int(field_plan.split()[1][1:])
    return (cs + 15) // 16 * 16 in ROUTED[fmt].get((family, K), set())


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kraskov_narrow_plan")
    (tmp / "main.cpp").write_text(MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'correrender_amd' / 'csrc'}",
                    str(tmp / "main.cpp"), "-o", str(tmp / "plan")], check=True)

    def run(cases):
        lines = "".join(f"{fmt} {cs} {k} " + " ".join(str(sw.get(name, -1)) for name in SWITCH_NAMES) + "\n"
                        for fmt, cs, k, sw in cases)
        out = subprocess.run([str(tmp / "plan")], input=lines, capture_output=True, text=True, check=True).stdout
        result = [tuple(line.split(" | ")) for line in out.splitlines()]
        assert len(result) == len(cases)
        return result
    return run


def test_a_native_plan_is_the_field_plan_under_every_switch(plans):
    cases = [(f, cs, k, sw) for f in FORMATS.values() for cs in range(2, 129) for k in range(1, cs + 3)
             for sw in SWITCH_SETTINGS]
    native = 0
    for case, (narrow, field) in zip(cases, plans(cases)):
        assert field != "no", case  # every field plan up to 128 members is supported
        assert narrow in ("no", field), f"{case}: narrow plan {narrow}, field plan {field}"
        native += narrow != "no"
    assert native > 0


def test_the_routed_set_is_the_profiles_table(plans):
    cases = [(f, cs, k, sw) for f in FORMATS for cs in range(2, 129) for k in range(1, cs + 3) for sw in SWITCH_SETTINGS]
    got = plans([(FORMATS[f], cs, k, sw) for f, cs, k, sw in cases])
    wrong = [f"{case}: {narrow}, field plan {field}" for case, (narrow, field) in zip(cases, got)
             if (narrow != "no") != routed(case[0], case[1], field)]
    assert not wrong, "\n".join(wrong[:20])


def test_the_sorted_family_stays_on_the_copy(plans):
    cases = [(f, cs, k, dict(sorted=1)) for f in FORMATS.values() for cs in (2, 32, 33, 48, 64) for k in (1, 3, 4)]
    for case, (narrow, field) in zip(cases, plans(cases)):
        assert field.startswith("Sorted") and narrow == "no", f"{case}: {narrow} | {field}"
    # where CRF_KRASKOV_SORTED=1 does not reach the sorted kernel the call is routed as without it
    cases = [(f, cs, k, sw) for f in FORMATS.values() for cs, k, sw in [(65, 3, dict(sorted=1)), (64, 5, dict(sorted=1)),
                                                                       (48, 3, dict(sorted=1, direct=1))]]
    plain = plans([(f, cs, k, {name: v for name, v in sw.items() if name != "sorted"}) for f, cs, k, sw in cases])
    assert plans(cases) == plain


def test_outside_the_native_range(plans):
    cases = [(f, cs, k, sw) for f in FORMATS.values() for cs in (1, 129, 130, 1000) for k in (1, 3, 8)
             for sw in SWITCH_SETTINGS]
    cases += [(F32, cs, k, sw) for cs in range(2, 129) for k in (1, 2, 3, 4, 8, 16) for sw in SWITCH_SETTINGS]
    cases += [(f, 64, 3, {}) for f in (-1, 4, 7)]
    for case, (narrow, _) in zip(cases, plans(cases)):
        assert narrow == "no", case
