"""CPU: which kernel evaluates a measure between two member vectors per item -- the symmetric field mode and pair requests.
two_vector_route (correrender_amd/csrc/two_vector_route.h, no HIP in it) decides it for api.cpp; a small host program
(tests/native/two_vector_route.cpp, plain g++, no GPU) prints that table over both modes x the seven measures x 1..2048
members x k x num_bins x the force switch, and this test compares it line by line with two_vector_rule below, which states
the documented rules on its own and does not call the C++.  tests/test_gpu_two_vector_route.py
asserts the kernel that actually ran against the same function."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

PEARSON, SPEARMAN, KENDALL, MI_BINNED, MI_KRASKOV, BINNED_MI_CC, KMI_CC = range(7)
ROUTES = ("Fill", "PearsonRegister", "KraskovDirect", "Sorted", "DirectSymmetric", "PairRequest")
# the routes each mode can take at all
ROUTES_OF_MODE = {False: set(ROUTES), True: {"PearsonRegister", "Sorted", "PairRequest"}}


def _sortable(measure, cs, num_bins):
    """The sort-based kernels: 2..128 members; the binned measures need bin codes of one byte."""
    if not 2 <= cs <= 128:
        return False
    return measure in (SPEARMAN, KENDALL) or (measure in (MI_BINNED, BINNED_MI_CC) and 1 <= num_bins <= 255)


def _kraskov_direct(cs, k):
    """The symmetric tile-free Kraskov kernel: at most 64 neighbours kept (min(k, members - 1)) and three tables of `members`
    doubles beside 20 KiB of partial sums within 60 KiB of LDS."""
    return min(k, cs - 1) <= 64 and 24 * cs + 20480 <= 60 * 1024


def two_vector_rule(requests, measure, cs, k=0, num_bins=0, force=False):
    """(route, reported kernel name).  requests: pair-request mode, else symmetric field mode; force:
    CRF_REQUESTS_GENERIC=1 / CRF_SYMMETRIC_DIRECT=1."""
    if requests:
        if not force and measure == PEARSON and 2 <= cs <= 128:
            return "PearsonRegister", "pearson_request_kernel"
        if not force and _sortable(measure, cs, num_bins):
            return "Sorted", "sorted_request_kernel"
        return "PairRequest", "pair_request_kernel"      # both Kraskov measures, one member, more than 128, the switch
    if measure == PEARSON:
        if cs == 1:
            return "Fill", "pearson_symmetric_kernel"
        return ("PearsonRegister", "pearson_symmetric_kernel") if cs <= 128 else ("PairRequest", "pair_request_kernel")
    if measure in (MI_KRASKOV, KMI_CC):
        if cs == 1:
            return "Fill", "kraskov_direct_kernel"
        return ("KraskovDirect", "kraskov_direct_kernel") if _kraskov_direct(cs, k) else ("PairRequest", "pair_request_kernel")
    if not force and _sortable(measure, cs, num_bins):   # the switch skips the sort-based kernels, nothing else
        return "Sorted", "sorted_symmetric_kernel"
    return "DirectSymmetric", "direct_symmetric_kernel"


def test_cpp_route_matches_the_documented_rules(tmp_path):
    exe = tmp_path / "two_vector_route"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'correrender_amd' / 'csrc'}",
                    str(ROOT / "tests" / "native" / "two_vector_route.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == 2 * 7 * 2048 * 6 * 5 * 2
    seen = {False: set(), True: set()}
    for line in lines:
        mode, measure, cs, k, num_bins, force, route, name = line.split()
        want = two_vector_rule(mode == "1", int(measure), int(cs), int(k), int(num_bins), force == "1")
        assert (route, name) == want, line
        seen[mode == "1"].add(route)
    assert seen == ROUTES_OF_MODE
