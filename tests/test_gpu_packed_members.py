"""GPU: the Pearson field from the packed member copy (crf_set_member_layout) against the raw members and the oracle, bit
for bit, and the lifetime of the copy (invalidation, AUTO's decisions)."""
import numpy as np
import pytest

from correrender_amd import Measure, synth
from parity import assert_bit_exact
import oracle_lib

pytestmark = pytest.mark.gpu


@pytest.fixture
def eng(engine):
    yield engine
    engine.set_member_layout("auto")


def _field(eng, members, ref, layout):
    """Pearson field of the bound members (torch [cs, zs, ys, xs]) under `layout`, as a host array."""
    import torch
    eng.set_member_layout(layout)
    out = torch.empty(members[0].numel(), dtype=torch.float32, device="cuda")
    eng.compute_device(Measure.PEARSON, out, ref)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_layouts(eng, oracle, ens, ref, what):
    import torch
    cs, zs, ys, xs = ens.shape
    eng.set_grid(xs, ys, zs, cs)
    members = torch.from_numpy(ens).cuda()
    eng.bind_members(members)
    raw = _field(eng, members, ref, "raw")
    assert eng.last_member_layout() == "raw"
    packed = _field(eng, members, ref, "packed")
    assert eng.last_member_layout() == "packed", what
    assert eng.last_kernel_name() == "pearson_reg_kernel"
    x, y, z = ref
    want = oracle.field(oracle_lib.PEARSON, ens, ens[:, z, y, x].copy())
    assert_bit_exact(raw, want, f"raw {what}")
    assert_bit_exact(packed, raw, f"packed vs raw {what}")
    return packed


@pytest.mark.parametrize("cs", [17, 31, 32, 33, 48, 50, 63, 64, 65, 100, 128])
def test_packed_member_counts(eng, oracle, cs):
    # 20*12*9 = 2160 voxels: 33 whole tiles and a ragged one; the last block has surplus waves
    ens = synth.box_ensemble(20, 12, 9, cs, seed=cs)
    _check_layouts(eng, oracle, ens, (5, 6, 4), f"cs={cs}")


@pytest.mark.parametrize("fallbacks", [0, 1, 2, 3, "all"])
def test_packed_special_values(eng, oracle, fallbacks):
    """+-0, denormals, NaN, +-Inf and segments wider than 15 binades: 0, 1, 2, 3 or all members of a tile fall back."""
    rng = np.random.default_rng(11)
    cs, n = 40, 64 * 7 + 13
    ens = (rng.standard_normal((cs, n)) * 3.0).astype(np.float32)
    ens[:, 130:140] = 0.0                                            # zeros: code 0
    ens[::3, 141:150] = -0.0
    ens[:, 150:160] = np.float32(1e-40) * rng.integers(1, 9, (cs, 10))  # denormals next to normals
    ens[5, 200:203] = np.float32(1e-38)                               # smallest normals beside O(1): falls back
    ens[7, 260] = np.inf                                              # falls back (and that voxel is NaN)
    ens[8, 330] = np.nan
    ens[9, 331] = -np.inf
    k = cs if fallbacks == "all" else fallbacks
    for e in range(k):                                                # a 2^30 spread inside one segment
        ens[e, 64 + e % 64] = np.float32(2.0 ** 30)
    ens = ens.reshape(cs, 1, 1, n)
    for ref in [(3, 0, 0), (70, 0, 0)]:
        _check_layouts(eng, oracle, ens, ref, f"fallbacks={fallbacks} ref={ref}")


def test_packed_wide_dynamic_range(eng, oracle):
    """Every member spans ~60 binades over the grid: most segments fit, some do not."""
    rng = np.random.default_rng(5)
    cs, n = 64, 64 * 40
    scale = np.exp2(rng.integers(-30, 30, (1, n))).astype(np.float32)
    ens = (rng.standard_normal((cs, n)).astype(np.float32) * scale).reshape(cs, 1, 1, n)
    _check_layouts(eng, oracle, ens, (17, 0, 0), "wide range")


def test_packed_unaligned_borrowed_views(eng, oracle):
    import torch
    cs, xs, ys, zs = 48, 13, 11, 7
    n = xs * ys * zs
    ens = synth.box_ensemble(xs, ys, zs, cs, seed=3)
    flat = torch.zeros(cs * n + 3, dtype=torch.float32, device="cuda")
    flat[1:1 + cs * n] = torch.from_numpy(ens.reshape(-1)).cuda()
    views = [flat[1 + c * n:1 + (c + 1) * n] for c in range(cs)]  # 4-byte aligned only
    eng.set_grid(xs, ys, zs, cs)
    eng.bind_members(views)
    ref = (2, 3, 4)
    raw = _field(eng, views, ref, "raw")
    packed = _field(eng, views, ref, "packed")
    assert eng.last_member_layout() == "packed"
    want = oracle.field(oracle_lib.PEARSON, ens, ens[:, 4, 3, 2].copy())
    assert_bit_exact(raw, want, "raw, unaligned views")
    assert_bit_exact(packed, want, "packed, unaligned views")


def test_packed_copy_follows_the_members(eng, oracle):
    """Writes into bound members: crf_members_changed (or a rebind) makes the next evaluation see them."""
    import torch
    cs, xs, ys, zs = 32, 16, 8, 8
    ens = synth.box_ensemble(xs, ys, zs, cs, seed=9)
    eng.set_grid(xs, ys, zs, cs)
    members = torch.from_numpy(ens).cuda()
    eng.bind_members(members)
    ref = (3, 3, 3)
    _field(eng, members, ref, "packed")
    ens2 = synth.box_ensemble(xs, ys, zs, cs, seed=10)
    members.copy_(torch.from_numpy(ens2))
    eng.members_changed()
    got = _field(eng, members, ref, "packed")
    assert eng.last_member_layout() == "packed"
    assert_bit_exact(got, oracle.field(oracle_lib.PEARSON, ens2, ens2[:, 3, 3, 3].copy()), "after crf_members_changed")
    other = torch.from_numpy(ens).cuda()
    eng.bind_members(other)
    got = _field(eng, other, ref, "packed")
    assert_bit_exact(got, oracle.field(oracle_lib.PEARSON, ens, ens[:, 3, 3, 3].copy()), "after a rebind")


def test_auto_layout_decisions(eng, oracle):
    """AUTO: a grid of 2^20 voxels at 64 members packs; one with too many wide segments declines; a small grid stays
    raw."""
    import torch
    cs, xs, ys, zs = 64, 128, 128, 64  # 2^20 voxels
    rng = np.random.default_rng(2)
    ens = rng.standard_normal((cs, zs, ys, xs)).astype(np.float32)
    eng.set_grid(xs, ys, zs, cs)
    members = torch.from_numpy(ens).cuda()
    eng.bind_members(members)
    ref = (1, 2, 3)
    want = oracle.field(oracle_lib.PEARSON, ens, ens[:, 3, 2, 1].copy())
    got = _field(eng, members, ref, "auto")
    assert eng.last_member_layout() == "packed"
    assert_bit_exact(got, want, "auto, packed")
    # every 8th voxel 2^40 larger: every segment spans more than 15 binades
    ens[:, :, :, ::8] *= np.float32(2.0 ** 40)
    members.copy_(torch.from_numpy(ens))
    eng.members_changed()
    want = oracle.field(oracle_lib.PEARSON, ens, ens[:, 3, 2, 1].copy())
    got = _field(eng, members, ref, "auto")
    assert eng.last_member_layout() == "raw"
    assert_bit_exact(got, want, "auto, declined")
    small = synth.box_ensemble(20, 12, 9, 32, seed=1)
    eng.set_grid(20, 12, 9, 32)
    t = torch.from_numpy(small).cuda()
    eng.bind_members(t)
    _field(eng, t, (1, 1, 1), "auto")
    assert eng.last_member_layout() == "raw"


@pytest.mark.parametrize("cs", [17, 24, 50, 60, 100])
def test_auto_stays_raw_where_the_copy_moves_more(eng, oracle, cs):
    """AUTO on a 2^20-voxel grid at member counts whose padded copy moves more than 92.5 % of the members' bytes."""
    import torch
    xs, ys, zs = 128, 128, 64
    rng = np.random.default_rng(cs)
    ens = rng.standard_normal((cs, zs, ys, xs)).astype(np.float32)
    eng.set_grid(xs, ys, zs, cs)
    members = torch.from_numpy(ens).cuda()
    eng.bind_members(members)
    got = _field(eng, members, (1, 2, 3), "auto")
    assert eng.last_member_layout() == "raw"
    assert_bit_exact(got, oracle.field(oracle_lib.PEARSON, ens, ens[:, 3, 2, 1].copy()), f"auto cs={cs}")
