"""GPU: the state of a context behind its kernels -- everything it derives from the members follows the members, and a
context gives its device memory back.

1. Derived state.  A context keeps a min/max cache per member set, a packed copy (Pearson field), an fp32 copy of narrow
members, and per-range member tables for host output above 8 MiB.  Each test builds one of them, replaces the data in every
way that applies -- upload, bind, a narrow upload, a narrow bind, overwriting bound members in place followed by
members_changed() -- and asks that the next result be the oracle's on the NEW data, bit for bit (member_minmax: numpy's).
Every step carries its own data, so a result served from state of the step before cannot pass.

2. Lifecycle.  Ten contexts are created, driven through every lazily allocated buffer and closed; the free device memory
after the tenth may be lower than after the second by at most one fp32 member block of the large grid."""
import numpy as np
import pytest
import torch

import correrender_amd as ca
from correrender_amd import Measure
from parity import assert_bit_exact
import oracle_lib
from test_gpu_member_formats import cast, convert, to_device, to_device_members

pytestmark = pytest.mark.gpu

SMALL, SMALL_CS, SMALL_REF = (16, 8, 4), 24, (5, 3, 2)
LARGE, LARGE_CS, LARGE_REF = (160, 128, 103), 8, (83, 63, 51)  # the smallest result above 8 MiB: the ranged host path


def make(grid, cs, step, fmt="f32"):
    """Data of step `step`: [cs, zs, ys, xs], values in [0, 0.3 + 0.1 * step) -- no two steps share their extrema."""
    xs, ys, zs = grid
    ens01 = np.random.default_rng(1000 + step).random((cs, zs, ys, xs), dtype=np.float32) * np.float32(0.3 + 0.1 * step)
    return ens01 if fmt == "f32" else cast(ens01, fmt)


def values(data):
    return data if data.dtype == np.float32 else convert(data)


class Members:
    """Replaces the primary members of `engine` in one of the ways under test."""

    def __init__(self, engine):
        self.engine, self.bound = engine, None

    def replace(self, how, data):
        cs = data.shape[0]
        if how == "upload":
            self.engine.upload_members(data)
            self.bound = None
        elif how == "bind":
            self.bound = to_device_members(data) if data.dtype != np.float32 else to_device(data.reshape(cs, -1))
            self.engine.bind_members(self.bound)
        else:  # in place: same tensors, new values
            assert how == "overwrite" and self.bound is not None and self.bound.shape[1] == data[0].size
            new = to_device(data.reshape(cs, -1))
            if new.dtype == torch.uint16:  # (a plain copy, whatever the torch release implements for uint16)
                self.bound.view(torch.int16).copy_(new.view(torch.int16))
            else:
                self.bound.copy_(new)
            torch.cuda.synchronize()
            self.engine.members_changed()


# (how, format) of every step; "overwrite" follows the "bind" of the same format
STEPS = [("upload", "f32"), ("bind", "f32"), ("overwrite", "f32"), ("upload", "u16"), ("bind", "u16"), ("overwrite", "u16"),
         ("upload", "f32")]


def check_field(engine, oracle, measure, om, data, ref, what, device=False):
    wide = values(data)
    x, y, z = ref
    want = oracle.field(om, wide, wide[:, z, y, x].copy())
    if device:
        out = torch.empty(wide[0].size, dtype=torch.float32, device="cuda")
        engine.compute_device(measure, out, ref)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
    else:
        got = engine.compute(measure, ref)
    assert_bit_exact(got, want, what)


def test_minmax_cache_follows_the_members(engine):
    engine.set_grid(*SMALL, SMALL_CS)
    members = Members(engine)
    for step, (how, fmt) in enumerate(STEPS):
        data = make(SMALL, SMALL_CS, step, fmt)
        members.replace(how, data)
        want = (float(values(data).min()), float(values(data).max()))
        assert engine.member_minmax() == want, f"step {step}: {how} {fmt}"
        assert engine.member_minmax() == want, f"step {step}: {how} {fmt}, cached"


def test_secondary_minmax_cache_follows_the_secondary_members(engine):
    engine.set_grid(*SMALL, SMALL_CS)
    engine.upload_members(make(SMALL, SMALL_CS, 0))
    bound = None
    for step, how in enumerate(["upload", "bind", "overwrite", "upload"]):
        data = make(SMALL, SMALL_CS, step + 1)
        if how == "upload":
            engine.upload_secondary_members(data)
        elif how == "bind":
            bound = to_device(data.reshape(SMALL_CS, -1))
            engine.bind_secondary_members(bound)
        else:
            bound.copy_(to_device(data.reshape(SMALL_CS, -1)))
            torch.cuda.synchronize()
            engine.members_changed()
        want = (float(data.min()), float(data.max()))
        assert engine.secondary_member_minmax() == want, f"step {step}: {how}"
        assert engine.secondary_member_minmax() == want, f"step {step}: {how}, cached"
        assert engine.member_minmax() == (float(make(SMALL, SMALL_CS, 0).min()), float(make(SMALL, SMALL_CS, 0).max()))


def test_wide_copy_follows_the_members(engine, oracle):
    """Spearman at 24 members has no native route: on uint16 members it builds the fp32 copy and reads it."""
    engine.set_grid(*SMALL, SMALL_CS)
    members = Members(engine)
    steps = [("upload", "u16"), ("upload", "u16"), ("bind", "u16"), ("overwrite", "u16"), ("upload", "f32"), ("bind", "u16"),
             ("bind", "f32"), ("upload", "u16")]
    for step, (how, fmt) in enumerate(steps):
        data = make(SMALL, SMALL_CS, step, fmt)
        members.replace(how, data)
        assert engine.wide_copy_bytes() == 0, f"step {step}: the copy of the members before outlived them"
        check_field(engine, oracle, Measure.SPEARMAN, oracle_lib.SPEARMAN, data, SMALL_REF, f"step {step}: {how} {fmt}")
        assert engine.last_member_format() == "f32"
        n = SMALL[0] * SMALL[1] * SMALL[2]
        assert engine.wide_copy_bytes() == (SMALL_CS * n * 4 if fmt == "u16" else 0)


def test_packed_copy_follows_the_members(engine, oracle):
    engine.set_grid(*SMALL, SMALL_CS)
    members = Members(engine)
    engine.set_member_layout("packed")
    try:
        for step, (how, fmt) in enumerate(STEPS):
            data = make(SMALL, SMALL_CS, step, fmt)
            members.replace(how, data)
            check_field(engine, oracle, Measure.PEARSON, oracle_lib.PEARSON, data, SMALL_REF, f"step {step}: {how} {fmt}",
                        device=True)
            assert engine.last_member_layout() == ("packed" if fmt == "f32" else "raw")  # the copy is an fp32 format
    finally:
        engine.set_member_layout("auto")


def test_host_range_tables_follow_the_members(engine, oracle):
    engine.set_grid(*LARGE, LARGE_CS)
    members = Members(engine)
    for step, (how, fmt) in enumerate(STEPS):
        data = make(LARGE, LARGE_CS, step, fmt)
        members.replace(how, data)
        check_field(engine, oracle, Measure.PEARSON, oracle_lib.PEARSON, data, LARGE_REF, f"step {step}: {how} {fmt}")
        assert engine.last_member_format() == fmt
    # ... and narrow members whose evaluations alternate between native ranges and ranges over the fp32 copy
    data = make(LARGE, LARGE_CS, 7, "u16")
    members.replace("upload", data)
    check_field(engine, oracle, Measure.PEARSON, oracle_lib.PEARSON, data, LARGE_REF, "u16, native ranges")
    check_field(engine, oracle, Measure.SPEARMAN, oracle_lib.SPEARMAN, data, LARGE_REF, "u16, ranges over the fp32 copy")
    check_field(engine, oracle, Measure.PEARSON, oracle_lib.PEARSON, data, LARGE_REF, "u16, native ranges again")


def test_regrid_drops_everything(engine, oracle):
    """After the tests above (module order): another grid, another member count, nothing of the old state shows."""
    engine.set_grid(*LARGE, LARGE_CS)
    engine.upload_members(make(LARGE, LARGE_CS, 0, "u16"))
    engine.upload_secondary_members(make(LARGE, LARGE_CS, 1))
    engine.compute(Measure.SPEARMAN, LARGE_REF)
    assert engine.wide_copy_bytes() > 0
    grid, cs = (13, 11, 7), 17
    engine.set_grid(*grid, cs)
    assert engine.wide_copy_bytes() == 0 and engine.member_format() == "f32"
    with pytest.raises(ca.CorrFieldError, match="no member volumes uploaded or bound"):
        engine.member_minmax()
    data = make(grid, cs, 3)
    engine.upload_members(data)
    with pytest.raises(ca.CorrFieldError, match="no secondary members are bound"):
        engine.secondary_member_minmax()
    assert engine.member_minmax() == (float(data.min()), float(data.max()))
    check_field(engine, oracle, Measure.PEARSON, oracle_lib.PEARSON, data, (5, 6, 3), "after set_grid")


def test_context_lifecycle_gives_memory_back():
    xs, ys, zs = LARGE
    block = xs * ys * zs * LARGE_CS * 4  # one fp32 member block of the large grid
    f32, u16, secondary = make(LARGE, LARGE_CS, 0), make(LARGE, LARGE_CS, 1, "u16"), make(LARGE, LARGE_CS, 2)
    small = make(SMALL, SMALL_CS, 3)
    rng = np.random.default_rng(7)
    pairs = np.stack([rng.integers(0, d, 200) for d in (xs, ys, zs, xs, ys, zs)], axis=1)
    free = []
    for cycle in range(10):
        eng = ca.CorrField(0)
        eng.set_grid(*LARGE, LARGE_CS)
        eng.upload_members(f32)
        eng.compute(Measure.PEARSON, LARGE_REF)   # ranged: range tables, staging buffer, copier pool, events
        eng.upload_members(u16)
        eng.compute(Measure.SPEARMAN, LARGE_REF)  # the fp32 copy, the deferred-voxel lists
        assert eng.wide_copy_bytes() == block
        eng.upload_secondary_members(secondary)
        eng.compute(Measure.PEARSON, symmetric=True)
        eng.compute_requests(Measure.PEARSON, pairs)
        eng.ensemble_stat(0)
        eng.set_grid(*SMALL, SMALL_CS)
        eng.upload_members(small)
        eng.compute(Measure.PEARSON, SMALL_REF)
        eng.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    print("free device memory after each cycle (MiB):", [f >> 20 for f in free])
    assert free[1] - free[9] <= block, f"{(free[1] - free[9]) / block:.2f} member blocks lost over eight cycles"
