"""Inputs that put the reciprocal-division code of the kernels (crf_exact_div.h: exact_div behind exact_div_guard;
crf_binned_bins.h: query_bin_rcp behind binned_range_takes_rcp) on its edges.  Plain numpy; imported by
test_division_edge_inputs.py (CPU: the conditions below, the stand-alone program, the oracle) and by
test_gpu_division_edges.py (the kernels), so each input has a single definition.

Bin-edge lattice: every sample is fl32(min + j * (max - min) / nb), j = 0..nb, or one of its two fp32 neighbours, so
(y - min) / (max - min) * nb sits within an ulp of an integer and a quotient that is one ulp off changes the bin.

Guard-edge families: standard-normal members times a per-voxel scale plus a per-voxel offset, a whole grid per family, so
every wave of a kernel behaves the same whatever its voxel-to-lane layout (as long as a wave covers whole aligned runs of
64 voxels):
    low-in    sd in [2^-60, 2^-57], |mean| in [2^-70, 2^-66]; in a quarter of the voxels one member sits one ulp beside
              the mean (a deviation near the 2^-100 bound of the exact remainder)             -> exact branch
    high-in   sd in [2^57, 2^60]                                                              -> exact branch
    low-out   even voxels: sd in [2^-61, 2^-60); odd voxels: sd as low-in, |mean| in [2^-73, 2^-70), every 8th a mean
              of exactly 0 (antithetic pairs, some of them tiny: _make_antithetic)            -> plain division
    high-out  sd in (2^60, 2^61]                                                              -> plain division
    one-out   as low-in, but one voxel of every 64 consecutive ones fails the guard (sd 2^-4 times too small, sd == 0
              through values 2^-45 times another voxel's, or a mean of exactly 0 through antithetic member pairs), at
              lane 0, 63 or 31 in turn                                                        -> plain division
Only voxels with a mean of exactly 0 and tiny members, or with sd == 0, hold deviations for which exact_div is wrong; an
sd just outside [2^-60, 2^60] leaves it correctly rounded (the window is conservative), so the "guard ignored" mutant of
test_division_edge_inputs.py can be caught on low-out and one-out and never on high-out.  In a RESULT the wrong quotient of
a tiny deviation is absorbed by the sum; the sd == 0 voxels (one-out, tiny_shadow) are where a kernel that ignored the
guard returns NaN for the reference's +-inf.
mean and sd are the reference's sequential fp32 passes (ref_mean_sd); guard_family() asserts each family lies where
this table says."""
import numpy as np

F32 = np.float32
GUARD_MEAN_MIN = 2.0 ** -70
GUARD_SD_MIN, GUARD_SD_MAX = 2.0 ** -60, 2.0 ** 60

# ---- ranges -----------------------------------------------------------------------------------------------------------
ORDINARY_RANGES = [(-3.7, 4.1), (250.0, 310.5), (-1e-3, 2.5e-3)]
# (max, inside the window): min = 0
BOUNDARY_RANGES = [
    ((0.0, float(np.nextafter(F32(2.0 ** -60), F32(0)))), False),
    ((0.0, 2.0 ** -60), True),
    ((0.0, float(F32(1.3 * 2.0 ** -60))), True),
    ((0.0, float(F32(0.7 * 2.0 ** 60))), True),
    ((0.0, 2.0 ** 60), True),
    ((0.0, float(np.nextafter(F32(2.0 ** 60), F32(np.inf)))), False),
]


def range_takes_rcp(mm) -> bool:
    """binned_range_takes_rcp on the fp32 difference the kernels form."""
    r = F32(mm[1]) - F32(mm[0])
    return bool(r >= F32(GUARD_SD_MIN) and r <= F32(GUARD_SD_MAX))


for _mm, _inside in BOUNDARY_RANGES:
    assert range_takes_rcp(_mm) == _inside, _mm
for _mm in ORDINARY_RANGES:
    assert range_takes_rcp(_mm)


# ---- bin-edge lattice -------------------------------------------------------------------------------------------------
def edge_lattice(mn, mx, nb) -> np.ndarray:
    """The sorted pool: fl32(mn + j * (mx - mn) / nb), j = 0..nb, and both fp32 neighbours of each, clipped to [mn, mx]."""
    mn, mx = F32(mn), F32(mx)
    j = np.arange(nb + 1, dtype=np.float64)
    centre = (float(mn) + j * ((float(mx) - float(mn)) / nb)).astype(F32)
    pool = np.concatenate([centre, np.nextafter(centre, F32(-np.inf)), np.nextafter(centre, F32(np.inf))])
    return np.unique(np.clip(pool, mn, mx))


# plants of lattice_ensemble: (x, y, z) of the voxel, each a voxel of its own
PLANT_NAN, PLANT_POS_INF, PLANT_NEG_INF, PLANT_TINY = (3, 2, 1), (7, 4, 2), (11, 1, 3), (14, 5, 4)
TINY_SAMPLES = [1e-35, 1e-41, -1e-35, -1e-41]      # 0 < |y| < 2^-100, one of each sign a denormal


def lattice_ensemble(cs, grid, mn, mx, nb, seed, plants=False) -> np.ndarray:
    """[cs, zs, ys, xs] float32, every sample drawn from edge_lattice(mn, mx, nb) (so is any voxel taken as the reference
    vector).  plants: a NaN at PLANT_NAN, a +inf at PLANT_POS_INF, a -inf at PLANT_NEG_INF and, where mn == 0,
    TINY_SAMPLES at PLANT_TINY."""
    xs, ys, zs = grid
    pool = edge_lattice(mn, mx, nb)
    rng = np.random.default_rng(seed)
    ens = pool[rng.integers(0, pool.size, (cs, zs, ys, xs))]
    if plants:
        at = lambda p: (p[2], p[1], p[0])
        ens[(1 % cs,) + at(PLANT_NAN)] = np.nan
        ens[(2 % cs,) + at(PLANT_POS_INF)] = np.inf
        ens[(3 % cs,) + at(PLANT_NEG_INF)] = -np.inf
        if float(mn) == 0.0:
            for e, t in enumerate(TINY_SAMPLES):
                ens[(2 * e,) + at(PLANT_TINY)] = F32(t)
    return ens


# ---- the reference's mean and standard deviation ----------------------------------------------------------------------
def ref_mean_sd(vectors: np.ndarray):
    """computePearson2's sequential fp32 passes over axis 0 of [cs, n]: mean += invN * x; var += invNm1 * d * d;
    sqrtf.  Every numpy operation below is one fp32 operation."""
    v = np.ascontiguousarray(vectors, F32)
    cs = v.shape[0]
    n = F32(cs)
    inv_n = F32(1) / n
    inv_nm1 = F32(1) / (n - F32(1))
    with np.errstate(all="ignore"):
        mean = np.zeros(v.shape[1:], F32)
        for e in range(cs):
            mean = mean + inv_n * v[e]
        var = np.zeros(v.shape[1:], F32)
        for e in range(cs):
            d = v[e] - mean
            var = var + inv_nm1 * d * d
        return mean, np.sqrt(var)


def guard_holds(mean, sd) -> np.ndarray:
    """exact_div_guard, elementwise."""
    return (np.abs(mean) >= F32(GUARD_MEAN_MIN)) & (sd >= F32(GUARD_SD_MIN)) & (sd <= F32(GUARD_SD_MAX))


# ---- guard-edge families ----------------------------------------------------------------------------------------------
FAMILIES = ["low-in", "high-in", "low-out", "high-out", "one-out"]
IN_FAMILIES = ["low-in", "high-in"]
ONE_OUT_LANES = (0, 63, 31)


def _unit_vectors(rng, cs, n, zero_member=None):
    """[cs, n] float64 with mean 0 and sample sd 1 per column; member `zero_member` is exactly 0 where given."""
    base = rng.standard_normal((cs, n))
    if zero_member is not None and cs >= 4:
        keep = np.arange(cs) != zero_member
        base[zero_member] = 0.0
        base[keep] -= base[keep].mean(axis=0)
    else:
        base -= base.mean(axis=0)
    return base / base.std(axis=0, ddof=1)


def _log_uniform(rng, lo, hi, n):
    return np.exp2(rng.uniform(np.log2(lo), np.log2(hi), n))


def one_out_voxels(n) -> np.ndarray:
    """The failing voxel of every run of 64: lane 0, 63, 31 in turn."""
    blocks = np.arange((n + 63) // 64)
    v = blocks * 64 + np.array(ONE_OUT_LANES)[blocks % 3]
    return v[v < n]


def _make_antithetic(col):
    """One voxel's members (a [cs] view) in pairs (y, -y), a last odd member 0: every partial sum of the reference's mean
    is exactly 0 after each pair, so the mean is exactly 0.  All but one pair (at most three) are tiny, TINY_SAMPLES and a
    second denormal: non-zero deviations below 2^-100, for which exact_div's remainder is no longer exact -- what the guard's
    test of the mean exists for."""
    half = col.size // 2
    col[1:2 * half:2] = -col[0:2 * half:2]
    if col.size % 2:
        col[-1] = 0
    for i, t in enumerate([1e-35, 1e-41, 3e-43][:max(half - 1, 0)]):
        col[2 * i], col[2 * i + 1] = F32(t), F32(-t)


TINY_SHADOW = 2.0 ** -45


def pattern_voxel(n) -> int:
    """The voxel some failing voxels of one-out are a tiny multiple of; never a failing voxel itself, never planted."""
    return 35 + 64 * min(2, n // 64 - 1) if n >= 64 else n // 2


def tiny_shadow(ens, one_lane_only=False) -> np.ndarray:
    """A copy of a low-in [cs, n] whose voxels (all, or one_out_voxels only) are TINY_SHADOW times the original: values
    around 2^-105, an exact scaling, so every deviation is the original's scaled and keeps its sign, but its square
    underflows: sd == 0 and the reference's quotients are +-inf.  Correlated with the original, all products have one
    sign and the reference gives +inf (-inf), where exact_div without its guard gives NaN: the one kind of input on which
    IGNORING THE GUARD changes a result rather than a quotient that the sum absorbs."""
    out = ens.copy()
    v = one_out_voxels(ens.shape[1]) if one_lane_only else slice(None)
    out[:, v] = out[:, v] * F32(TINY_SHADOW)
    m, s = ref_mean_sd(out[:, v])
    assert (s == 0).all() and (m != 0).all()
    return out


def guard_family(name, cs, n, seed) -> np.ndarray:
    """[cs, n] float32 of family `name` (module docstring); asserts the family's condition on every voxel."""
    assert name in FAMILIES and cs >= 2
    rng = np.random.default_rng([seed, FAMILIES.index(name), cs])
    sign = rng.choice([-1.0, 1.0], n)
    planted = np.zeros(n, bool)
    plant_member = cs // 3
    if name in ("low-in", "low-out", "one-out"):
        sd = _log_uniform(rng, 2.0 ** -60 * 1.001, 2.0 ** -57, n)
        mean = sign * _log_uniform(rng, 2.0 ** -70 * 1.05, 2.0 ** -66, n)
        sd[:4] = 2.0 ** -60 * 1.0001                   # right at the edges
        mean[:4] = sign[:4] * 2.0 ** -70 * 1.01       # (the fp32 mean of cs terms carries ~2^-80 of rounding)
        if name == "low-out":
            sd[0::2] = _log_uniform(rng, 2.0 ** -61, 2.0 ** -60 * 0.999, (n + 1) // 2)
            mean[1::2] = sign[1::2] * _log_uniform(rng, 2.0 ** -73, 2.0 ** -70 * 0.95, n // 2)
            sd[0], mean[1] = 2.0 ** -60 * 0.9999, sign[1] * 2.0 ** -70 * 0.99
        elif cs >= 16:
            planted[2::4] = True
    elif name == "high-in":
        sd = _log_uniform(rng, 2.0 ** 57, 2.0 ** 60 * 0.999, n)
        sd[:4] = 2.0 ** 60 * 0.9999
        mean = sign * sd * rng.uniform(0.1, 2.0, n)
    else:
        sd = _log_uniform(rng, 2.0 ** 60 * 1.001, 2.0 ** 61, n)
        sd[:4] = 2.0 ** 60 * 1.0001
        mean = sign * sd * rng.uniform(0.1, 2.0, n)
    unit = _unit_vectors(rng, cs, n)
    if planted.any():                                  # the planted member starts AT the mean
        unit[:, planted] = _unit_vectors(rng, cs, int(planted.sum()), zero_member=plant_member)
    ens = (unit * sd + mean).astype(F32)
    if planted.any():                                  # ... and moves one ulp beside the fp32 mean it then has
        up = np.arange(n) % 8 < 4
        for _ in range(8):
            m, _sd = ref_mean_sd(ens)
            beside = np.where(up, np.nextafter(m, F32(np.inf)), np.nextafter(m, F32(-np.inf)))
            ens[plant_member, planted] = beside[planted]
    if name == "one-out":
        for i, v in enumerate(one_out_voxels(n)):
            if i % 4 == 0:                             # sd (and mean) 2^-4 times too small: exact scaling
                ens[:, v] *= F32(2.0 ** -4)
            elif i % 4 == 2:                           # 2^-45 times the pattern voxel: sd underflows to 0 (tiny_shadow)
                ens[:, v] = ens[:, pattern_voxel(n)] * F32(TINY_SHADOW)
            else:
                _make_antithetic(ens[:, v])
    if name == "low-out":
        for v in range(5, n, 8):
            _make_antithetic(ens[:, v])
    # the family lies where the table says
    m, s = ref_mean_sd(ens)
    ok = guard_holds(m, s)
    if name in IN_FAMILIES:
        assert ok.all(), f"{name} cs={cs}: {int((~ok).sum())} voxels fail the guard"
    elif name == "one-out":
        expect = np.ones(n, bool)
        expect[one_out_voxels(n)] = False
        assert (ok == expect).all(), f"{name} cs={cs}: the guard fails elsewhere than planned"
        assert (m[one_out_voxels(n)[1::2]] == 0).all()
    else:
        assert not ok.any(), f"{name} cs={cs}: {int(ok.sum())} voxels pass the guard"
    if name == "low-in":
        assert (s <= F32(2.0 ** -56)).all() and (np.abs(m) <= F32(2.0 ** -65)).all()
    if name == "high-in":
        assert (s >= F32(2.0 ** 56)).all()
    if name in ("low-out", "high-out"):                # just outside: within a factor of 8 of the guard's bounds
        near_sd = ((s >= F32(2.0 ** -63)) & (s <= F32(2.0 ** -57))) | ((s > F32(2.0 ** 60)) & (s <= F32(2.0 ** 63)))
        assert ((near_sd & (np.abs(m) >= F32(2.0 ** -74))) | (m == 0)).all()
    if planted.any():                                  # most planted members ended exactly one ulp beside the mean
        d = np.abs(ens[plant_member, planted].astype(np.float64) - m[planted].astype(np.float64))
        ulp = np.spacing(np.abs(m[planted])).astype(np.float64)
        assert (d <= 4 * ulp).all() and (d > 0).mean() >= 0.5, (name, cs)
    assert np.isfinite(ens).all()
    return ens


def with_unit_voxel(ens, v, seed=0) -> np.ndarray:
    """A copy of [cs, n] with standard-normal members at voxel v (mean and sd O(1): the guard holds there)."""
    out = ens.copy()
    out[:, v] = np.random.default_rng([seed, 77]).standard_normal(ens.shape[0]).astype(F32) + F32(0.5)
    return out


def antithetic_f16(cs, n, seed) -> np.ndarray:
    """[cs, n] float16, members in pairs (y, -y): every mean is exactly 0 in the reference's fp32 pass."""
    assert cs % 2 == 0
    rng = np.random.default_rng([seed, 16])
    half = (rng.standard_normal((cs // 2, n)) * 2.0).astype(np.float16)
    ens = np.empty((cs, n), np.float16)
    ens[0::2], ens[1::2] = half, -half
    m, s = ref_mean_sd(ens.astype(F32))
    assert (m == 0).all() and (s > 0).all() and not guard_holds(m, s).any()
    return ens


def denormal_f16(cs, n, seed) -> np.ndarray:
    """[cs, n] float16 denormals of either sign only (|y| < 2^-14, sd far inside the guard's window)."""
    rng = np.random.default_rng([seed, 17])
    bits = rng.integers(1, 0x0400, (cs, n)).astype(np.uint16) | (rng.integers(0, 2, (cs, n)).astype(np.uint16) << 15)
    ens = bits.view(np.float16)
    assert (np.abs(ens.astype(F32)) < 2.0 ** -14).all() and (ens != 0).all()
    return ens


# ---- the cases both test files run ------------------------------------------------------------------------------------
GRID = (16, 6, 5)              # xs, ys, zs of the lattice ensembles: 480 voxels, several waves, not a multiple of 64
LATTICE_REF = (5, 3, 2)        # a lattice voxel without a plant
NUM_BINS = (10, 80, 255)
GUARD_GRID = (16, 8, 8)        # xs, ys, zs of the guard-edge ensembles: 1024 voxels, whole waves and whole blocks only
GUARD_REF = (3, 2, 1)          # pattern_voxel(1024): one-out's sd == 0 voxels are multiples of it


def lattice_case(cs, mm, nb, plants=False, side=0) -> np.ndarray:
    """The lattice ensemble of (member count, range, bins); side 1 is an independent second field."""
    seed = [cs, nb, int(F32(mm[0]).view(np.uint32)), int(F32(mm[1]).view(np.uint32)), side]
    return lattice_ensemble(cs, GRID, mm[0], mm[1], nb, seed, plants)


def voxel(ens, xyz) -> np.ndarray:
    x, y, z = xyz
    return ens[:, z, y, x].copy()


def request_pairs(grid, n, seed):
    """n random (xi, yi, zi, xj, yj, zj) on `grid` and the two linear voxel indices."""
    xs, ys, zs = grid
    rng = np.random.default_rng([seed, 99])
    pairs = np.stack([rng.integers(0, xs, n), rng.integers(0, ys, n), rng.integers(0, zs, n),
                      rng.integers(0, xs, n), rng.integers(0, ys, n), rng.integers(0, zs, n)], axis=1)
    return pairs, linear_index(pairs[:, 0:3], grid), linear_index(pairs[:, 3:6], grid)


def linear_index(p, grid):
    return (p[:, 2] * grid[1] + p[:, 1]) * grid[0] + p[:, 0]


def guard_field(name, cs, seed) -> np.ndarray:
    """guard_family on GUARD_GRID as [cs, zs, ys, xs]."""
    xs, ys, zs = GUARD_GRID
    return guard_family(name, cs, xs * ys * zs, seed).reshape(cs, zs, ys, xs)


REQUEST_ROW = 128              # voxels per family in guard_request_case
REQUEST_COUNT = 333


def guard_request_case(cs, seed):
    """One ensemble on a (REQUEST_ROW, 6, 1) grid whose row y < 5 holds family FAMILIES[y] and whose row 5 holds
    tiny_shadow of the low-in row, and REQUEST_COUNT requests that pair voxels of different families.  Items 0..63 pair
    low-in with low-in, 64..127 low-in with high-in and 192..255 high-in with high-in (whole waves on the exact branch);
    128..191 pair high-in with low-in except item 159, which pairs a low-in voxel with its shadow (one failing lane, +inf);
    256..319 pair every second low-in voxel with its shadow and a random voxel with the shadow of another; the rest pair
    random voxels of all rows.  Returns (ens [cs, 1, 6, REQUEST_ROW], pairs, idx_i, idx_j)."""
    rows = [guard_family(f, cs, REQUEST_ROW, seed) for f in FAMILIES]
    rows.append(tiny_shadow(rows[FAMILIES.index("low-in")]))
    grid = (REQUEST_ROW, len(rows), 1)
    ens = np.stack(rows, axis=1).reshape(cs, 1, len(rows), REQUEST_ROW)
    pairs, _, _ = request_pairs(grid, REQUEST_COUNT, seed)
    low_in, high_in, shadow = FAMILIES.index("low-in"), FAMILIES.index("high-in"), len(FAMILIES)
    pairs[0:64, 1], pairs[0:64, 4] = low_in, low_in
    pairs[64:128, 1], pairs[64:128, 4] = low_in, high_in
    pairs[128:192, 1], pairs[128:192, 4] = high_in, low_in
    pairs[159, 1], pairs[159, 4], pairs[159, 3] = low_in, shadow, pairs[159, 0]
    pairs[192:256, 1], pairs[192:256, 4] = high_in, high_in
    pairs[256:320, 1], pairs[256:320, 4] = low_in, shadow
    pairs[256:320:2, 3] = pairs[256:320:2, 0]
    return ens, pairs, linear_index(pairs[:, 0:3], grid), linear_index(pairs[:, 3:6], grid)
