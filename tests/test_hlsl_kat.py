"""Known-answer tests of the oracle's shading stages against tests/hlsl_ref.py, an independent float64 restatement
of the HLSL (noise3d, getDensity, getFog, getNormal, getColor, traceSample's composite, getPixelRay).  The GPU tests
compare the kernels with oracle/rt_oracle.c bit for bit, which cannot see a misreading of the HLSL that the two share;
these hold the oracle (and tests/test_gpu_hlsl_kat.py the device) to the HLSL's real-number meaning, within the
rounding of float32 under the oracle's evaluation rules.

MEASURED holds the oracle's worst difference from float64 on the fixed sets below; every bound is twice that,
rounded up to one significant digit (bound()).  The sets are fixed and the device repeats the oracle's bits, so the
margin only has to absorb a later change of seeds.  Density figures are relative to max(1, |ref| + |p.y|), all
others absolute; normals are the vector norm of the difference, colours per channel.

    stage                        nomadplains       testing           simple            greenrocks
    noise3d (every landscape)    6.13e-07 / 2e-06
    getDensity                   2.38e-05 / 5e-05  1.10e-05 / 3e-05  1.80e-05 / 4e-05  6.06e-05 / 2e-04
    getFog                       0 / 0             0 / 0             0 / 0             3.61e-06 / 8e-06
    getNormal                    3.90e-04 / 8e-04  1.13e-05 / 3e-05  1.02e-04 / 3e-04  1.12e-04 / 3e-04
    getColor, oracle's normals   2.03e-05 / 5e-05  1.08e-07 / 3e-07  6.88e-06 / 2e-05  2.18e-07 / 5e-07
    composite, oracle's normals  2.06e-05 / 5e-05  1.13e-05 / 3e-05  1.29e-05 / 3e-05  1.29e-05 / 3e-05
    composite, float64 normals   1.51e-04 / 4e-04  1.13e-05 / 3e-05  1.78e-05 / 4e-05  5.48e-05 / 2e-04
    composite, misses            1.99e-05 / 4e-05  1.99e-05 / 4e-05  1.99e-05 / 4e-05  1.99e-05 / 4e-05
    getPixelRay (both poses)     3.75e-06 / 8e-06
(measured worst / bound.)  The largest figure is getNormal's, whose three density differences cancel to a few
thousandths of the terms they are made of; the sky (the misses) repeats tests/test_sky_kat.py's star field error.

Points where a float loop bound lies within 1e-4 of an integer (hlsl_ref's `unsafe`) are left out, and every set
asserts that at most 0.5 % of it is.  getFog of nomadplains, testing and simple is exactly 0.

The mutation check changes the last printed digit of every literal of getDensity, getFog and getColor by one (and
swaps the coordinates under the two small factors of the colour FBM) and requires the mutant to exceed the stage's
bound on the stage's own set.  ESCAPES lists the literals whose mutant stays inside, each with its measured worst
deviation and the reason.
"""
import numpy as np
import pytest

import golden_index as GI
import hlsl_ref as H
import oracle_lib as O
import ray_fixture as RF
import shade_ref as SH
import stage_ref as ST
import surface_ref as SR

LANDS = RF.LANDSCAPES
F_EYE = RF.eye("F0")
EYES = [(0.0, 100.0, 0.0), (13.0, 92.0, -9.5)]
MAX_UNSAFE = 0.005

# The oracle's worst difference from the restatement, measured with this module's own sets (columns as LANDS).
MEASURED = {
    "noise3d": 6.13e-07,
    "density": (2.38e-05, 1.10e-05, 1.80e-05, 6.06e-05),
    "fog": (0.0, 0.0, 0.0, 3.61e-06),
    "normal": (3.90e-04, 1.13e-05, 1.02e-04, 1.12e-04),
    "color": (2.03e-05, 1.08e-07, 6.88e-06, 2.18e-07),
    "composite": (2.06e-05, 1.13e-05, 1.29e-05, 1.29e-05),
    "end_to_end": (1.51e-04, 1.13e-05, 1.78e-05, 5.48e-05),
    "miss": (1.99e-05, 1.99e-05, 1.99e-05, 1.99e-05),
    "pixel_ray": 3.75e-06,
}


def bound(stage, land=None):
    """Twice the measured worst, rounded up to one significant digit."""
    m = MEASURED[stage]
    return twice_rounded_up(m if land is None else m[LANDS.index(land)])


def twice_rounded_up(m):
    x = 2.0 * m
    if x == 0.0:
        return 0.0
    e = np.floor(np.log10(x))
    return float(np.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e)


# --- the sets (fixed seeds) ------------------------------------------------------------------------
def noise_points():
    rng = np.random.default_rng(51)
    lattice = rng.integers(-300, 300, (2000, 3)).astype(np.float32)
    side = rng.integers(-1, 2, (2000, 3))  # integer - 1 ulp, the integer, integer + 1 ulp
    lattice = np.where(side < 0, np.nextafter(lattice, np.float32(-np.inf)),
                       np.where(side > 0, np.nextafter(lattice, np.float32(np.inf)), lattice)).astype(np.float32)
    return np.concatenate([rng.uniform(-500, 500, (20000, 3)).astype(np.float32), lattice,
                           rng.uniform(-2e6, 2e6, (2000, 3)).astype(np.float32)])


def density_points():
    """test_density_bitexact's two sets, the wide one narrowed to |x|, |z| <= 600."""
    rng = np.random.default_rng(6)
    return np.concatenate([rng.uniform(-3000, 3000, (30000, 3)) * [0.2, 0.05, 0.2] + [0, 50, 0],
                           rng.uniform(-20, 20, (5000, 3)) + [0, 100, 0]]).astype(np.float32)


def fog_points():
    """5000 points, the second half deep enough for the fog density's slope ((-y - 2) * 0.0003) to reach its
    saturation; dist log-uniform over 0.01 .. 5000, which saturates 1 - dist * 0.0012 from 833 on."""
    rng = np.random.default_rng(8)
    p = rng.uniform(-600, 600, (5000, 3))
    p[:2500, 1] = rng.uniform(-300, 100, 2500)
    p[2500:, 1] = rng.uniform(-4000, 0, 2500)
    dist = np.exp(rng.uniform(np.log(0.01), np.log(5000.0), 5000))
    dist[:4] = [0.01, 5000.0, 833.0, 834.0]
    return p.astype(np.float32), dist.astype(np.float32)


def pixel_sets():
    """(consts, px, py): 64x48 and 50x36 (the 64x48 matrices under another ScreenSize) for both golden poses."""
    out = []
    for pose in ("reset", "lookdown"):
        for w, h in ((64, 48), (50, 36)):
            c = dict(GI.consts(64, 48, pose))
            c["width"], c["height"] = w, h
            py, px = np.mgrid[0:h, 0:w]
            out.append((c, px.ravel().astype(np.float32), py.ravel().astype(np.float32)))
    return out


def density_error(got, ref, p):
    ref = np.asarray(ref, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref) / np.maximum(1.0, np.abs(ref) + np.abs(np.asarray(p, np.float64)[:, 1]))


def kept(unsafe):
    """The rows that stay in; asserts that at most 0.5 % of the set is left out."""
    unsafe = np.asarray(unsafe, bool)
    assert unsafe.mean() <= MAX_UNSAFE, unsafe.mean()
    return ~unsafe


def unit(d):
    d = np.asarray(d, np.float64)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def oracle_density(land, eye):
    def make():
        c = dict(RF.consts("F0"))
        c["eye"] = np.array(list(eye) + [0], np.float32)
        return O.density(O.noise_tables(), O.make_frame(c, landscape=O.LANDSCAPES[land]), density_points())
    return cached(("density", land, tuple(eye)), make)


class Shaded:
    """The F0-F3 rays of a landscape through the checkers, and what the restatement needs of them."""

    def __init__(self, land):
        self.land = land
        o, d = RF.query(RF.F_SET)
        surf, _ = SR.query(RF.F_SET, land)
        res, px, _, cls, fog_w, fog_rgb = SH.query(RF.F_SET, land, fog_rgb=True)
        # the march with and without the fog accumulation walks the same steps
        assert np.array_equal(surf[:, :4].view(np.uint32), res[:, [4, 5, 6, 3]].view(np.uint32))
        assert np.array_equal(surf[:, 7].view(np.uint32), res[:, 7].view(np.uint32))
        self.dirs, self.res, self.px, self.cls = d, res, px, cls
        self.pd = res[:, [4, 5, 6, 3]]
        self.density = res[:, 7]
        self.fcolord = np.concatenate([fog_rgb, fog_w[:, None]], axis=1)
        self.hit = np.flatnonzero(self.density > 0)
        self.miss = np.flatnonzero(~(self.density > 0))
        self.pdn = unit(d)
        self.pdn32 = self.pdn.astype(np.float32)
        h = self.hit
        self.normal32 = np.zeros((len(o), 3), np.float32)
        self.normal32[h] = ST.normal(land, self.pd[h, :3], self.density[h], F_EYE)
        assert np.array_equal(self.normal32.view(np.uint32), surf[:, 4:7].view(np.uint32))  # the export is get_normal
        self.color32, cls2, self.shadow_w = (np.zeros((len(o), 3), np.float32), np.zeros(len(o), np.uint8),
                                             np.zeros(len(o), np.float32))
        self.color32[h], cls2[h], self.shadow_w[h] = ST.color(land, self.pd[h, :3], self.normal32[h], self.pdn32[h],
                                                              self.pd[h, 3], F_EYE)
        assert np.array_equal(cls2, cls)  # both classify by get_color's own shadow ray
        self.shadowed = cls == SH.SHADOWED

    def normal64(self):
        if not hasattr(self, "_n64"):
            h = self.hit
            self._n64 = np.zeros((len(self.pd), 3)), np.zeros(len(self.pd), bool)
            self._n64[0][h], self._n64[1][h] = H.normal(self.land, self.pd[h, :3], self.density[h], F_EYE)
        return self._n64


def shaded(land):
    return cached(("shaded", land), lambda: Shaded(land))


# --- what each stage is measured by (shared with the GPU tests and the mutation check) ----------------
def worst_noise(got):
    return float(np.abs(got.astype(np.float64) - H.noise3d(noise_points())).max())


def worst_density(land, eye, got, tweak=None, rows=slice(None)):
    p = density_points()[rows]
    ref, unsafe = H.density(land, p, eye, tweak)
    keep = kept(unsafe)
    return float(density_error(got[rows], ref, p)[keep].max())


def worst_fog(land, got, tweak=None):
    p, dist = fog_points()
    return float(np.abs(got.astype(np.float64) - H.fog(land, p, dist, tweak)).max())


def worst_normal(land, pos, w, got):
    ref, unsafe = H.normal(land, pos, w, F_EYE)
    keep = kept(unsafe)
    assert np.all(np.isfinite(ref[keep]))
    return float(np.linalg.norm(got.astype(np.float64) - ref, axis=1)[keep].max())


def worst_color(s, tweak=None, rows=None):
    """getColor alone: the oracle's get_color against the restatement at the oracle's own normals."""
    h = s.hit if rows is None else s.hit[rows]
    ref, unsafe = H.color(s.land, s.pd[h, :3], s.normal32[h], s.pdn32[h], s.pd[h, 3], SH.SUN, s.shadowed[h],
                          s.shadow_w[h], tweak)
    return float(np.abs(s.color32[h].astype(np.float64) - ref)[kept(unsafe)].max())


def composite(s, pd, density, normals, colours):
    """(worst over the hits, worst over the misses, the reference, the kept rows) of traceSample's colour with
    these positions, densities and normals; the march's fcolord and the shadow class are the checker's."""
    ref, unsafe = H.sample_color(s.land, pd, density, s.fcolord, s.pdn, F_EYE, SH.SUN, normals, s.shadowed, s.shadow_w)
    keep = kept(unsafe)
    err = np.abs(colours.astype(np.float64) - ref).max(axis=1)
    return float(err[s.hit][keep[s.hit]].max()), float(err[s.miss].max()), ref, keep


# --- the tests ---------------------------------------------------------------------------------------
def test_noise3d():
    got = O.noise3d(O.noise_tables(), noise_points())
    assert worst_noise(got) <= bound("noise3d")


def test_the_restatement_reads_the_reference_tables():
    nz = O.noise_tables()
    perm2d, grad = H.tables()
    assert np.array_equal(perm2d, np.frombuffer(bytes(nz.perm2d), np.uint8))
    assert np.array_equal(grad.ravel(), np.array(nz.grad[:], np.float32))


@pytest.mark.parametrize("eye", EYES)
@pytest.mark.parametrize("land", LANDS)
def test_density(land, eye):
    assert worst_density(land, eye, oracle_density(land, eye)) <= bound("density", land)


@pytest.mark.parametrize("land", LANDS)
def test_fog(land):
    p, dist = fog_points()
    got = ST.fog(land, p, dist)
    if land != "greenrocks":
        assert not got.any() and not H.fog(land, p, dist).any()  # exactly 0
    else:
        assert (got[:, 3] > 0).sum() >= 1000 and (got[:, 3] == 0).sum() >= 1000
    assert worst_fog(land, got) <= bound("fog", land)


@pytest.mark.parametrize("land", LANDS)
def test_normal(land):
    s = shaded(land)
    h = s.hit
    assert worst_normal(land, s.pd[h, :3], s.density[h], s.normal32[h]) <= bound("normal", land)


@pytest.mark.parametrize("land", LANDS)
def test_census(land):
    """shade_ref.SUN was chosen so that every landscape holds each class."""
    cls = shaded(land).cls
    for c in (SH.MISS, SH.LIT, SH.SHADOWED):
        assert (cls == c).sum() >= 64, (land, c)


@pytest.mark.parametrize("land", LANDS)
def test_color(land):
    assert worst_color(shaded(land)) <= bound("color", land)


@pytest.mark.parametrize("land", LANDS)
def test_composite_with_the_oracles_normals(land):
    s = shaded(land)
    hit, miss, _, _ = composite(s, s.pd, s.density, s.normal32, s.res[:, :3])
    assert hit <= bound("composite", land)
    assert miss <= bound("miss", land)


@pytest.mark.parametrize("land", LANDS)
def test_composite_end_to_end(land):
    """Once more with the restatement's own normals: getNormal's cancellation reaches the colour."""
    s = shaded(land)
    n64, unsafe = s.normal64()
    keep = kept(unsafe[s.hit])
    ref, u2 = H.sample_color(land, s.pd, s.density, s.fcolord, s.pdn, F_EYE, SH.SUN, n64, s.shadowed, s.shadow_w)
    err = np.abs(s.res[:, :3].astype(np.float64) - ref).max(axis=1)[s.hit]
    assert err[keep & kept(u2[s.hit])].max() <= bound("end_to_end", land)


def test_pixel_ray():
    worst = 0.0
    for c, px, py in pixel_sets():
        p, d = ST.pixel_ray(c, px, py)
        rp, rd = H.pixel_ray(c, px, py)
        worst = max(worst, np.abs(p - rp).max(), np.abs(d - rd).max())
    assert worst <= bound("pixel_ray")


# --- the mutation check ------------------------------------------------------------------------------
# Literals whose mutant stays inside the stage's bound: name (or "prefix.*") -> (measured worst deviation, reason).
ESCAPES = {
    "nomadplains.density.dist_min": (2.38e-05, "saturated: below dist 0.02 detail stays in (17.7, 17.8), the same 17 octaves"),
    "nomadplains.density.detail_floor": (2.38e-05, "N <= 2.1 runs the same two octaves as N <= 2.0; and the floor needs "
                                         "dist >= 4450, outside |x|, |z| <= 600"),
    "nomadplains.color.octaves": (2.04e-05, "the 21st octave adds at most 0.5 / 2.03**21 = 2e-7"),
    "nomadplains.color.fresnel_floor": (2.03e-05, "saturated: max(fresnel, 0.1)**40 is at least 1e-40, not 0"),
    "testing.color.fresnel_floor": (1.08e-07, "as nomadplains.color.fresnel_floor"),
    "simple.color.fresnel_floor": (6.88e-06, "as nomadplains.color.fresnel_floor"),
    "greenrocks.color.fresnel_floor": (2.18e-07, "as nomadplains.color.fresnel_floor"),
    "testing.fog.*": (0.0, "dead: `return 0.0f` (terrain.hlsl:56) stands before `return f`"),
    "simple.fog.*": (0.0, "dead: `return 0.0f` (terrain.hlsl:68) stands before `return f`"),
    "simple.density.dist_min": (1.80e-05, "dead: nothing reads dist (terrain.hlsl:37; the detail line is commented out)"),
    "simple.density.octaves": (1.80e-05, "N <= 1.1 runs the same single octave as N <= 1.0 (octaves+1 does leave)"),
    "simple.color.detail_floor": (6.88e-06, "N <= 2.1 runs the same two octaves as N <= 2.0"),
    "greenrocks.density.a_octaves": (6.06e-05, "N <= 7.1 runs the same seven octaves (a_octaves+1 does leave)"),
    "greenrocks.density.b_octaves": (6.06e-05, "N <= 5.1 runs the same five octaves (b_octaves+1 does leave)"),
    "greenrocks.fog.falloff_one": (3.61e-06, "only falloff's sign is read, and dist <= 1 keeps 1.1 - 0.1 dist^2 positive"),
    "greenrocks.fog.falloff_slope": (3.61e-06, "only falloff's sign is read: 1 - 0.2 dist^2 >= 0.8"),
    "greenrocks.fog.falloff_min": (3.61e-06, "only falloff's sign is read: falloff >= 0.9 > 0.1"),
}


def escape(name):
    if name in ESCAPES:
        return ESCAPES[name]
    return ESCAPES.get(name.rsplit(".", 1)[0] + ".*")


def mutant_density(land, tweak):
    """The worst deviation of a mutant; a thinned set first, the whole set only if that stays inside the bound."""
    worst = 0.0
    for rows in (slice(0, None, 16), slice(None)):
        for eye in EYES:
            worst = max(worst, worst_density(land, eye, oracle_density(land, eye), tweak, rows))
            if worst > bound("density", land):
                return worst
    return worst


def mutant_fog(land, tweak):
    p, dist = fog_points()
    return worst_fog(land, cached(("fog", land), lambda: ST.fog(land, p, dist)), tweak)


def mutant_color(land, tweak):
    return worst_color(shaded(land), tweak)


STAGES = {"density": mutant_density, "fog": mutant_fog, "color": mutant_color}


def mutant_cases():
    for land in LANDS:
        for stage in STAGES:
            for name, tweak in H.mutants(land + "." + stage):
                yield land, stage, name, tweak


@pytest.mark.parametrize("land", LANDS)
@pytest.mark.parametrize("stage", list(STAGES))
def test_mutants(land, stage):
    """Every literal, its last printed digit changed by one, leaves the stage's bound on the stage's own set, or
    is listed in ESCAPES with the reason (and then does stay inside)."""
    wrong = []
    for name, tweak in H.mutants(land + "." + stage):
        worst = STAGES[stage](land, tweak)
        outside = worst > bound(stage, land)
        if outside == (escape(name) is not None):
            wrong.append((name, worst, bound(stage, land)))
    assert not wrong, wrong


def test_every_escape_names_a_literal():
    names = {n for _, _, n, _ in mutant_cases()}
    for k in ESCAPES:
        assert k in names or (k.endswith(".*") and any(n.startswith(k[:-1]) for n in names)), k


if __name__ == "__main__":  # the figures of MEASURED and ESCAPES, from this module's own sets
    print("noise3d %.2e" % worst_noise(O.noise3d(O.noise_tables(), noise_points())))
    for land in LANDS:
        s = shaded(land)
        p, dist = fog_points()
        h = s.hit
        hit, miss, _, _ = composite(s, s.pd, s.density, s.normal32, s.res[:, :3])
        n64, unsafe = s.normal64()
        ref, u2 = H.sample_color(land, s.pd, s.density, s.fcolord, s.pdn, F_EYE, SH.SUN, n64, s.shadowed, s.shadow_w)
        e2e = np.abs(s.res[:, :3].astype(np.float64) - ref).max(axis=1)[h][~(unsafe | u2)[h]].max()
        print(land, "density %.2e" % max(worst_density(land, e, oracle_density(land, e)) for e in EYES),
              "fog %.2e" % worst_fog(land, ST.fog(land, p, dist)),
              "normal %.2e" % worst_normal(land, s.pd[h, :3], s.density[h], s.normal32[h]),
              "color %.2e" % worst_color(s), "composite %.2e" % hit, "end_to_end %.2e" % e2e, "miss %.2e" % miss)
    worst = 0.0
    for c, px, py in pixel_sets():
        p, d = ST.pixel_ray(c, px, py)
        rp, rd = H.pixel_ray(c, px, py)
        worst = max(worst, np.abs(p - rp).max(), np.abs(d - rd).max())
    print("pixel_ray %.2e" % worst)
    if all(v is not None for v in MEASURED.values()):
        for land, stage, name, tweak in mutant_cases():
            worst = STAGES[stage](land, tweak)
            if not worst > bound(stage, land):
                print("escape", name, "%.2e" % worst, "bound %.0e" % bound(stage, land))
