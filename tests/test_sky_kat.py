"""Sky known-answer vectors: the oracle's getRayleighMieColor and
getSpaceColor (oracle/rt_oracle.c get_rayleigh_mie / get_space_color, float32 under rules R1-R9)
against tests/sky_ref.py, an independent float64 restatement of Media/common/shaders/sky.hlsl
with exact exp / pow.

The first three tests compare at 110 fixed view directions (directions()), 7 sun angles and 3 eye
positions.  Their bound is BASELINE.md's parity tolerance, 1e-4 per channel; the measured worst case
of 5.8e-5 (the star field: float32 rounding of dir * 500 before the lattice) and 1.2e-5 for the
scattering is true of those 110 directions only: over the sphere the stars reach 1.37e-4 and the Mie
term, in the hundreds next to the sun, is off by whole units.  The GPU's sky equals the oracle's bit
for bit there (tests/test_gpu_parity.py::test_sky_known_answers_device).

The tests after them cover the sphere: base_directions() (a 2000-point Fibonacci sphere, the horizon
band y = +-1e-3, +-1e-7, +-0 at 16 azimuths, the zenith and the nadir, 100 directions each of length
0.5 and 2) and cones() of 0, 1e-4, 1e-3, 1e-2, 5e-2 and 0.2 rad about +SunDirection and -SunDirection,
for the 15 suns of suns() and the 8 eyes of SPHERE_EYES: 2620 directions per case, 120 cases.  An
absolute bound cannot hold there, for three reasons that are float32 conditioning and no bug:
  - the base of getMiePhase's pow, 1 + g^2 - 2 g fCos, falls to (1 + g)^2 = 1e-4 along SunDirection,
    where one rounding of fCos is 6e-4 of it;
  - at twilight exp(-fScatter * ...) reaches e^-10 and carries ten times its exponent's relative error;
  - outerRadius - camHeight cancels as Eye.y nears 5000, and every output is proportional to it.
So the model is relative, per channel, with |v| + FLOOR as the scale (FLOOR = 1e-6):
    Rayleigh  a_r + c * 2^-24 * outerRadius / |distToTop|
    Mie       a_m + b * 2^-24 / base + c * 2^-24 * outerRadius / |distToTop|
    stars     s, absolute
with base and distToTop taken from the restatement.  measure() fits it in this order: a_r, and a_m where
base >= DENOM_FAR, at the eyes a whole unit below the top; then b from what a_m leaves at those eyes;
then c from what those leave at every eye.  Measured (the oracle against the restatement, never the device):
    a_r = 2.2933e-4 (twilight, t = 0.2; by day 3.7e-5)     a_m = 1.2517e-4     b = 9.0648
    c = 0.97435 (Eye.y = 4999: one rounding of camHeight)   s = 1.3704e-4
MEASURED holds them rounded up to three digits and every bound is twice its figure.  The stars' figure is
the float32 rounding of the normalised direction and of dir * 500 before the lattice: a relative 2^-24 of its
argument moves noise3d by at most 500 * 2^-24 * |grad noise3d| = 3e-5 * 2.8 = 8.3e-5 (|grad| <= 2.8 by central
differences at 20000 arguments), the two other terms add 0.5 * (150.2 + 200.2) / 500 of that, and two such
roundings (the normalisation, the product) come to 2.2e-4, which the measured 1.37e-4 stays under.

No point is left out.  Where the restatement itself is NaN (the nadir: modRayDir normalises a zero vector, in
the HLSL too) the oracle must be NaN; at Eye.y = 5000 the oracle's scattering is NaN everywhere (float32
camHeight == outerRadius: far = 0, t = 0, 0 / 0) and the restatement finite.  Where the night's restatement
has underflowed below 1e-30 and the oracle returns 0, 0 is required.

The mutation check changes the last printed digit of each of the 57 sky.* literals (hlsl_ref.LITERALS) and
applies the 15 structural misreadings of sky_ref.STRUCTURES; each must leave a bound on some case.  ESCAPES
lists the three that do not, with the worst multiple of a bound they reach and the reason.  tracescreen.hlsl:22's
0.0005 (sample.sky_amount) is judged on test_hlsl_kat's F0-F3 hits, 16 of which lie beyond 1000."""
import numpy as np
import pytest

import hlsl_ref as H
import oracle_lib as O
import sky_ref as R

TOL = 1e-4  # BASELINE.md parity bound, per channel


def directions():
    az = np.radians(np.arange(0, 360, 30))
    el = np.radians([-30, -5, 0, 2, 5, 15, 30, 60, 89.5])
    d = [[np.cos(e) * np.cos(a), np.sin(e), np.cos(e) * np.sin(a)] for e in el for a in az]
    return np.array(d + [[0.0, 1.0, 0.0], [0.3, 0.0, -0.7]], np.float32)


def sun(t):
    """Terrain::setTimeOfDay (Terrain.cpp:292-298): normalize(-sin 2 pi t, -cos 2 pi t, 0.1)."""
    s = np.array([-np.sin(2 * np.pi * t), -np.cos(2 * np.pi * t), 0.1])
    return (s / np.linalg.norm(s)).astype(np.float32)


EYES = [(0.0, 100.0, 0.0), (1234.0, 350.0, -987.0), (-50.0, 2.0, 75.0)]
TIMES = [0.05, 0.2, 0.25, 0.3, 0.45, 0.7, 0.9]


def frame(eye, t):
    c = {"width": 64, "height": 48, "eye": list(eye) + [1.0], "view_inverse": np.eye(4), "projection": np.eye(4),
         "sun": sun(t)}
    return O.make_frame(c)


@pytest.mark.parametrize("eye", EYES)
@pytest.mark.parametrize("t", TIMES)
def test_sky_oracle_matches_float64_restatement(eye, t):
    nz = O.noise_tables()
    perm2d = np.frombuffer(bytes(nz.perm2d), np.uint8)
    grad = np.array(nz.grad[:], np.float32).reshape(128, 4)
    d = directions()
    got = O.sky(nz, frame(eye, t), d).astype(np.float64)
    mie, ray = R.rayleigh_mie(d, np.array(eye, np.float32), sun(t))
    space = R.space_color(perm2d, grad, d, sun(t))
    assert np.all(np.isfinite(got))
    assert np.abs(got[:, 0:3] - mie).max() <= TOL
    assert np.abs(got[:, 3:6] - ray).max() <= TOL
    assert np.abs(got[:, 6] - space).max() <= TOL


def test_sky_known_answer_properties():
    """Structure the restatements share with the HLSL: below-horizon directions see the horizon's
    sky (modRayDir saturates y) and no stars; the day hack adds (0.3, 0.4, 0.6) * saturate(sun.y)."""
    nz = O.noise_tables()
    d = np.array([[0.6, -0.4, 0.2], [0.6, 0.0, 0.2]], np.float32)
    got = O.sky(nz, frame(EYES[0], 0.3), d)
    assert np.array_equal(got[0, :3], got[1, :3])  # mie of the clamped direction
    assert got[0, 6] == 0.0 and got[1, 6] == 0.0  # getSpaceColor: dir.y <= 0 -> 0
    noon = O.sky(nz, frame(EYES[0], 0.5), np.array([[0.0, 1.0, 0.0]], np.float32))[0]
    assert np.all(noon[3:6] >= np.array([0.3, 0.4, 0.6], np.float32) * sun(0.5)[1] - 1e-6)


# ====================================================================================================
# The sky over the sphere and at the sun (shared with tests/test_gpu_sky_kat.py)
# ----------------------------------------------------------------------------------------------------
# The oracle's worst figures against the restatement on the sets below (the __main__ of this module prints
# them), each rounded up to three digits; every bound is twice its figure.
MEASURED = {
    "a_r": 2.30e-4,   # Rayleigh, relative to |v| + FLOOR, at the eyes well below the top
    "a_m": 1.26e-4,   # Mie, likewise, where the pow's base is at least DENOM_FAR
    "b": 9.07,        # Mie, the sun's conditioning: (relative error - a_m) * base / 2^-24
    "c": 0.975,       # both, the eye's conditioning: (relative error - the above) * |distToTop| / (2^-24 outerRadius)
    "stars": 1.38e-4, # getSpaceColor, absolute
}
FLOOR = 1e-6
DENOM_FAR = 0.03  # the base 1e-4 + 1.98 (1 - cos angle) beyond 0.17 rad of the sun: there b's term is below 2e-5
EYE_FAR = 205.0   # outerRadius / |distToTop| of an eye a whole unit (1000 of the world's) below the top
ULP = 2.0 ** -24
UNDERFLOW = 1e-30

SPHERE_EYES = EYES + [(0.0, -300.0, 0.0), (0.0, 0.0, 0.0), (0.0, 4000.0, 0.0), (0.0, 4999.0, 0.0), (0.0, 5001.0, 0.0)]
NAN_EYE = (0.0, 5000.0, 0.0)  # float32 camHeight == outerRadius: far = 0, t = 0, 0 / 0
SPHERE_TIMES = [0.05, 0.2, 0.22, 0.25, 0.27, 0.3, 0.45, 0.5, 0.7, 0.9]
NADIR = 2097  # its index in base_directions(): x = z = 0 and y <= 0 is normalize(0, 0, 0), NaN in every reading
CONE_ANGLES = [0.0, 1e-4, 1e-3, 1e-2, 5e-2, 0.2]
# the time at which the stars' gate -SunDirection.y * 2.7 - 0.5 crosses 0 in the evening: cos(2 pi t) = sqrt(1.01) * 0.5 / 2.7
T_GATE = float(np.arccos(np.sqrt(1.01) * 0.5 / 2.7) / (2 * np.pi))


def _unit32(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(np.float32)


def suns():
    """name -> SunDirection (float32): setTimeOfDay's, the two either side of the stars' gate, one off the z = 0.1
    plane, and two that are not unit vectors (the variable manager sets any vector; the HLSL never normalises)."""
    out = {"t=%g" % t: sun(t) for t in SPHERE_TIMES}
    out["gate-"] = sun(T_GATE - 1e-3)  # stars faintly on
    out["gate+"] = sun(T_GATE + 1e-3)  # stars off
    out["off-plane"] = _unit32([-0.4, 0.35, -0.6])
    out["half"] = (sun(0.3).astype(np.float64) * 0.5).astype(np.float32)
    out["long"] = (sun(0.27).astype(np.float64) * 1.01).astype(np.float32)
    return out


def fibonacci_sphere(n=2000):
    i = np.arange(n) + 0.5
    y = 1.0 - 2.0 * i / n
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - y * y)
    return np.stack([r * np.cos(phi), y, r * np.sin(phi)], axis=1)


def horizon_band():
    az = np.arange(16) * (2 * np.pi / 16) + 0.1
    ys = np.array([-1e-3, -1e-7, -0.0, 0.0, 1e-7, 1e-3])
    return np.array([[np.cos(a), y, np.sin(a)] for y in ys for a in az])


def base_directions():
    """The Fibonacci sphere, the horizon band, the zenith and the nadir, and every 20th direction of the sphere at
    length 0.5 and at length 2 (getPixelRay's output arrives unnormalised, and :132 reads orgRayDir.y)."""
    def make():
        sph = fibonacci_sphere()
        d = np.concatenate([sph, horizon_band(), [[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]], sph[::20] * 0.5, sph[::20] * 2.0])
        d = d.astype(np.float32)
        assert tuple(d[NADIR]) == (0.0, -1.0, 0.0)
        d.setflags(write=False)
        return d
    return _cached("base", make)


def cone(axis):
    """Directions at CONE_ANGLES from `axis`, 32 azimuths each (one for the axis itself)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    u = np.cross(a, [0.0, 0.0, 1.0] if abs(a[2]) < 0.9 else [1.0, 0.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(a, u)
    out = []
    for th in CONE_ANGLES:
        for ph in (np.arange(32) * (2 * np.pi / 32) + 0.05) if th > 0 else [0.0]:
            out.append(np.cos(th) * a + np.sin(th) * (np.cos(ph) * u + np.sin(ph) * v))
    return np.array(out)


def cones(sun_vec):
    """The cone about +SunDirection (where the Mie phase peaks when the sun is up) and the one about -SunDirection."""
    s = np.asarray(sun_vec, np.float64)
    return np.concatenate([cone(s), cone(-s)]).astype(np.float32)


def sphere_directions(sun_name):
    def make():
        d = np.concatenate([base_directions(), cones(suns()[sun_name])])
        d.setflags(write=False)
        return d
    return _cached(("dirs", sun_name), make)


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def sky_frame(eye, sun_vec):
    c = {"width": 64, "height": 48, "eye": list(eye) + [1.0], "view_inverse": np.eye(4), "projection": np.eye(4),
         "sun": sun_vec}
    return O.make_frame(c)


def tables():
    def make():
        nz = O.noise_tables()
        return np.frombuffer(bytes(nz.perm2d), np.uint8), np.array(nz.grad[:], np.float32).reshape(128, 4)
    return _cached("tables", make)


STAR_TWEAKS = ("sky.space_", "sky.eSpace", "sky.structure=stars_", "sky.structure=space_")
BOTH_TWEAKS = ("sky.structure=no_saturate_in_modraydir",)


def restated(eye, sun_name, tweak=None, name=None):
    """(mie, rayleigh, base of the Mie pow, outerRadius / |distToTop|, stars) of the restatement for a case;
    computed once when untweaked.
    `name` (a mutant's) leaves out the half a mutant cannot reach: that half is the untweaked one."""
    def make(tw=None, stars=True, scatter=True):
        d, s = sphere_directions(sun_name), suns()[sun_name]
        perm2d, grad = tables()
        e = np.array(eye, np.float32)
        with np.errstate(all="ignore"):  # the nadir's 0 / 0, and what a mutant overflows
            out = list(R.rayleigh_mie(d, e, s, tw, conditioning=True)) if scatter else [None] * 4
            out.append(R.space_color(perm2d, grad, d, s, tw) if stars else None)
        return out
    plain = _cached(("ref", tuple(eye), sun_name), make)
    if not tweak:
        return plain
    stars = name.startswith(STAR_TWEAKS + BOTH_TWEAKS)
    scatter = not name.startswith(STAR_TWEAKS)
    got = make(tweak, stars, scatter)
    return [g if g is not None else p for g, p in zip(got, plain)]


def oracle_sky(eye, sun_name):
    def make():
        got = O.sky(O.noise_tables(), sky_frame(eye, suns()[sun_name]), sphere_directions(sun_name))
        got.setflags(write=False)
        return got
    return _cached(("oracle", tuple(eye), sun_name), make)


def figures(got, ref):
    """The four figures of MEASURED's model for one case: (Rayleigh's relative error, Mie's where the base is at
    least DENOM_FAR, Mie's everywhere as (relative error, base), the stars' absolute error), every point in.  Where
    the restatement itself is NaN (the nadir: modRayDir normalises a zero vector) a NaN is the right answer and
    counts as no error; a NaN on one side alone is an infinite one."""
    mie, ray, denom, _, stars = ref
    got = np.asarray(got, np.float64)

    def err(g, r):
        with np.errstate(invalid="ignore"):
            e = np.abs(g - r)
        return np.where(np.isnan(g) & np.isnan(r), 0.0, np.where(np.isnan(e), np.inf, e))

    rel_m = (err(got[:, 0:3], mie) / (np.abs(np.nan_to_num(mie)) + FLOOR)).max(axis=1)
    rel_r = (err(got[:, 3:6], ray) / (np.abs(np.nan_to_num(ray)) + FLOOR)).max(axis=1)
    return rel_r, rel_m, np.where(np.isnan(denom), 1.0, denom), err(got[:, 6], stars)


def bounds(denom, eye_cond):
    """(Rayleigh's relative bound, Mie's per point, the stars' absolute): twice the measured model."""
    m = MEASURED
    eye_term = m["c"] * ULP * eye_cond
    return 2.0 * (m["a_r"] + eye_term), 2.0 * (m["a_m"] + eye_term + m["b"] * ULP / denom), 2.0 * m["stars"]


def excess(got, ref):
    """The largest error of a case as a multiple of its bound (<= 1: inside), over every point and output.
    A non-finite error counts as outside."""
    rel_r, rel_m, denom, err_s = figures(got, ref)
    b_r, b_m, b_s = bounds(denom, ref[3])
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = max(np.max(rel_r / b_r), np.max(rel_m / b_m), np.max(err_s / b_s))
    return float(worst) if np.isfinite(worst) else np.inf


def check_case(got, eye, sun_name):
    """What both the oracle and the device must satisfy on a case: finite, inside the bounds, and exactly 0 where
    the restatement has underflowed below UNDERFLOW and the oracle returns 0 (the night's Mie and Rayleigh)."""
    ref = restated(eye, sun_name)
    finite = np.arange(len(got)) != NADIR
    assert np.all(np.isfinite(got[finite])) and np.all(np.isnan(got[NADIR])), (eye, sun_name)
    assert all(np.all(np.isfinite(r[finite])) and np.all(np.isnan(r[NADIR])) for r in ref if np.ndim(r)), (eye, sun_name)
    assert excess(got, ref) <= 1.0, (eye, sun_name, excess(got, ref))
    tiny = np.abs(np.concatenate([ref[0], ref[1]], axis=1)) < UNDERFLOW
    zero = tiny & (oracle_sky(eye, sun_name)[:, 0:6] == 0)
    assert np.all(np.asarray(got)[:, 0:6][zero] == 0), (eye, sun_name)


@pytest.mark.parametrize("eye", SPHERE_EYES)
def test_sky_over_the_sphere_and_at_the_sun(eye):
    for name in suns():
        check_case(oracle_sky(eye, name), eye, name)


def test_the_gate_suns_straddle_the_gate():
    gate = lambda s: -np.float64(s[1]) * 2.7 - 0.5  # noqa: E731
    assert 0 < gate(suns()["gate-"]) < 0.02 and -0.02 < gate(suns()["gate+"]) < 0
    on, off = (np.delete(oracle_sky(EYES[0], n)[:, 6], NADIR) for n in ("gate-", "gate+"))
    assert np.any(on != 0) and not np.any(off)


def test_eye_height_edges():
    """Eye.y = 5000 makes float32 camHeight equal outerRadius: far = 0, t = 0 and applyPhase's 0 / 0 reaches every
    scattering output, while the float64 restatement (camHeight 3.8e-6 short of outerRadius) stays finite.  The
    stars do not read the eye.  4999 and 5001 (SPHERE_EYES) are finite and inside the bounds."""
    for name in ("t=0.3", "t=0.05"):
        d, s = sphere_directions(name), suns()[name]
        got = O.sky(O.noise_tables(), sky_frame(NAN_EYE, s), d)
        finite = np.arange(len(d)) != NADIR
        assert np.all(np.isnan(got[:, 0:6])) and np.all(np.isfinite(got[finite, 6]))
        with np.errstate(invalid="ignore"):
            mie, ray = R.rayleigh_mie(d, np.array(NAN_EYE, np.float32), s)
        assert np.all(np.isfinite(mie[finite])) and np.all(np.isfinite(ray[finite]))
        for eye in SPHERE_EYES[-2:]:
            check_case(oracle_sky(eye, name), eye, name)


# --- the restatement before its literals had names --------------------------------------------------
def _unnamed_rayleigh_mie(dirs, eye, sun):
    """sky_ref.rayleigh_mie as it stood with its literals written out, kept to show that naming them moved no bit."""
    f32 = lambda x: np.float64(np.float32(x))  # noqa: E731
    sat = lambda x: np.clip(x, 0.0, 1.0)  # noqa: E731
    norm = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)  # noqa: E731
    scale_depth, kr, km, pi, inner = f32(0.19), f32(0.003), f32(0.0025), f32(3.14159265), 200.0
    outer = inner * f32(1.025)
    inv_wl = 1.0 / np.array([0.650, 0.570, 0.475], np.float32).astype(np.float64) ** 4
    g = f32(-0.99)
    kr_esun, km_esun, kr_4pi, km_4pi = 12.0 * kr, 12.0 * km, kr * 4.0 * pi, km * 4.0 * pi
    f_scale = 1.0 / (outer - inner)
    sosd = f_scale / scale_depth

    def scale(fcos):
        x = 1.0 - fcos
        return scale_depth * np.exp(-0.00287 + x * (0.459 + x * (3.83 + x * (-6.80 + x * 5.25))))

    org = np.asarray(dirs, np.float64).reshape(-1, 3)
    eye, sun = np.asarray(eye, np.float64), np.asarray(sun, np.float64)
    rd = np.array(org, copy=True)
    rd[:, 1] = sat(rd[:, 1])
    rd = norm(rd)
    cam_h = max(inner + eye[1] * 0.001, 0.0)
    dist_to_top = outer - cam_h
    far = dist_to_top + (1.0 - rd[:, 1]) * dist_to_top * 2.0
    start = np.array([eye[0] * 0.001, cam_h, eye[2] * 0.001])
    depth0 = np.exp(sosd * (inner - cam_h))
    start_offset = depth0 * scale(rd @ norm(start))
    sample_len = far / 3.0
    scaled_len = sample_len * f_scale
    sample_ray = rd * sample_len[:, None]
    sp = start[None, :] + sample_ray * 0.5
    front = np.zeros_like(rd)
    for _ in range(3):
        h = np.linalg.norm(sp, axis=1)
        dep = np.exp(sosd * (inner - h))
        scatter = start_offset + dep * (scale((sp @ sun) / h) - scale(np.sum(rd * sp, axis=1) / h))
        front += np.exp(-scatter[:, None] * (inv_wl * kr_4pi + km_4pi)[None, :]) * (dep * scaled_len)[:, None]
        sp = sp + sample_ray
    mie_var, ray_var = front * (inv_wl * kr_esun)[None, :], front * km_esun
    t = -rd * far[:, None]
    fcos = (t @ sun) / np.linalg.norm(t, axis=1)
    fcos2, g2 = fcos * fcos, g * g
    mie = (1.5 * ((1.0 - g2) / (2.0 + g2)) * (1.0 + fcos2) / np.power(np.abs(1.0 + g2 - 2.0 * g * fcos), 1.5))[:, None] * ray_var
    rayleigh = (0.75 + 0.75 * fcos2)[:, None] * mie_var
    rayleigh = rayleigh * sat((org[:, 1] * 0.5 + 0.5) * 4.0)[:, None]
    return mie, rayleigh + np.array([0.3, 0.4, 0.6]) * sat(sun[1])


def _unnamed_space_color(perm2d, grad, dirs, sun):
    d = R.mod_ray_dir(np.asarray(dirs, np.float64).reshape(-1, 3))
    s = R.noise3d(perm2d, grad, d * 500.0)
    s = s - (R.noise3d(perm2d, grad, d * 150.2) * 0.5 + 0.13)
    s = s - (R.noise3d(perm2d, grad, d * 200.2) * 0.5 + 0.5)
    s = s * 1.0 * np.clip(-np.asarray(sun, np.float64)[1] * 2.7 - 0.5, 0.0, 1.0)
    return np.where(d[:, 1] <= 0.0, 0.0, s)


def test_naming_the_literals_moved_no_bit():
    perm2d, grad = tables()
    d = directions()
    same = lambda a, b: np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))  # noqa: E731
    for eye in EYES:
        for t in TIMES:
            e, s = np.array(eye, np.float32), sun(t)
            for new, old in zip(R.rayleigh_mie(d, e, s), _unnamed_rayleigh_mie(d, e, s)):
                assert same(new, old), (eye, t)
            assert same(R.space_color(perm2d, grad, d, s), _unnamed_space_color(perm2d, grad, d, s)), t


# --- the mutation check --------------------------------------------------------------------------
# Mutants that stay inside every bound on every case: name -> (worst multiple of a bound, reason).
ESCAPES = {
    "sky.pi": (0.5, "3.14159266 is the same float32 as 3.14159265: not a mutant"),
    "sky.scale_c0": (0.627, "-0.00288 for -0.00287 scales every scale() by exp(-1e-5): the optical depths move by 1e-5 "
                            "of themselves, the colours by at most 1e-4 where the attenuation is e^-10, under 2 a_r"),
    "sky.cam_floor": (0.5, "saturated: max(camHeight, 0.1) is camHeight down to Eye.y = -199900, beyond the overflow"),
}


def mutant_excess(name, tweak, stop=1.0):
    """The worst multiple of a bound that the oracle reaches against the tweaked restatement; returns at the
    first case beyond `stop`."""
    worst = 0.0
    for eye in SPHERE_EYES:
        for sun_name in suns():
            worst = max(worst, excess(oracle_sky(eye, sun_name), restated(eye, sun_name, tweak, name)))
            if worst > stop:
                return worst
    return worst


def test_sky_mutants():
    """Every sky literal with its last printed digit changed by one, and every structural misreading, takes the
    oracle outside a bound on some case, or is listed in ESCAPES with the reason (and then does stay inside)."""
    wrong = []
    for name, tweak in H.mutants("sky"):
        worst = mutant_excess(name, tweak)
        if (worst > 1.0) == (name in ESCAPES):
            wrong.append((name, worst))
    assert not wrong, wrong
    names = {n for n, _ in H.mutants("sky")}
    assert set(ESCAPES) <= names
    assert {n for n in H.LITERALS if n.startswith("sky.")} | {"sky.structure=" + s for s in R.STRUCTURES} == names


def test_sky_amount_mutant():
    """tracescreen.hlsl:22's 0.0005 read as 0.0006 leaves the composite's bound on test_hlsl_kat's F0-F3 hits
    (16 of them lie beyond 1000, where (dist * 0.0005)^2 passes 0.25, and two beyond 2000, where it saturates)."""
    import test_hlsl_kat as HK
    s = HK.shaded("nomadplains")
    assert (s.pd[s.hit, 3] > 1000.0).sum() >= 16 and (s.pd[s.hit, 3] > 2000.0).sum() >= 2
    (name, tweak), = H.mutants("sample")
    assert name == "sample.sky_amount"
    ref, unsafe = H.sample_color(s.land, s.pd, s.density, s.fcolord, s.pdn, HK.F_EYE, HK.SH.SUN, s.normal32, s.shadowed,
                                 s.shadow_w, tweak)
    err = np.abs(s.res[:, :3].astype(np.float64) - ref).max(axis=1)
    assert err[s.hit][HK.kept(unsafe)[s.hit]].max() > HK.bound("composite", "nomadplains")
    assert err[s.miss].max() <= HK.bound("miss", "nomadplains")  # a miss is lerp(sky, sky, skyAmount)


def measure():
    """The figures of MEASURED from this module's own sets and the oracle: a_r, a_m and then b at the eyes whose
    outerRadius / |distToTop| is at most EYE_FAR, then c over every eye from what those three leave."""
    cases = [(eye, name) for eye in SPHERE_EYES for name in suns()]
    fig = {k: (figures(oracle_sky(*k), restated(*k)), restated(*k)[3]) for k in cases}
    low = [f for f, cond in fig.values() if cond <= EYE_FAR]
    a_r = max(f[0].max() for f in low)
    a_m = max(f[1][f[2] >= DENOM_FAR].max() for f in low)
    b = max(((f[1] - a_m) * f[2] / ULP).max() for f in low)
    c = max(max((f[0] - a_r).max(), (f[1] - a_m - b * ULP / f[2]).max()) / (ULP * cond) for f, cond in fig.values())
    return {"a_r": a_r, "a_m": a_m, "b": b, "c": c, "stars": max(f[3].max() for f, _ in fig.values())}


if __name__ == "__main__":
    import sys
    import time
    t0 = time.time()
    m = measure()
    print("measured", {k: "%.5g" % v for k, v in m.items()}, "%.1f s" % (time.time() - t0))
    if "mutants" in sys.argv and all(v is not None for v in MEASURED.values()):
        for name, tweak in H.mutants("sky"):
            t0 = time.time()
            worst = mutant_excess(name, tweak, stop=np.inf if "full" in sys.argv else 1.0)
            print("%-8s %-48s %10.3g  %.1f s" % ("killed" if worst > 1.0 else "ESCAPE", name, worst, time.time() - t0))
