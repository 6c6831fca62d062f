"""Float64 numpy restatement of the terrain shaders (TEST INFRASTRUCTURE, an independent checker).

Follows the HLSL line by line in double precision, as tests/sky_ref.py does for the sky:
    Media/common/shaders/tracing.hlsl:107-116 (getNormal), :124-134 (getPixelRay)
    Media/common/shaders/tracescreen.hlsl:16-48 (the hit and the miss composite of traceSample)
    Media/{nomadplains,simple,testing,greenrocks}/shaders/terrain.hlsl (getDensity, getFog)
    Media/{nomadplains,simple,testing,greenrocks}/shaders/color.hlsl (getColor)
noise3d (noise.hlsl:139-179), getRayleighMieColor and getSpaceColor are sky_ref's.  A literal is its float32 value
widened to float64; everything else is real-number arithmetic (numpy `**`, log2, sqrt, sin, cos).  It shares no
code, no fma rule and no polynomial with oracle/rt_oracle.c or rt_shader.h, so agreement within a tolerance pins
their arithmetic to the HLSL's real-number meaning (tests/test_hlsl_kat.py, tests/test_gpu_hlsl_kat.py).

Not restated: the march (traceRay), whose outcome is an input wherever a stage needs it (the shadow ray of
getColor: whether it hit and its fcolord.w; traceSample's rr); the AA patterns, AO and the camera matrices.
RECORDING changes only march constants.  Dead code of the HLSL whose value never reaches a result is left out
where it costs noise evaluations (getColor's blend, n1 and first FBM, color2, `s *= 30`, the `precision` of the
shadow ray, which is a march input); cheap dead terms are evaluated so that their literals stay in the table.

Loops bounded by a float `detail` (nomadplains' getDensity, simple's getColor) are the one discontinuity besides
the march: density, normal, color and sample_color return an `unsafe` mask next to the value, set where
detail > 2 lies within DETAIL_BAND of an integer (more than ten float32 ulps of a value <= 18), and tests leave
those points out.

Every literal of getDensity, getFog and getColor has a name in LITERALS (its text as the HLSL prints it, and where
it stands); `tweak={name: value}` replaces it, which is how the mutation check of test_hlsl_kat.py shows that the
bounds notice a misread constant.  Two tweaks are not numbers: "<land>.color.swizzle" ("yxz" by default) names the
coordinates of p that the colour FBM's three factors multiply.
"""
import os

import numpy as np

import sky_ref as S

LANDSCAPES = ("nomadplains", "testing", "simple", "greenrocks")
DETAIL_BAND = 1e-4
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noise_reference_msvc_seed300.npz")
_tables = None


def f32(text):
    """A literal: the float32 value of its text, widened."""
    return np.float64(np.float32(float(text)))


def tables():
    """(perm2d, grad) of seed 300 under the MSVC rand: the committed dump of the reference's own Noise.cpp."""
    global _tables
    if _tables is None:
        z = np.load(_GOLDEN)
        _tables = (np.array(z["perm2d"], np.uint8), np.array(z["grad"], np.float32).reshape(128, 4))
    return _tables


def noise3d(p, tab=None):
    perm2d, grad = tab or tables()
    return S.noise3d(perm2d, grad, p)


# ------------------------------------------------------------------------------------------------
# The literals.  name -> (text as printed in the HLSL without its f, file:line)
LITERALS = {}


def _lits(prefix, where, **kv):
    for k, v in kv.items():
        LITERALS[prefix + "." + k] = (v, where)


_T = "nomadplains/shaders/terrain.hlsl"
_lits("nomadplains.density", _T + ":10", dist_min="0.01")
_lits("nomadplains.density", _T + ":14", p_scale="0.4")
_lits("nomadplains.density", _T + ":20", detail_top="18.0", detail_exp="0.33", detail_floor="2.0")
_lits("nomadplains.density", _T + ":2,22", fbm_first="1.0", lucan="1.96", freq="0.006", y_scale="0.35")
_lits("nomadplains.density", _T + ":24", mountains="0.1")
_lits("nomadplains.density", _T + ":25", s_gain="30.0")
_lits("nomadplains.density", _T + ":26", s_offset="1.0", s_scale="35.0", s_exp="0.68")
_lits("nomadplains.density", _T + ":28", steep_freq="0.007138", steep_z="0.0", steep_bias="0.2", steep_gain="6.0",
      steep_scale="7.5")
_lits("nomadplains.density", _T + ":29", floor_scale="1.8")
_lits("nomadplains.density", _T + ":30", terrace1_y="13.0", terrace1_exp="2.0")
_lits("nomadplains.density", _T + ":31", terrace2_y="16.0", terrace2_exp="2.0")
_lits("nomadplains.density", _T + ":32", terrace3_y="19.0", terrace3_exp="2.0")
_lits("nomadplains.density", _T + ":33", terrace4_y="22.0", terrace4_exp="2.0")
_lits("nomadplains.density", _T + ":35", low_y="10.0", low_gain="1.6", low_exp="1.5", low_scale="19.0")

_T = "testing/shaders/terrain.hlsl"
_lits("testing.density", _T + ":15", x_freq="0.1", z_freq="0.1", amp="10.0")

_T = "simple/shaders/terrain.hlsl"
_lits("simple.density", _T + ":31", freq="0.006", mask_x="1.0", mask_y="0.0", mask_z="1.0", amp="150.0")
_lits("simple.density", _T + ":34", a_freq="0.002", a_half="0.5", a_bias="0.5", a_top="50.0", a_slope="1.5",
      a_floor="0.0", a_cap="36.0")
_lits("simple.density", _T + ":35", b_freq="0.003", b_half="0.5", b_bias="0.5", b_top="10.0", b_slope="1.5",
      b_floor="0.0", b_cap="36.0")
_lits("simple.density", _T + ":37", dist_min="0.01")
_lits("simple.density", _T + ":2,41", fbm_first="1.0", octaves="1.0", lucan="1.96", fbm_freq="0.06", y_scale="0.35")

_T = "greenrocks/shaders/terrain.hlsl"
_lits("greenrocks.density", _T + ":6", y_offset="170.0")
_lits("greenrocks.density", _T + ":8", d_start="0.0")
_lits("greenrocks.density", _T + ":13", g_freq="0.01")
_lits("greenrocks.density", _T + ":14", noh_x="1.0", noh_gain="1.4", noh_bias="0.1", noh_z="1.0")
_lits("greenrocks.density", _T + ":2", fbm_first="1.0", fbm_base="2.0")
_lits("greenrocks.density", _T + ":18", a_octaves="7.0", a_freq_x="0.011", a_freq_y="0.0013", a_freq_z="0.011",
      a_shift="0.32", a_amp="210.0")
_lits("greenrocks.density", _T + ":20", sub="50.0")
_lits("greenrocks.density", _T + ":22", b_octaves="5.0", b_freq="0.002", b_bias="0.1", b_half="0.5", b_add="0.5",
      b_amp="220.0")

for _land, _line in (("nomadplains", None), ("testing", 37), ("simple", 49), ("greenrocks", 33)):
    if _line is None:
        continue  # nomadplains' getFog is `return 0.0f` alone (terrain.hlsl:42-45): no literal to name
    _T = "%s/shaders/terrain.hlsl:%d-%d" % (_land, _line, _line + 20)
    _lits(_land + ".fog", _T, color_r="0.9", color_g="0.9", color_b="0.9", dist_one="1.0", dist_slope="0.0012",
          falloff_one="1.0", falloff_slope="0.1", falloff_min="0.0", y_offset="2.0", y_slope="0.0003",
          noise_freq="0.1261", noise_gain="0.2", noise_bias="0.8")

# the part of getColor the four landscapes share (nomadplains color.hlsl:45-71 and its twins)
for _land, _l0 in (("nomadplains", 45), ("testing", 17), ("simple", 47), ("greenrocks", 16)):
    _T = "%s/shaders/color.hlsl:%d-%d" % (_land, _l0, _l0 + 26)
    _lits(_land + ".color", _T, shadow_dim="0.1", fresnel_floor="0.0", spec_exp="40.0", shadow_r="0.08",
          shadow_g="0.12", shadow_b="0.14", lit="1")
for _land in ("nomadplains", "simple"):
    _T = "%s/shaders/color.hlsl" % _land
    _lits(_land + ".color", _T + (":25" if _land == "nomadplains" else ":27"), base_r="193", base_g="131",
          base_b="92", base_div="255.0")
    # nomadplains' colour FBM is terrain.hlsl's FBM_THIS (its own FBM_THIS_C goes unused), simple's is FBM_THIS_C
    _lits(_land + ".color", "nomadplains/shaders/terrain.hlsl:2" if _land == "nomadplains" else _T + ":2", fbm_first="1.0")
    _lits(_land + ".color", _T + (":43" if _land == "nomadplains" else ":45"), alpha="0.2")
_lits("nomadplains.color", "nomadplains/shaders/color.hlsl:31", octaves="20", lucan="2.03", f_y="0.5", f_x="0.01",
      f_z="0.01")
_lits("nomadplains.color", "nomadplains/shaders/color.hlsl:32", s_gain="0.5")
_lits("simple.color", "simple/shaders/color.hlsl:10", detail_top="16.0", detail_exp="0.33", detail_floor="2.0")
_lits("simple.color", "simple/shaders/color.hlsl:33", lucan="2.03", f_y="0.5", f_x="0.01", f_z="0.1")
_lits("simple.color", "simple/shaders/color.hlsl:34", fade_from="200.0", fade_over="200.0", fade_floor="0.0")
_lits("testing.color", "testing/shaders/color.hlsl:15", base_r="0.6", base_g="0.5", base_b="0.3", alpha="0.1")
_lits("greenrocks.color", "greenrocks/shaders/color.hlsl:14", base_r="0.6", base_g="0.7", base_b="0.3", alpha="0.1")

SWIZZLES = ("nomadplains.color.swizzle", "simple.color.swizzle")
# loop bounds printed with a fraction digit, which a change of that digit cannot move to another octave count
OCTAVE_BOUNDS = ("simple.density.octaves", "greenrocks.density.a_octaves", "greenrocks.density.b_octaves")


def mutate(text):
    """The literal with its last printed digit changed by one (up; a 9 goes down)."""
    d = int(text[-1])
    return text[:-1] + str(d + 1 if d < 9 else d - 1)


def mutants(prefix):
    """(name, tweak) for every literal under `prefix` ("<land>.<density|fog|color>"), last digit changed by one;
    for an OCTAVE_BOUNDS literal one octave more as well ("<name>+1"), and for a colour FBM the swap of the two
    coordinates under the small factors."""
    for name, (text, _) in LITERALS.items():
        if name.startswith(prefix + "."):
            yield name, {name: f32(mutate(text))}
            if name in OCTAVE_BOUNDS:
                yield name + "+1", {name: f32(text) + 1.0}
    if prefix + ".swizzle" in SWIZZLES:
        yield prefix + ".swizzle", {prefix + ".swizzle": "yzx"}


class _K:
    def __init__(self, prefix, tweak):
        self.prefix, self.tweak = prefix, tweak or {}
        for k in self.tweak:
            assert k in LITERALS or k in SWIZZLES, k

    def __call__(self, name):
        full = self.prefix + "." + name
        if full in self.tweak:
            return np.float64(self.tweak[full])
        return f32(LITERALS[full][0])

    def swizzle(self):
        return self.tweak.get(self.prefix + ".swizzle", "yxz")


def _sat(x):
    return np.clip(x, 0.0, 1.0)


def _lerp(a, b, t):
    return a + t * (b - a)


def _vec(a):
    return np.asarray(a, np.float64).reshape(-1, 3)


def _col(*xs):
    return np.stack(np.broadcast_arrays(*xs), axis=-1)


def _near_integer(detail, floor):
    return (detail > floor) & (np.abs(detail - np.rint(detail)) < DETAIL_BAND)


def _fbm(first, bound, term):
    """FBM_THIS (terrain.hlsl:1-2): for(N = first; N <= bound; N++) OUT += term(N, rows), bound per point."""
    bound = np.asarray(bound, np.float64)
    out = np.zeros(bound.shape)
    n = first
    while True:
        rows = np.flatnonzero(n <= bound)
        if rows.size == 0:
            return out
        out[rows] += term(n, rows)
        n = n + 1.0


# ------------------------------------------------------------------------------------------------
def _density_nomadplains(p, eye, K, tab):
    """nomadplains/shaders/terrain.hlsl:8-39"""
    dist = np.maximum(np.linalg.norm(p - eye, axis=1), K("dist_min"))  # :10
    d = -p[:, 1]  # :13
    p = p * K("p_scale")  # :14
    detail = np.maximum(K("detail_top") - dist ** K("detail_exp"), K("detail_floor"))  # :20
    unsafe = _near_integer(detail, K("detail_floor"))

    def octave(n, rows):  # :22
        sc = K("lucan") ** n
        q = p[rows] * K("freq") * _col(sc, sc * K("y_scale"), sc)
        return noise3d(q, tab) / sc

    s = _fbm(K("fbm_first"), detail, octave)
    mountains = K("mountains")  # :24
    s = s * K("s_gain")  # :25
    s = (np.abs(s + K("s_offset")) * K("s_scale")) ** (K("s_exp") + mountains)  # :26
    q = _col(p[:, 0] * K("steep_freq"), p[:, 2] * K("steep_freq"), K("steep_z"))
    steep = _sat((noise3d(q, tab) - K("steep_bias")) * K("steep_gain")) * K("steep_scale")  # :28
    floorsize = steep * K("floor_scale")  # :29
    for i in "1234":  # :30-33
        s = s - _sat((p[:, 1] - K("terrace%s_y" % i)) * steep) ** K("terrace%s_exp" % i) * floorsize
    s = s + _sat((-p[:, 1] + K("low_y")) * K("low_gain")) ** K("low_exp") * K("low_scale")  # :35
    return d + s, unsafe


def _density_testing(p, eye, K, tab):
    """testing/shaders/terrain.hlsl:6-36"""
    d = -p[:, 1]
    d = d + np.sin(p[:, 0] * K("x_freq")) * np.cos(p[:, 2] * K("z_freq")) * K("amp")  # :15
    return d, np.zeros(len(p), bool)


def _density_simple(p, eye, K, tab):
    """simple/shaders/terrain.hlsl:7-48"""
    d = -p[:, 1]
    n = noise3d(p * K("freq") * _col(K("mask_x"), K("mask_y"), K("mask_z")), tab) * K("amp")  # :31
    for t in "ab":  # :34-35
        w = np.minimum(np.maximum(K(t + "_top") - p[:, 1] * K(t + "_slope"), K(t + "_floor")), K(t + "_cap"))
        n = n - (noise3d(p * K(t + "_freq"), tab) * K(t + "_half") + K(t + "_bias")) * w
    dist = np.maximum(np.linalg.norm(p - eye, axis=1), K("dist_min"))  # :37, read by nothing
    del dist

    def octave(k, rows):  # :41
        sc = K("lucan") ** k
        q = p[rows] * K("fbm_freq") * _col(sc, sc * K("y_scale"), sc)
        return noise3d(q, tab) / sc

    n = n + _fbm(K("fbm_first"), np.full(len(p), K("octaves")), octave)
    return d + n, np.zeros(len(p), bool)


def _density_greenrocks(p, eye, K, tab):
    """greenrocks/shaders/terrain.hlsl:4-32"""
    p = p - _col(0.0, K("y_offset"), 0.0)  # :6
    d = K("d_start") - p[:, 1]  # :8-10
    g = noise3d(p * K("g_freq"), tab)  # :13
    noh = _col(K("noh_x"), np.abs(g) * K("noh_gain") + K("noh_bias"), K("noh_z"))  # :14
    fa = _col(K("a_freq_x"), K("a_freq_y"), K("a_freq_z"))

    def octave_a(n, rows):  # :18
        sc = K("fbm_base") ** n
        q = p[rows] * fa * sc + (g[rows] * K("a_shift"))[:, None]
        return np.abs(noise3d(q, tab)) * K("a_amp") * g[rows] / sc

    d = d + _fbm(K("fbm_first"), np.full(len(p), K("a_octaves")), octave_a)
    d = d - K("sub")  # :20

    def octave_b(n, rows):  # :22
        sc = K("fbm_base") ** n
        q = p[rows] * K("b_freq") * noh[rows] * sc
        return -((noise3d(q, tab) + K("b_bias")) * K("b_half") + K("b_add")) * (K("b_amp") / sc)

    d = d + _fbm(K("fbm_first"), np.full(len(p), K("b_octaves")), octave_b)
    return d, np.zeros(len(p), bool)


_DENSITY = {"nomadplains": _density_nomadplains, "testing": _density_testing, "simple": _density_simple,
            "greenrocks": _density_greenrocks}


def density(land, p, eye, tweak=None, tab=None):
    """getDensity(p) with Eye = eye: (value (n,), unsafe (n,) bool)."""
    return _DENSITY[land](_vec(p), np.asarray(eye, np.float64)[:3], _K(land + ".density", tweak), tab)


def fog(land, p, dist, tweak=None, tab=None):
    """getFog(p, dist): (n, 4).  nomadplains returns 0 (terrain.hlsl:42-45); testing (:56) and simple (:68) return
    0 before the `return f` that greenrocks (:53) reaches."""
    p = _vec(p)
    if land == "nomadplains":
        return np.zeros((len(p), 4))
    K = _K(land + ".fog", tweak)
    dist = np.asarray(dist, np.float64).reshape(-1)
    dist = _sat(K("dist_one") - dist * K("dist_slope"))
    falloff = _sat(K("falloff_one") - (dist * dist * K("falloff_slope")))
    live = falloff > K("falloff_min")
    d = np.where(live, _sat((-p[:, 1] - K("y_offset")) * K("y_slope")), 0.0)
    fogd = np.where(live, np.abs(noise3d(p * K("noise_freq"), tab)) * K("noise_gain") + K("noise_bias"), 0.0)
    rgb = _col(K("color_r"), K("color_g"), K("color_b")) * (fogd * d)[:, None]
    f = np.concatenate([rgb, d[:, None]], axis=1) * dist[:, None]
    if land != "greenrocks":
        return np.zeros_like(f)
    return f


def normal(land, pos, w, eye, tweak=None, tab=None):
    """getNormal(float4(pos, w)) (tracing.hlsl:107-116): (unit normals (n, 3), unsafe (n,))."""
    pos, eye = _vec(pos), np.asarray(eye, np.float64)[:3]
    w = np.asarray(w, np.float64).reshape(-1)
    nd = np.linalg.norm(pos - eye, axis=1) * f32("0.005")  # :109-110
    g, unsafe = [], np.zeros(len(pos), bool)
    for axis in range(3):  # :112-114
        off = np.zeros_like(pos)
        off[:, axis] = nd
        v, u = density(land, pos - off, eye, tweak, tab)
        g.append(v - w)
        unsafe |= u
    g = np.stack(g, axis=1)
    return g / np.linalg.norm(g, axis=1, keepdims=True), unsafe


def _swizzled(p, K):
    ax = ["xyz".index(c) for c in K.swizzle()]
    return _col(p[:, ax[0]] * K("f_y"), p[:, ax[1]] * K("f_x"), p[:, ax[2]] * K("f_z"))


def color(land, p, n, d, dist, sun, shadowed, shadow_fog_w, tweak=None, tab=None):
    """getColor(p, n, d, dist) with SunDirection = sun: (rgb (n, 3), unsafe (n,)).  The shadow ray's outcome is an
    input: shadowed (its rr.density > 0) and shadow_fog_w (its rr.fcolord.w)."""
    p, n, d = _vec(p), _vec(n), _vec(d)
    dist = np.asarray(dist, np.float64).reshape(-1)
    sun = np.asarray(sun, np.float64)
    K = _K(land + ".color", tweak)
    unsafe = np.zeros(len(p), bool)
    if land in ("nomadplains", "simple"):
        base = _col(K("base_r"), K("base_g"), K("base_b")) / K("base_div")  # color1
        q = _swizzled(p, K)

        def octave(k, rows):
            sc = K("lucan") ** k
            return np.abs(noise3d(q[rows] * sc, tab)) / sc

        if land == "nomadplains":  # color.hlsl:31-32
            s = _fbm(K("fbm_first"), np.full(len(p), K("octaves")), octave)
            gain = K("s_gain")
        else:  # simple color.hlsl:10, :33-34
            detail = np.maximum(K("detail_top") - dist ** K("detail_exp"), K("detail_floor"))
            unsafe = _near_integer(detail, K("detail_floor"))
            s = _fbm(K("fbm_first"), detail, octave)
            gain = np.maximum((K("fade_from") - dist) / K("fade_over"), K("fade_floor"))
        rgb = base[None, :] - (s * gain)[:, None]
        # Specular: dot(SunDirection, reflect(n, -d)), reflect(i, m) = i - 2 m dot(i, m)
        m = -d
        fresnel = (n - 2.0 * m * np.sum(n * m, axis=1, keepdims=True)) @ sun
    else:  # testing color.hlsl:15, :36; greenrocks :14, :35
        rgb = np.tile(_col(K("base_r"), K("base_g"), K("base_b")), (len(p), 1))
        fresnel = np.sum(-d * n, axis=1)
    brightness = n @ sun
    shadowed = np.asarray(shadowed, bool).reshape(-1)
    w = np.asarray(shadow_fog_w, np.float64).reshape(-1)
    brightness = np.where(shadowed, brightness * K("shadow_dim"), _sat(brightness - w))
    specular = _sat(np.maximum(fresnel, K("fresnel_floor")) ** K("spec_exp")) * K("alpha")
    rgb = rgb + specular[:, None]
    shadow = _col(K("shadow_r"), K("shadow_g"), K("shadow_b"))
    rgb = rgb * _lerp(shadow[None, :], K("lit"), brightness[:, None])
    return rgb, unsafe


def sample_color(land, pd, dens, fcolord, pdn, eye, sun, normals, shadowed, shadow_fog_w, tweak=None, tab=None):
    """traceSample's colour after the march (tracescreen.hlsl:22-39), not saturated: pd = rr.pd (n, 4),
    dens = rr.density, fcolord = rr.fcolord (n, 4), pdn the unit directions; for the hits (dens > 0) the normal and
    the shadow ray's outcome as color() takes them (rows of misses are not read).  (rgb (n, 3), unsafe (n,))."""
    pd, fc = np.asarray(pd, np.float64).reshape(-1, 4), np.asarray(fcolord, np.float64).reshape(-1, 4)
    dens, pdn = np.asarray(dens, np.float64).reshape(-1), _vec(pdn)
    perm2d, grad = tab or tables()
    sky_amount = pd[:, 3] * f32("0.0005")  # :22
    sky_amount = _sat(sky_amount * sky_amount)[:, None]  # :23
    mie, rayleigh = S.rayleigh_mie(pdn, np.asarray(eye, np.float64)[:3], sun)  # :25
    sky = mie + rayleigh + S.space_color(perm2d, grad, pdn, sun)[:, None]  # :26-27
    hit = dens > 0.0  # :29
    out = _lerp(_lerp(sky, fc[:, :3], fc[:, 3:4]), sky, sky_amount)  # :37-38
    unsafe = np.zeros(len(pd), bool)
    if hit.any():
        h = np.flatnonzero(hit)
        c, u = color(land, pd[h, :3], _vec(normals)[h], pdn[h], pd[h, 3], sun, np.asarray(shadowed).reshape(-1)[h],
                     np.asarray(shadow_fog_w).reshape(-1)[h], tweak, tab)  # :32
        c = _lerp(c, fc[h, :3], fc[h, 3:4])  # :33
        out[h] = _lerp(c, rayleigh[h], sky_amount[h])  # :35
        unsafe[h] = u
    return out, unsafe


def pixel_ray(consts, px, py):
    """getPixelRay(float2(px, py)) (tracing.hlsl:124-134) with ScreenSize = (width, height), Projection, ViewInverse
    and Eye from consts (HLSL matrices, M[row][column]): (p (n, 3), dir (n, 3))."""
    px, py = np.asarray(px, np.float64).reshape(-1), np.asarray(py, np.float64).reshape(-1)
    wide = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    proj, vinv, eye = wide(consts["projection"]).reshape(4, 4), wide(consts["view_inverse"]).reshape(4, 4), wide(consts["eye"])
    sx = ((px + 0.5) / float(consts["width"]) - 0.5) * 2.0  # :126
    sy = ((py + 0.5) / float(consts["height"]) - 0.5) * 2.0
    sx = sx * proj[1, 1]  # :127 Projection._22
    sy = sy * proj[0, 0]  # :128 Projection._11
    loc = np.stack([sx, sy, np.ones_like(sx), np.ones_like(sx)], axis=1)
    p = (loc @ vinv)[:, :3]  # :131 mul(row vector, matrix)
    return p, p - eye[None, :3]  # :132


def unorm8(x):
    """The RGBA8 code of a colour: saturate, then round(x * 255) (round half up; the tests allow one code)."""
    return np.floor(_sat(np.asarray(x, np.float64)) * 255.0 + 0.5).astype(np.int64)
