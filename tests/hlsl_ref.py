"""Float64 numpy restatement of the terrain shaders (TEST INFRASTRUCTURE, an independent checker).

Follows the HLSL line by line in double precision, as tests/sky_ref.py does for the sky:
    Media/common/shaders/tracing.hlsl:32-105 (traceRay), :107-116 (getNormal), :124-134 (getPixelRay)
    Media/common/shaders/tracescreen.hlsl:16-48 (the hit and the miss composite of traceSample)
    Media/{nomadplains,simple,testing,greenrocks}/shaders/terrain.hlsl (getDensity, getFog)
    Media/{nomadplains,simple,testing,greenrocks}/shaders/color.hlsl (getColor)
noise3d (noise.hlsl:139-179), getRayleighMieColor and getSpaceColor are sky_ref's, and so are the sky's literals
("sky.*", listed in LITERALS here) and its structural misreadings ("sky.structure").  A literal is its float32 value
widened to float64; everything else is real-number arithmetic (numpy `**`, log2, sqrt, sin, cos).  It shares no
code, no fma rule and no polynomial with oracle/rt_oracle.c or rt_shader.h, so agreement within a tolerance pins
their arithmetic to the HLSL's real-number meaning (tests/test_hlsl_kat.py, tests/test_gpu_hlsl_kat.py).

The march (traceRay, tracing.hlsl:32-105) is restated teacher-forced (march(), at the end of this module): its
branches and densities are read from the implementation under test, its own arithmetic is float64
(tests/test_march_kat.py, tests/test_gpu_march_kat.py).  No stage marches by itself: the march's outcome is an
input wherever one needs it (the shadow ray of getColor: whether it hit and its fcolord.w; traceSample's rr).
The AO extension (pcg_hash, ao_uv, ao_dir, ao_ray, ao_factor) and the AA resolve
(tracescreen.hlsl:63-75: resolve) stand at the end of this module; the AO rays' occlusion is a march's outcome and
an input like the shadow ray's (tests/test_ao_kat.py, tests/test_gpu_ao_kat.py).
Not restated: the camera matrices.  RECORDING changes only march constants.  Dead code of
the HLSL whose value never reaches a result is left out where it costs noise evaluations (getColor's blend, n1 and
first FBM, color2, `s *= 30`; the `precision` of the shadow ray is a march input, restated by shadow_ray()); cheap
dead terms are evaluated so that their literals stay in the table.

Loops bounded by a float `detail` (nomadplains' getDensity, simple's getColor) are the one discontinuity besides
the march: density, normal, color and sample_color return an `unsafe` mask next to the value, set where
detail > 2 lies within DETAIL_BAND of an integer (more than ten float32 ulps of a value <= 18), and tests leave
those points out.

Every literal of getDensity, getFog and getColor has a name in LITERALS (its text as the HLSL prints it, and where
it stands); `tweak={name: value}` replaces it, which is how the mutation check of test_hlsl_kat.py shows that the
bounds notice a misread constant; the march's literals ("march.*") and the shadow ray's ("<land>.shadow.*") stand
in the same table.  Some tweaks are not numbers: "march.structure" names one of MARCH_STRUCTURES, and
"<land>.color.swizzle" ("yxz" by default) names the coordinates of p that the colour FBM's three factors multiply;
"ao.structure", "resolve.structure" and "sky.structure" name one of AO_STRUCTURES, RESOLVE_STRUCTURES and
sky_ref.STRUCTURES.  The AO hash's literals
(INTEGER_LITERALS) are integers, printed in hexadecimal or decimal as DESIGN.md prints them, and are tweaked by
Python integers.
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

# the sky's literals ("sky.*") stand in sky_ref's table, which restates them; traceSample's own blend factor here
LITERALS.update(S.LITERALS)
_lits("sample", "common/shaders/tracescreen.hlsl:22", sky_amount="0.0005")

SWIZZLES = ("nomadplains.color.swizzle", "simple.color.swizzle")
# loop bounds printed with a fraction digit, which a change of that digit cannot move to another octave count
OCTAVE_BOUNDS = ("simple.density.octaves", "greenrocks.density.a_octaves", "greenrocks.density.b_octaves")


def mutate(text):
    """The literal with its last printed digit changed by one (up; a 9 goes down, and the F of a hexadecimal one)."""
    base = 16 if text.startswith("0x") else 10
    d = int(text[-1], base)
    return text[:-1] + "%X" % (d + 1 if d < base - 1 else d - 1)


def mutants(prefix):
    """(name, tweak) for every literal under `prefix` ("<land>.<density|fog|color>", "march", "ao", "resolve", "sky",
    "sample"), last digit changed by one;
    for an OCTAVE_BOUNDS literal one octave more as well ("<name>+1"), and for a colour FBM the swap of the two
    coordinates under the small factors."""
    for name, (text, _) in LITERALS.items():
        if name.startswith(prefix + "."):
            if name in INTEGER_LITERALS:
                yield name, {name: int(mutate(text), 0)}
                continue
            yield name, {name: f32(mutate(text))}
            if name in OCTAVE_BOUNDS:
                yield name + "+1", {name: f32(text) + 1.0}
    if prefix + ".swizzle" in SWIZZLES:
        yield prefix + ".swizzle", {prefix + ".swizzle": "yzx"}
    yield from _march_mutants(prefix)


class _K:
    def __init__(self, prefix, tweak):
        self.prefix, self.tweak = prefix, tweak or {}
        for k in self.tweak:
            assert k in LITERALS or k in SWIZZLES or k in STRUCTURES, k

    def __call__(self, name):
        full = self.prefix + "." + name
        if full in self.tweak:
            return np.float64(self.tweak[full])
        return f32(LITERALS[full][0])

    def integer(self, name):
        full = self.prefix + "." + name
        assert full in INTEGER_LITERALS, full
        return int(self.tweak[full]) if full in self.tweak else int(LITERALS[full][0], 0)

    def structure(self, allowed):
        s = self.tweak.get(self.prefix + ".structure")
        assert s is None or s in allowed, s
        return s

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
    sky_amount = pd[:, 3] * _K("sample", tweak)("sky_amount")  # :22
    sky_amount = _sat(sky_amount * sky_amount)[:, None]  # :23
    mie, rayleigh = S.rayleigh_mie(pdn, np.asarray(eye, np.float64)[:3], sun, tweak)  # :25
    sky = mie + rayleigh + S.space_color(perm2d, grad, pdn, sun, tweak)[:, None]  # :26-27
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


# ------------------------------------------------------------------------------------------------
# The march (traceRay, Media/common/shaders/tracing.hlsl:32-105), teacher-forced.
_T = "common/shaders/tracing.hlsl"
_lits("march", _T + ":32", ray_step="0.03")
_lits("march", _T + ":33", final_precision="0.02")
_lits("march", _T + ":36", recording_density_factor="0.15")
_lits("march", _T + ":37", recording_step_factor="1.001")
_lits("march", _T + ":39", density_factor="0.35")
_lits("march", _T + ":40", step_factor="1.009")
_lits("march", _T + ":54", first_one="1.0")
_lits("march", _T + ":61", mid_half="0.5")
_lits("march", _T + ":86", refine="0.3")
_lits("march", _T + ":90", stepmult_one="1.0", density_bias="5.0", stepmult_cap="0.0")
# the shadow ray of getColor, which every landscape's color.hlsl casts with the same constants
for _land, _l0 in (("nomadplains", 47), ("testing", 19), ("simple", 49), ("greenrocks", 18)):
    _T = "%s/shaders/color.hlsl" % _land
    _lits(_land + ".shadow", _T + ":%d" % _l0, mip_half="0.5", mip_floor="0")
    _lits(_land + ".shadow", _T + ":%d" % (_l0 + 3), mip_bias="3.2", mip_gain="3.0", precision_floor="1.0",
          precision_gain="8.0")
    _lits(_land + ".shadow", _T + ":%d" % (_l0 + 4), start="0.4", length="100.0")

# what only the RECORDING build reads, and what only the other reads
MARCH_RECORDING = ("march.recording_density_factor", "march.recording_step_factor")
MARCH_NOT_RECORDING = ("march.density_factor", "march.step_factor")
# structural misreadings of the loop: values of the tweak "march.structure"
MARCH_STRUCTURES = {
    "dist_minus_step": "a hit backs up by step, not lastStep (:85)",
    "laststep_before_growth": "lastStep from step before `step *= RAY_STEP_FACTOR` (:92-93)",
    "no_fog_refund": "no `f -= fogstep` on a hit (:88)",
    "fog_by_laststep": "fogstep weighted by lastStep, not step (:78)",
    "dir_not_normalised": "rayp from dir as given, without `dir /= dirLength` (:56, :71)",
    "no_dirlength_in_first_step": "the first step without dirLength (:54)",
}
MARCH_FOG = ("march.mid_half", "march.structure=no_fog_refund", "march.structure=fog_by_laststep")
TIE_BAND = 1e-5
STRUCTURES = ("march.structure", "ao.structure", "resolve.structure", "sky.structure")


def _march_mutants(prefix):
    """The structural misreadings of a prefix that has some: "<prefix>.structure=<name>"."""
    for s in {"march": MARCH_STRUCTURES, "ao": AO_STRUCTURES, "resolve": RESOLVE_STRUCTURES,
              "sky": S.STRUCTURES}.get(prefix, ()):
        yield prefix + ".structure=" + s, {prefix + ".structure": s}


def shadow_ray(land, dist, tweak=None):
    """The arguments of getColor's shadow ray (nomadplains color.hlsl:47-51 and its twins): (dist0, enddist,
    stepmod (n,)) of traceRay(p, 0.4f, SHADOW_LENGTH, precision, SunDirection, true, true) for a hit at `dist`."""
    K = _K(land + ".shadow", tweak)
    dist = np.asarray(dist, np.float64).reshape(-1)
    mipf = np.maximum(K("mip_half") * np.log2(dist), K("mip_floor"))
    precision = np.maximum((mipf - K("mip_bias")) * K("mip_gain"), K("precision_floor")) * K("precision_gain")
    return K("start"), K("length"), precision


class March:
    """What march() returns; K steps, n rays.  Index k of the (K + 1, n) arrays is the state after k steps (0: at
    loop entry); index k - 1 of the (K, n) arrays is step k."""


def march(land, p, dir, dist0, enddist, stepmod, recording, calcfog, skiprefine, d, rayp, dist, ran, tweak=None,
          tab=None):
    """traceRay (tracing.hlsl:47-105) with its branches and densities read from an implementation's own trajectory.

    p, dir (n, 3); dist0, enddist, stepmod scalars or (n,); recording, calcfog, skiprefine the build's and the call's
    flags.  Observed, step k at index k - 1: d (K, n) the density of the k-th sample, rayp (K, n, 3) its position,
    dist (K, n) the distance after the k-th update, ran (K, n) whether the ray ran a k-th step (rows that did not
    are not read, and their state stays as it was).  The branch of step k is d[k] > 0 and stepmult reads d[k]; the
    step, lastStep and f run free in float64 from line 54 on; each distance is advanced once from the observed one
    before it.  Nothing here knows of a cap on the step count.

    Returns a March with pos (K, n, 3) the predicted sample p + normalize(dir) * dist[k-1], dist (K, n) the
    predicted distance after step k, step and last_step (K + 1, n), f (K + 1, n, 4) the accumulated fog (zero
    without calcfog), cond (K + 1, n) the loop condition `dist < enddist && step > RAY_MIN_LIMIT` at the observed
    distance and the restated step, ended (K + 1, n) where skiprefine's break has ended the ray, and unsafe
    (K + 1, n) where the condition lies within TIE_BAND (relative) of a tie."""
    C = _K("march", tweak)
    structure = C.tweak.get("march.structure")
    assert structure is None or structure in MARCH_STRUCTURES, structure
    p, dir = _vec(p), _vec(dir)
    n = len(p)
    d = np.asarray(d, np.float64)
    steps = d.shape[0]
    rayp_obs, dist_obs, ran = np.asarray(rayp, np.float64), np.asarray(dist, np.float64), np.asarray(ran, bool)
    assert d.shape == dist_obs.shape == ran.shape == (steps, n) and rayp_obs.shape == (steps, n, 3)
    dist0, enddist, stepmod = (np.broadcast_to(np.asarray(v, np.float32).astype(np.float64).reshape(-1), (n,))
                               for v in (dist0, enddist, stepmod))
    ray_step = C("ray_step")  # :32
    min_limit = C("final_precision") * ray_step  # :33-34
    density_factor = C("recording_density_factor") if recording else C("density_factor")  # :35-41
    step_factor = C("recording_step_factor") if recording else C("step_factor")

    dir_length = np.linalg.norm(dir, axis=1)  # :53
    first = ray_step * stepmod * (1.0 if structure == "no_dirlength_in_first_step" else dir_length)
    step = first - dist0 * (C("first_one") - step_factor)  # :54
    last_step = step.copy()  # :55
    ndir = dir if structure == "dir_not_normalised" else dir / dir_length[:, None]  # :56
    f = np.zeros((n, 4))  # :50
    if calcfog:  # :59-63
        half = C("mid_half")
        f = f + fog(land, p + ndir * (dist0 * half)[:, None], dist0 * half, None, tab) * dist0[:, None]

    out = March()
    out.pos, out.dist = np.zeros((steps, n, 3)), np.zeros((steps, n))
    out.step, out.last_step = np.zeros((steps + 1, n)), np.zeros((steps + 1, n))
    out.f = np.zeros((steps + 1, n, 4))
    out.cond, out.unsafe, out.ended = (np.zeros((steps + 1, n), bool) for _ in range(3))
    ended = np.zeros(n, bool)

    def record(k, at):
        out.step[k], out.last_step[k], out.f[k], out.ended[k] = step, last_step, f, ended
        out.cond[k] = (at < enddist) & (step > min_limit)  # :68
        out.unsafe[k] = ((np.abs(at - enddist) <= TIE_BAND * np.maximum(1.0, np.abs(enddist)))
                         | (np.abs(step - min_limit) <= TIE_BAND * min_limit))

    at = dist0.copy()
    record(0, at)
    for k in range(steps):
        r = ran[k]
        out.pos[k] = p + ndir * at[:, None]  # :71
        dk = d[k]
        hit = r & (dk > 0.0)  # :81, observed
        air = r & ~hit
        fogstep = np.zeros((n, 4))
        if calcfog and r.any():  # :76-79
            rows = np.flatnonzero(r)
            weight = last_step if structure == "fog_by_laststep" else step
            fogstep[rows] = fog(land, rayp_obs[k][rows], at[rows], None, tab) * weight[rows, None]
        nxt = at.copy()
        step, last_step, f = step.copy(), last_step.copy(), f.copy()
        if skiprefine:  # :83
            ended = ended | hit
        else:
            back = step if structure == "dist_minus_step" else last_step
            nxt[hit] = at[hit] - back[hit]  # :85
            step[hit] = step[hit] * C("refine")  # :86
            if structure != "no_fog_refund":
                f[hit] = f[hit] - fogstep[hit]  # :88
        stepmult = C("stepmult_one") + np.abs(np.minimum(dk + C("density_bias"), C("stepmult_cap"))) ** density_factor  # :90
        before = step[air]
        step[air] = step[air] * step_factor  # :92
        last_step[air] = (before if structure == "laststep_before_growth" else step[air]) * stepmult[air]  # :93
        nxt[air] = at[air] + last_step[air]  # :94
        f[air] = f[air] + fogstep[air]  # :95
        out.dist[k] = nxt
        # the next step starts from the observed distance, not from the prediction
        at = np.where(r, dist_obs[k], at)
        record(k + 1, at)
    return out


# ------------------------------------------------------------------------------------------------
# The AO extension and the AA resolve (tracescreen.hlsl:63-75).  AO has no shader to follow:
# its definition is the paragraph of DESIGN.md, read here on its own.  The hash is integer arithmetic mod 2^32
# (Python integers, or uint64 arrays masked to 32 bits); everything after it is float64 with real sqrt, sin, cos
# and 2 pi.
_T = "DESIGN.md section 9"
_lits("ao", _T + ", the key", key_px="0x9E3779B1", key_py="0x85EBCA77", key_k="0xC2B2AE3D", pack="16")
_lits("ao", _T + ", pcg_hash", pcg_mul="747796405", pcg_add="2891336453", pcg_out="277803737", shift_top="28",
      shift_base="4", shift_out="22")
_lits("ao", _T + ", u1 and u2", shift_u="8")
_lits("ao", _T + ", the basis", up_switch="0.9", up_steep_x="0.0", up_steep_y="1.0", up_steep_z="0.0", up_x="1.0",
      up_y="0.0", up_z="0.0")
_lits("ao", _T + ", the ray", start="0.4", end="25")
_lits("ao", _T + ", the factor", strength="0.6")
_lits("resolve", "common/shaders/tracescreen.hlsl:63", start="0.0")
_lits("resolve", "common/shaders/tracescreen.hlsl:75", alpha="1.0")
INTEGER_LITERALS = tuple("ao." + k for k in ("key_px", "key_py", "key_k", "pack", "pcg_mul", "pcg_add", "pcg_out",
                                             "shift_top", "shift_base", "shift_out", "shift_u")) + S.INTEGER_LITERALS
AO_STRUCTURES = {
    "swap_u": "u1 and u2 exchanged",
    "uniform_hemisphere": "sz = 1 - u1, r = sqrt(1 - sz^2): uniform over the hemisphere, not cosine-weighted",
    "rehash_key": "h2 = pcg(key + 1), not pcg(h)",
    "left_handed": "ty = tx x n",
    "k_major": "k * 16 + a in the key",
    "swap_pixel": "px and py exchanged in the key",
    "fog_on": "the AO ray marched with fog on",
    "refine": "the AO ray marched with skiprefine off",
}
RESOLVE_STRUCTURES = {
    "ao_inside_saturate": "saturate(c * ao)",
    "ao_on_misses": "the AO factor applied to sky samples too",
    "saturate_after_mean": "saturate(sum c_a / A)",
}
_M32 = 0xFFFFFFFF


def _words(x):
    """(x, the constructor of a constant): Python integers stay so; arrays become uint64, whose products of two
    32-bit words cannot overflow."""
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64), np.uint64
    return int(x), int


def pcg_hash(x, tweak=None):
    """pcg_hash of 32-bit words: st = x * 747796405 + 2891336453; w = ((st >> ((st >> 28) + 4)) ^ st) * 277803737;
    (w >> 22) ^ w, all mod 2^32.  x: a Python integer or an integer array (any shape, at least 1-d)."""
    K = _K("ao", tweak)
    x, c = _words(x)
    m = c(_M32)
    st = (x * c(K.integer("pcg_mul")) + c(K.integer("pcg_add"))) & m
    w = (((st >> ((st >> c(K.integer("shift_top"))) + c(K.integer("shift_base")))) ^ st) * c(K.integer("pcg_out"))) & m
    return ((w >> c(K.integer("shift_out"))) ^ w) & m


def ao_key(px, py, a, k, tweak=None):
    """(px * 0x9E3779B1) ^ (py * 0x85EBCA77) ^ ((a * 16 + k) * 0xC2B2AE3D) mod 2^32."""
    K = _K("ao", tweak)
    s = K.structure(AO_STRUCTURES)
    (px, c), py, a, k = _words(px), _words(py)[0], _words(a)[0], _words(k)[0]
    if s == "swap_pixel":
        px, py = py, px
    if s == "k_major":
        a, k = k, a
    m = c(_M32)
    return ((((px & m) * c(K.integer("key_px"))) & m) ^ (((py & m) * c(K.integer("key_py"))) & m)
            ^ (((a * c(K.integer("pack")) + k) * c(K.integer("key_k"))) & m))


def ao_uv(px, py, a, k, tweak=None):
    """(u1, u2) of AO ray k of AA sample a of pixel (px, py): the top 24 bits of two successive hashes, over 2^24."""
    K = _K("ao", tweak)
    s = K.structure(AO_STRUCTURES)
    key = ao_key(px, py, a, k, tweak)
    h = pcg_hash(key, tweak)
    h2 = pcg_hash((key + 1) & _words(key)[1](_M32), tweak) if s == "rehash_key" else pcg_hash(h, tweak)
    shift = _words(h)[1](K.integer("shift_u"))
    u1, u2 = ((np.asarray(v >> shift).astype(np.float64)) * 2.0 ** -24 for v in (h, h2))
    return (u2, u1) if s == "swap_u" else (u1, u2)


def ao_dir(n, px, py, a, k, tweak=None):
    """The direction of that AO ray about the normal n (m, 3), used as given: (m, 3) float64."""
    K = _K("ao", tweak)
    s = K.structure(AO_STRUCTURES)
    n = _vec(n)
    u1, u2 = ao_uv(px, py, a, k, tweak)
    r, sz = np.sqrt(u1), np.sqrt(1.0 - u1)
    if s == "uniform_hemisphere":
        sz = 1.0 - u1
        r = np.sqrt(1.0 - sz * sz)
    phi = u2 * (2.0 * np.pi)
    sx, sy = r * np.cos(phi), r * np.sin(phi)
    steep = np.abs(n[:, 0]) > K("up_switch")
    up = np.where(steep[:, None], _col(K("up_steep_x"), K("up_steep_y"), K("up_steep_z"))[None, :],
                  _col(K("up_x"), K("up_y"), K("up_z"))[None, :])
    tx = np.cross(up, n)
    tx = tx / np.linalg.norm(tx, axis=1, keepdims=True)
    ty = np.cross(tx, n) if s == "left_handed" else np.cross(n, tx)
    return tx * np.reshape(sx, (-1, 1)) + ty * np.reshape(sy, (-1, 1)) + n * np.reshape(sz, (-1, 1))


def ao_ray(dist, tweak=None, land="nomadplains"):
    """The arguments of an AO ray's march from a hit at `dist`: (dist0, enddist, stepmod (n,), calcfog, skiprefine,
    max_steps) of traceRay(hit, 0.4, 25, the shadow ray's precision, dir, no fog, skiprefine), with no step cap."""
    K = _K("ao", tweak)
    s = K.structure(AO_STRUCTURES)
    return K("start"), K("end"), shadow_ray(land, dist)[2], s == "fog_on", s != "refine", 0


def ao_factor(occ, samples, tweak=None):
    """1 - 0.6 * occ / K for occ occluded rays of K."""
    K = _K("ao", tweak)
    return 1.0 - K("strength") * np.asarray(occ, np.float64) / float(samples)


def resolve(samples, ao, hit, tweak=None):
    """CSMain's pixel (tracescreen.hlsl:63-75) with the AO extension: samples (n, A, 3) traceSample's colours, ao
    (n, A) each sample's AO factor (read for the hits alone), hit (n, A).  sum_a saturate(c_a) * (ao_a if hit_a else
    1) / A, alpha 1: (n, 4)."""
    K = _K("resolve", tweak)
    s = K.structure(RESOLVE_STRUCTURES)
    c = np.asarray(samples, np.float64)
    n, count = c.shape[:2]
    assert c.shape == (n, count, 3)
    ao, hit = np.asarray(ao, np.float64).reshape(n, count), np.asarray(hit, bool).reshape(n, count)
    f = (ao if s == "ao_on_misses" else np.where(hit, ao, 1.0))[:, :, None]
    color = np.full((n, 3), K("start"))  # :63
    for a in range(count):  # :67-72
        if s == "saturate_after_mean":
            color = color + c[:, a] * f[:, a]
        elif s == "ao_inside_saturate":
            color = color + _sat(c[:, a] * f[:, a])
        else:
            color = color + _sat(c[:, a]) * f[:, a]
    color = color / float(count)  # :74
    if s == "saturate_after_mean":
        color = _sat(color)
    return np.concatenate([color, np.full((n, 1), K("alpha"))], axis=1)  # :75
