"""Float64 numpy restatement of the reference sky (TEST INFRASTRUCTURE, an independent checker).

Follows Media/common/shaders/sky.hlsl line by line in double precision with exact
transcendentals (numpy exp / power), and Media/common/shaders/noise.hlsl:139-179 (the live
`#if 1` noise3d) for the star field, on the perm2D / permGradients tables the caller passes.
It shares no code and no evaluation rule with oracle/rt_oracle.c (float32, fixed fma and
polynomial conventions), so agreement within a tolerance pins the oracle's sky arithmetic to the
HLSL's real-number meaning.

Every literal of sky.hlsl:1-16, :26-55, :74-80 and :83-137 has a name in LITERALS ("sky.<name>": its
text as the HLSL prints it without the f, and where it stands), which tests/hlsl_ref.py lists in its own
table; `tweak={name: value}` replaces one, and "sky.structure" names one of STRUCTURES, a misreading of
the shader's structure.  With no tweak the functions return the bits they returned before the literals
had names: a literal is its float32 value widened, except those in DECIMAL, which this restatement has
always read as the float64 value of the printed decimal (at most 6e-8 of the literal away from its
float32 value, three orders below any bound held against it).
"""
import numpy as np

LITERALS = {}


def _lits(where, **kv):
    for k, v in kv.items():
        LITERALS["sky." + k] = (v, "common/shaders/sky.hlsl:" + where)


_lits("2", fSamples="3.0")
_lits("4", nSamples="3")
_lits("6", scaleDepth="0.19")
_lits("7", eSpace="1.0")
_lits("8", eSun="12.0")
_lits("9", kr="0.003")
_lits("10", km="0.0025")
_lits("11", pi="3.14159265")
_lits("12", innerRadius="200.0")
_lits("13", outer_factor="1.025")
_lits("14", wavelength_r="0.650", wavelength_g="0.570", wavelength_b="0.475")
_lits("15", wavelength_exp="4")
_lits("16", g="-0.99")
_lits("29", space_horizon="0.0")
_lits("32", space_freq1="500.0")
_lits("33", space_freq2="150.2", space_gain2="0.5", space_bias2="0.13")
_lits("34", space_freq3="200.2", space_gain3="0.5", space_bias3="0.5")
_lits("35", space_sun_gain="2.7", space_sun_bias="0.5")
_lits("41", scale_one="1.0")
_lits("42", scale_c0="-0.00287", scale_c1="0.459", scale_c2="3.83", scale_c3="-6.80", scale_c4="5.25")
_lits("48", mie_front="1.5", mie_num_one="1.0", mie_num_two="2.0", mie_cos_one="1.0", mie_den_one="1.0",
      mie_den_two="2.0", mie_exp="1.5")
_lits("54", rayleigh_bias="0.75", rayleigh_gain="0.75")
_lits("74", inv_wavelength_one="1.0")
_lits("77", kr_four="4.0")
_lits("78", km_four="4.0")
_lits("79", scale_num="1.0")
_lits("89", eye_y_scale="0.001")
_lits("90", cam_floor="0.0")
_lits("93", far_one="1.0", far_two="2.0")
_lits("96", eye_x_scale="0.001", eye_z_scale="0.001")
_lits("106", first_sample="0.5")
_lits("132", fade_gain="0.5", fade_bias="0.5", fade_scale="4.0")
_lits("133", day_b="0.6")
_lits("134", day_g="0.4")
_lits("135", day_r="0.3")

INTEGER_LITERALS = ("sky.nSamples",)
# read as the float64 value of the decimal, as this module always has (see the module docstring)
DECIMAL = frozenset("sky." + k for k in (
    "scale_c0", "scale_c1", "scale_c2", "scale_c3", "scale_c4", "eye_x_scale", "eye_y_scale", "eye_z_scale",
    "day_r", "day_g", "day_b", "space_freq2", "space_bias2", "space_freq3", "space_sun_gain"))

# structural misreadings: values of the tweak "sky.structure"
STRUCTURES = {
    "phase_args_as_named": "applyPhase(rayleigh, mie, t): the arguments in the order their names suggest, not :131's",
    "no_saturate_in_modraydir": "modRayDir normalises rayDir as given (:21)",
    "fade_on_clamped_dir": ":132 fades on rayDir.y, not orgRayDir.y",
    "t_plus": "t = +rayDir * far (:129)",
    "first_sample_whole": "samplePoint = start + sampleRay, no 0.5 (:106)",
    "g_for_g2": "getMiePhase(fCos, fCos2, g, g) (:69)",
    "scale_on_fcos": "scale() of fCos itself, x = fCos (:41)",
    "day_hack_unsaturated": "the day hack adds SunDirection.y unsaturated (:133-135)",
    "start_angle_unnormalised": "fStartAngle = dot(rayDir, start) (:99)",
    "angles_not_over_height": "fLightAngle, fCameraAngle without `/ height` (:115-116)",
    "loop_depth_from_camheight": "the loop's depth from camHeight, not the sample's height (:113)",
    "km4pi_times_inv_wavelength": "attenuate's exponent v3InvWavelength * (fKr4PI + fKm4PI) (:120)",
    "stars_gate_plus": "the stars' gate saturate(SunDirection.y * 2.7 - 0.5) (:35)",
    "stars_all_added": "space = n1 + (n2 * 0.5 + 0.13) + (n3 * 0.5 + 0.5) (:33-34)",
    "space_horizon_on_original": "`if (dir.y <= 0)` on the direction as given, before modRayDir (:28-29)",
}


def f32(text):
    """A literal: the float32 value of its text, widened."""
    return np.float64(np.float32(float(text)))


class _K:
    def __init__(self, tweak):
        self.tweak = tweak or {}

    def __call__(self, name):
        full = "sky." + name
        if full in self.tweak:
            return np.float64(self.tweak[full])
        text = LITERALS[full][0]
        return np.float64(float(text)) if full in DECIMAL else f32(text)

    def integer(self, name):
        full = "sky." + name
        assert full in INTEGER_LITERALS, full
        return int(self.tweak[full]) if full in self.tweak else int(LITERALS[full][0])

    def structure(self):
        s = self.tweak.get("sky.structure")
        assert s is None or s in STRUCTURES, s
        return s


class _Consts:
    """sky.hlsl:1-16 and :74-80 (const static)."""

    def __init__(self, K):
        self.scale_depth = K("scaleDepth")
        self.inner = K("innerRadius")
        self.outer = self.inner * K("outer_factor")  # :13
        wavelength = np.array([K("wavelength_r"), K("wavelength_g"), K("wavelength_b")])
        self.inv_wavelength = K("inv_wavelength_one") / wavelength ** K("wavelength_exp")  # :15, :74
        self.kr_esun = K("eSun") * K("kr")
        self.km_esun = K("eSun") * K("km")
        self.kr_4pi = K("kr") * K("kr_four") * K("pi")
        self.km_4pi = K("km") * K("km_four") * K("pi")
        self.f_scale = K("scale_num") / (self.outer - self.inner)
        self.scale_over_scale_depth = self.f_scale / self.scale_depth


def _sat(x):
    return np.clip(x, 0.0, 1.0)


def _normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def mod_ray_dir(d, tweak=None):
    """sky.hlsl:18-23"""
    d = np.array(d, np.float64, copy=True)
    if _K(tweak).structure() != "no_saturate_in_modraydir":
        d[..., 1] = _sat(d[..., 1])
    return _normalize(d)


def _scale(fcos, K, C):
    """sky.hlsl:39-43"""
    x = fcos if K.structure() == "scale_on_fcos" else K("scale_one") - fcos
    return C.scale_depth * np.exp(K("scale_c0") + x * (K("scale_c1") + x * (K("scale_c2") + x * (K("scale_c3") + x * K("scale_c4")))))


def mie_denominator(fcos, g, g2, K):
    """The base of getMiePhase's pow (sky.hlsl:48), which falls to (1 + g)^2 = 1e-4 along SunDirection."""
    return np.abs(K("mie_den_one") + g2 - K("mie_den_two") * g * fcos)


def _mie_phase(fcos, fcos2, g, g2, K):
    """sky.hlsl:46-49"""
    return (K("mie_front") * ((K("mie_num_one") - g2) / (K("mie_num_two") + g2)) * (K("mie_cos_one") + fcos2)
            / np.power(mie_denominator(fcos, g, g2, K), K("mie_exp")))


def rayleigh_mie(dirs, eye, sun, tweak=None, conditioning=False):
    """getRayleighMieColor (sky.hlsl:83-137), applyPhase (:62-72) with the call's argument order
    (:131: applyPhase(mie, rayleigh, t) into the parameters (rayleigh, mie, camDir)).
    dirs (n, 3); returns (mie (n, 3), rayleigh (n, 3)), and with `conditioning` the two quantities whose
    float32 rounding the result magnifies: the base of getMiePhase's pow (n,), and outerRadius / |distToTop|
    (:92: a difference of two numbers near 205, which every output is proportional to)."""
    K = _K(tweak)
    C = _Consts(K)
    s = K.structure()
    org = np.asarray(dirs, np.float64).reshape(-1, 3)
    eye = np.asarray(eye, np.float64)
    sun = np.asarray(sun, np.float64)
    rd = mod_ray_dir(org, tweak)
    cam_h = max(C.inner + eye[1] * K("eye_y_scale"), K("cam_floor"))
    dist_to_top = C.outer - cam_h
    far = dist_to_top + (K("far_one") - rd[:, 1]) * dist_to_top * K("far_two")
    start = np.array([eye[0] * K("eye_x_scale"), cam_h, eye[2] * K("eye_z_scale")])
    depth0 = np.exp(C.scale_over_scale_depth * (C.inner - cam_h))
    start_angle = rd @ (start if s == "start_angle_unnormalised" else _normalize(start))
    start_offset = depth0 * _scale(start_angle, K, C)
    sample_len = far / K("fSamples")
    scaled_len = sample_len * C.f_scale
    sample_ray = rd * sample_len[:, None]
    sp = start[None, :] + (sample_ray if s == "first_sample_whole" else sample_ray * K("first_sample"))
    front = np.zeros_like(rd)
    if s == "km4pi_times_inv_wavelength":
        extinction = C.inv_wavelength * (C.kr_4pi + C.km_4pi)
    else:
        extinction = C.inv_wavelength * C.kr_4pi + C.km_4pi
    for _ in range(K.integer("nSamples")):
        h = np.linalg.norm(sp, axis=1)
        dep = depth0 if s == "loop_depth_from_camheight" else np.exp(C.scale_over_scale_depth * (C.inner - h))
        over = 1.0 if s == "angles_not_over_height" else h
        light = (sp @ sun) / over
        camera = np.sum(rd * sp, axis=1) / over
        scatter = start_offset + dep * (_scale(light, K, C) - _scale(camera, K, C))
        att = np.exp(-scatter[:, None] * extinction[None, :])
        front += att * (dep * scaled_len)[:, None]
        sp = sp + sample_ray
    mie_var = front * (C.inv_wavelength * C.kr_esun)[None, :]
    ray_var = front * C.km_esun
    t = rd * far[:, None] if s == "t_plus" else -rd * far[:, None]
    # applyPhase(rayleigh := mie_var, mie := ray_var, camDir := t)
    if s == "phase_args_as_named":
        mie_var, ray_var = ray_var, mie_var
    fcos = (t @ sun) / np.linalg.norm(t, axis=1)
    fcos2 = fcos * fcos
    g = K("g")
    g2 = g if s == "g_for_g2" else g * g
    mie = _mie_phase(fcos, fcos2, g, g2, K)[:, None] * ray_var
    rayleigh = (K("rayleigh_bias") + K("rayleigh_gain") * fcos2)[:, None] * mie_var
    fade_y = rd[:, 1] if s == "fade_on_clamped_dir" else org[:, 1]
    rayleigh = rayleigh * _sat((fade_y * K("fade_gain") + K("fade_bias")) * K("fade_scale"))[:, None]
    sy = sun[1] if s == "day_hack_unsaturated" else _sat(sun[1])
    rayleigh = rayleigh + np.array([K("day_r"), K("day_g"), K("day_b")]) * sy
    if conditioning:
        return mie, rayleigh, mie_denominator(fcos, g, g2, K), C.outer / abs(dist_to_top)
    return mie, rayleigh


def noise3d(perm2d, grad, p):
    """noise.hlsl:139-179 (live block) in float64: perm2d (128*128*4) uint8, grad (128, 4)."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    P = np.floor(p)
    f = p - P
    u = f * f * f * (f * (f * 6.0 - 15.0) + 10.0)
    X, Y, Z = [(P[:, i].astype(np.int64) & 127) for i in range(3)]
    tex = perm2d.reshape(128, 128, 4)[Y, X].astype(np.int64)  # texel (x, y) at (x + y*128)*4
    g = np.asarray(grad, np.float64).reshape(128, 4)[:, :3]

    def gp(idx, x, y, z):
        gg = g[idx % 128]
        return gg[:, 0] * x + gg[:, 1] * y + gg[:, 2] * z

    x, y, z = f[:, 0], f[:, 1], f[:, 2]
    A, AB, B, BB = [tex[:, i] + Z for i in range(4)]  # Pu = texel + P.z (noise.hlsl:166)
    lerp = lambda a, b, t: a + t * (b - a)  # noqa: E731
    l0 = lerp(lerp(gp(A, x, y, z), gp(B, x - 1, y, z), u[:, 0]),
              lerp(gp(AB, x, y - 1, z), gp(BB, x - 1, y - 1, z), u[:, 0]), u[:, 1])
    l1 = lerp(lerp(gp(A + 1, x, y, z - 1), gp(B + 1, x - 1, y, z - 1), u[:, 0]),
              lerp(gp(AB + 1, x, y - 1, z - 1), gp(BB + 1, x - 1, y - 1, z - 1), u[:, 0]), u[:, 1])
    return lerp(l0, l1, u[:, 2])


def space_color(perm2d, grad, dirs, sun, tweak=None):
    """getSpaceColor (sky.hlsl:26-36): 0 below the horizon."""
    K = _K(tweak)
    s = K.structure()
    org = np.asarray(dirs, np.float64).reshape(-1, 3)
    d = mod_ray_dir(org, tweak)
    sun_y = np.asarray(sun, np.float64)[1]
    n1 = noise3d(perm2d, grad, d * K("space_freq1"))
    n2 = noise3d(perm2d, grad, d * K("space_freq2")) * K("space_gain2") + K("space_bias2")
    n3 = noise3d(perm2d, grad, d * K("space_freq3")) * K("space_gain3") + K("space_bias3")
    sp = n1 + n2 + n3 if s == "stars_all_added" else n1 - n2 - n3
    gate = sun_y * K("space_sun_gain") - K("space_sun_bias") if s == "stars_gate_plus" \
        else -sun_y * K("space_sun_gain") - K("space_sun_bias")
    sp = sp * K("eSpace") * _sat(gate)
    below = (org if s == "space_horizon_on_original" else d)[:, 1] <= K("space_horizon")
    return np.where(below, 0.0, sp)
