"""The exact-camera fixture of the ray-query tests (TEST INFRASTRUCTURE).

The oracle evaluates camerarays.hlsl:12-21 for the 1024 prepass rays of a camera; it takes no rays.  For the
cameras here every operation of getPixelRay (tracing.hlsl:124-134) and of `p - Eye` is exact in binary32, so the
rays the oracle forms inside are known bit for bit, fused or not: width = height = 256, Projection all zero but
_11 = _22 = 1, ViewInverse rows 0-2 = R0, R1, R2 (w = 0) and row 3 = (T, 1).  For cell i (tx = i % 32,
ty = i / 32), in float32:
    px = uint32((tx * (1/31)) * 256),  sx = ((px + 0.5) / 256 - 0.5) * 2,  sy likewise from ty
    origin = T + (R2 + (sy * R1 + sx * R0)),  dir = origin - E
rays() computes them in float64 and step by step in float32 and asserts the two are equal: the condition that
makes the oracle's internal rays known.
"""
import ctypes as C

import numpy as np

import oracle_lib as O

f32 = np.float32
SIZE = 256
_F_AXES = ((1, 0, -0.5), (0, -1, -0.5), (0.5, -0.5, 1))
# name -> (E, T, R0, R1, R2)
CAMERAS = {
    "F0": ((0, 100, 0), (0, 100, 0)) + _F_AXES,
    "F1": ((0, 100, 0), (0, 100, 0), (1, 0, 0), (0, 0, 1), (0, 1.5, 0)),
    "F2": ((0, 100, 0), (4, 40, 4)) + _F_AXES,
    "F3": ((0, 100, 0), (-8, 96, 2), (0, 0.5, 1), (1, 0.25, 0), (-1, -0.25, 0.5)),
    "G": ((13, 92, -9.5), (16, 90, -8), (0.5, 0, 1), (0, -1, 0.25), (1, -0.75, -0.5)),
    "Z": ((0.5, 99.5, 1), (0, 100, 0), (0, 0, 0), (0, 0, 0), (0.5, -0.5, 1)),
}
F_SET = ("F0", "F1", "F2", "F3")  # one eye: their 4096 rays form one query
LANDSCAPES = ("nomadplains", "testing", "simple", "greenrocks")
FAR = 5000.0


def camera(name, shift=(0, 0, 0)):
    """(E, T, R0, R1, R2) as float64 rows; shift moves T (the bench's cameras: F0 moved by multiples of (8, 0, 8))."""
    e, t, r0, r1, r2 = (np.array(v, np.float64) for v in CAMERAS[name])
    return e, t + np.array(shift, np.float64), r0, r1, r2


def screen_coords():
    """(sx, sy) of the 1024 prepass cells, float32, by k_camerarays' / the oracle's operations."""
    i = np.arange(1024)
    out = []
    for t in (i % 32, i // 32):
        px = ((t.astype(f32) * (f32(1) / f32(31))) * f32(SIZE)).astype(np.uint32)
        s = ((px.astype(f32) + f32(0.5)) / f32(SIZE) - f32(0.5)) * f32(2)
        out.append(s.astype(f32))
    return out[0], out[1]


def rays(name, shift=(0, 0, 0)):
    """(origins, dirs) (1024, 3) float32 of the camera's prepass rays; asserts the float32 evaluation is exact."""
    e, t, r0, r1, r2 = camera(name, shift)
    sx, sy = screen_coords()
    sx64, sy64 = sx.astype(np.float64)[:, None], sy.astype(np.float64)[:, None]
    o64 = t + (r2 + (sy64 * r1 + sx64 * r0))
    d64 = o64 - e
    e32, t32, a0, a1, a2 = (v.astype(f32) for v in (e, t, r0, r1, r2))
    for v64, v32 in ((e, e32), (t, t32), (r0, a0), (r1, a1), (r2, a2)):
        assert np.array_equal(v64, v32.astype(np.float64)), name
    sxr0 = (sx[:, None] * a0).astype(f32)               # sx * m[0..2]
    inner = (sy[:, None] * a1).astype(f32)              # the fma's product, then its sum, each rounded ...
    inner = (inner + sxr0).astype(f32)
    o32 = (t32 + (a2 + inner).astype(f32)).astype(f32)
    d32 = (o32 - e32).astype(f32)
    # ... and exactly representable at every step, so rounding once per fma or once per operation is the same
    assert np.array_equal((sy64 * r1), (sy[:, None] * a1).astype(f32).astype(np.float64)), name
    assert np.array_equal(sy64 * r1 + sx64 * r0, inner.astype(np.float64)), name
    assert np.array_equal(r2 + (sy64 * r1 + sx64 * r0), (a2 + inner).astype(f32).astype(np.float64)), name
    assert np.array_equal(o64, o32.astype(np.float64)), name
    assert np.array_equal(d64, d32.astype(np.float64)), name
    return o32, d32


def eye(name):
    return np.array(CAMERAS[name][0], f32)


def consts(name, shift=(0, 0, 0)):
    """The camera as frame constants (FixedCamera / O.make_frame): HLSL matrices, M[r][c]."""
    e, t, r0, r1, r2 = camera(name, shift)
    vinv = np.zeros((4, 4), f32)
    vinv[0, :3], vinv[1, :3], vinv[2, :3], vinv[3, :3], vinv[3, 3] = r0, r1, r2, t, 1
    proj = np.zeros((4, 4), f32)
    proj[0, 0] = proj[1, 1] = 1
    return {"width": SIZE, "height": SIZE, "eye": np.array([e[0], e[1], e[2], 0], f32), "view_inverse": vinv,
            "projection": proj, "sun": np.array([0.0, -1.0, 0.0], f32)}


_oracle = {}


def oracle(name, landscape):
    """(results (1024, 4) float32, steps (1024,) uint32) of ro_camerarays_steps for the camera; computed once."""
    key = (name, landscape)
    if key not in _oracle:
        fr = O.make_frame(consts(name), landscape=O.LANDSCAPES[landscape])
        cr = np.zeros(1024 * 4, f32)
        st = np.zeros(1024, f32)
        O.lib().ro_camerarays_steps(C.byref(O.noise_tables()), C.byref(fr), O._fp(cr), O._fp(st), C.byref(O.Stats()))
        res, steps = cr.reshape(1024, 4), st.astype(np.uint32)
        res.setflags(write=False)
        steps.setflags(write=False)
        _oracle[key] = (res, steps)
    return _oracle[key]


def query(names):
    """(origins, dirs) of the cameras' rays, concatenated."""
    parts = [rays(n) for n in names]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def oracle_query(names, landscape):
    parts = [oracle(n, landscape) for n in names]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
