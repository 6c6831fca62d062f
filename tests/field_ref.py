"""The checker of the field queries (TEST INFRASTRUCTURE): densities from the oracle's ro_get_density_batch with
the frame's eye set as surface_ref.trace sets it, normals from stage_ref.normal (the oracle's get_normal), lattice
points formed in float64 and rounded once, occupancy words from numpy's packbits.  Results are computed once per
argument set and handed out read-only."""
from fractions import Fraction

import numpy as np

import oracle_lib as O
import shade_ref as SH
import stage_ref as ST

_cache = {}


def field(points, eye, landscape, normals=False):
    """The definition in include/frosttrace.h: (n,) float32 densities, or with normals (n, 4) float32 rows
    getNormal(float4(p, d)), d -- the normal for every point, inside or outside."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    d = O.density(O.noise_tables(), SH.frame(eye, landscape), p)
    if not normals:
        return d
    n = ST.normal(landscape, p, d, eye)
    return np.ascontiguousarray(np.concatenate([n, d[:, None]], axis=1), np.float32)


def cached(key, points, eye, landscape, normals=False):
    """field() once per (key, landscape, normals); key names the points and the eye."""
    k = (key, landscape, normals)
    if k not in _cache:
        r = field(points, eye, landscape, normals)
        r.setflags(write=False)
        _cache[k] = r
    return _cache[k]


def lattice_axis(origin, spacing, n):
    """fmaf((float)i, spacing, origin) for i < n: origin + i * spacing formed in float64 and rounded ONCE to
    float32.  That is the fused result when the float64 value is exact; asserted here by the condition the issue
    states (|origin| < 2^14, |spacing| 0 or >= 2^-12, n <= 4096) and, value by value, in rational arithmetic."""
    o, s = np.float32(origin), np.float32(spacing)
    assert abs(float(o)) < 2.0 ** 14 and (s == 0 or abs(float(s)) >= 2.0 ** -12) and 0 <= n <= 4096, (origin, spacing, n)
    v = np.float64(o) + np.arange(n, dtype=np.float64) * np.float64(s)
    fo, fs = Fraction(float(o)), Fraction(float(s))
    for i in (range(n) if n <= 128 else list(range(64)) + list(range(n - 64, n)) + list(range(64, n - 64, 37))):
        assert Fraction(float(v[i])) == fo + i * fs, (origin, spacing, i)
    return v.astype(np.float32)


def lattice_points(origin, spacing, dims):
    """The lattice's points in result order (iz * ny + iy) * nx + ix: (nx ny nz, 3) float32."""
    nx, ny, nz = (int(v) for v in dims)
    x, y, z = (lattice_axis(origin[a], spacing[a], n) for a, n in enumerate((nx, ny, nz)))
    p = np.empty((nz, ny, nx, 3), np.float32)
    p[..., 0] = x[None, None, :]
    p[..., 1] = y[None, :, None]
    p[..., 2] = z[:, None, None]
    return p.reshape(-1, 3)


def occupancy_words(density, dims):
    """One bit per lattice point, density > 0, in uint32 words: (nz, ny, ceil(nx / 32)), bit ix % 32 of word
    ix // 32, the padding bits 0."""
    nx, ny, nz = (int(v) for v in dims)
    inside = (np.asarray(density, np.float32).reshape(nz, ny, nx) > 0)
    words = (nx + 31) // 32
    bits = np.zeros((nz, ny, words * 32), np.uint8)
    bits[..., :nx] = inside
    return np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little")).view("<u4").reshape(nz, ny, words)


def lattice(key, origin, spacing, dims, eye, landscape, normals=False):
    """(points, results) of the lattice, the results shaped (nz, ny, nx[, 4]); cached under key."""
    nx, ny, nz = (int(v) for v in dims)
    p = lattice_points(origin, spacing, dims)
    r = cached(key, p, eye, landscape, normals)
    return p, r.reshape((nz, ny, nx, 4) if normals else (nz, ny, nx))
