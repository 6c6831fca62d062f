"""The checker of the mesh extraction (TEST INFRASTRUCTURE): the definition in include/frosttrace.h (section "mesh
extraction") restated in numpy float32 from a density array shaped (nz, ny, nx).  Every float32 step is one numpy
float32 operation (IEEE add, subtract and divide, correctly rounded); the fmaf of the world coordinate is formed in
float64 where that sum is exact (checked value by value with TwoSum) and in rational arithmetic otherwise, as
field_ref.lattice_axis argues.  Normals come from field_ref.field (the oracle's density and get_normal)."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import field_ref as FR

F32 = np.float32
_cache = {}


def _round32(x):
    """A Fraction rounded once to float32, ties to even."""
    c = F32(float(x))  # (rounded twice: at most one float32 off)
    best = None
    for cand in (np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - x)
        even = (int(np.array(cand, F32).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[1]):
            best = (err, even, cand)
    return best[2]


def fma32(a, s, o):
    """fmaf(a, s, o) per element of the float32 array a with float32 scalars s and o: ONE rounding."""
    a = np.ascontiguousarray(a, F32)
    s, o = F32(s), F32(o)
    a64, s64, o64 = a.astype(np.float64), np.float64(s), np.float64(o)
    p = a64 * s64  # exact: 24 x 24 significant bits, far from the float64 range's ends
    assert np.isfinite(p).all() and (np.abs(p[p != 0]) > 1e-200).all()
    r = p + o64
    bb = r - p
    err = (p - (r - bb)) + (o64 - bb)  # TwoSum: p + o == r + err exactly
    out = r.astype(F32)  # r exact: rounded once
    for i in np.flatnonzero(err != 0):
        out[i] = _round32(Fraction(float(a[i])) * Fraction(float(s)) + Fraction(float(o)))
    return out


def _corner(a, k):
    nz, ny, nx = a.shape
    kx, ky, kz = k & 1, (k >> 1) & 1, (k >> 2) & 1
    return a[kz:nz - 1 + kz, ky:ny - 1 + ky, kx:nx - 1 + kx]


def edge_corners(e):
    """Edge e (0..11) -> (axis, corner a, corner b): 0-3 along x with (ky, kz) = (0,0) (1,0) (0,1) (1,1), 4-7 along
    y with (kx, kz), 8-11 along z with (kx, ky) in the same pattern."""
    axis, p, q = e >> 2, e & 1, (e >> 1) & 1
    k = [0, 0, 0]
    others = [i for i in range(3) if i != axis]
    k[others[0]], k[others[1]] = p, q
    a = k[0] + 2 * k[1] + 4 * k[2]
    return axis, a, a + (1 << axis), k


def mesh(density, origin, spacing):
    """The mesh of a density array (nz, ny, nx): a namespace of vertices (nv, 3) float32, cells (nv,) uint32,
    triangles (nt, 3) uint32, and per quad its axis (quad_axis) and whether its lower endpoint is inside
    (quad_inside)."""
    d = np.ascontiguousarray(density, F32)
    nz, ny, nx = d.shape
    empty = SimpleNamespace(vertices=np.zeros((0, 3), F32), cells=np.zeros(0, np.uint32),
                            triangles=np.zeros((0, 3), np.uint32), quad_axis=np.zeros(0, np.int64),
                            quad_inside=np.zeros(0, bool))
    if min(nx, ny, nz) < 2:
        return empty
    inside = d > 0
    n_in = sum(_corner(inside, k).astype(np.int32) for k in range(8))
    active = (n_in > 0) & (n_in < 8)
    cz, cy, cx = np.nonzero(active)  # C order: ascending cell index
    nv = len(cx)
    cells = ((cz * (ny - 1) + cy) * (nx - 1) + cx).astype(np.uint32)
    dd = [_corner(d, k)[active] for k in range(8)]
    sums = np.zeros((3, nv), F32)
    count = np.zeros(nv, np.int32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for e in range(12):
            axis, a, b, k = edge_corners(e)
            cross = (dd[a] > 0) != (dd[b] > 0)
            t = dd[a] / (dd[a] - dd[b])
            assert t.dtype == F32
            for ax in range(3):
                loc = t if ax == axis else np.full(nv, k[ax], F32)
                sums[ax] = np.where(cross, sums[ax] + loc, sums[ax])
            count += cross
        assert sums.dtype == F32 and (count >= 3).all()
        local = sums / count.astype(F32)[None, :]
    assert local.dtype == F32
    vertices = np.empty((nv, 3), F32)
    for ax, c in enumerate((cx, cy, cz)):
        lattice_coord = c.astype(F32) + local[ax]  # one float32 rounding
        assert lattice_coord.dtype == F32
        vertices[:, ax] = fma32(lattice_coord, spacing[ax], origin[ax])
    # faces: the edge from a cell's corner 0 along each axis, interior where the other two coordinates are >= 1
    vid = np.full(active.shape, -1, np.int64)
    vid[active] = np.arange(nv)
    in0 = _corner(inside, 0)
    gz, gy, gx = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    coord = (gx, gy, gz)
    quads = np.zeros(active.shape + (3,), bool)
    for ax in range(3):
        u, v = (ax + 1) % 3, (ax + 2) % 3
        quads[..., ax] = (in0 != _corner(inside, 1 << ax)) & (coord[u] >= 1) & (coord[v] >= 1)
    qz, qy, qx, qa = np.nonzero(quads)  # ascending owning cell, then axis
    c = np.stack([qx, qy, qz], axis=1)
    eu, ev = np.zeros_like(c), np.zeros_like(c)
    eu[np.arange(len(qa)), (qa + 1) % 3] = 1
    ev[np.arange(len(qa)), (qa + 2) % 3] = 1

    def ids(p):
        return vid[p[:, 2], p[:, 1], p[:, 0]]

    A, B, C, D = ids(c - eu - ev), ids(c - ev), ids(c), ids(c - eu)
    assert all((x >= 0).all() for x in (A, B, C, D))  # the four cells around a crossing edge are active
    q_in = in0[qz, qy, qx]
    second, fourth = np.where(q_in, B, D), np.where(q_in, D, B)
    tris = np.stack([np.stack([A, second, C], axis=1), np.stack([A, C, fourth], axis=1)], axis=1).reshape(-1, 3)
    return SimpleNamespace(vertices=vertices, cells=cells, triangles=tris.astype(np.uint32), quad_axis=qa,
                           quad_inside=q_in)


def normals(key, positions, eye, landscape):
    """float4(getNormal(float4(p, d)), d) with d = getDensity(p) at the vertex positions: (nv, 4) float32; cached
    under key."""
    p = np.ascontiguousarray(positions, F32).reshape(-1, 3)
    if len(p) == 0:
        return np.zeros((0, 4), F32)
    return FR.cached(("mesh", key), p, eye, landscape, normals=True)


def lattice_mesh(key, origin, spacing, dims, eye, landscape):
    """The mesh of a lattice of the landscape's density (the oracle's, through field_ref.lattice); cached."""
    k = (key, landscape)
    if k not in _cache:
        _, d = FR.lattice(("mesh-density", key), origin, spacing, dims, eye, landscape)
        m = mesh(d, [F32(x) for x in origin], [F32(x) for x in spacing])
        for a in vars(m).values():
            a.setflags(write=False)
        _cache[k] = m
    return _cache[k]


def triangle_normals(vertices, triangles):
    """Unnormalised geometric normals (b - a) x (c - a), float64."""
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles, np.int64)
    return np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
