"""The checker of the distance fields (TEST INFRASTRUCTURE): the definition in include/frosttrace.h in numpy
integers.  The squared distance to a set is formed axis by axis as a min-plus product over WHOLE axes,
h(j) = min over k of f(k) + (j - k)^2 with every k of the axis in the minimum: no bit tricks and no pruned scan, so
it shares nothing with the device's passes but the separability of the squared Euclidean metric.  Occupancy comes
in as words in rt_terrain_sample_lattice's layout; the terrain's own comes from field_ref's lattice helpers."""
import numpy as np

import field_ref as FR

FAR = 0xFFFFFFFF
_BIG = np.int64(1) << 40  # above every finite sum (3 * 4095^2 < 2^26), and three of them stay far below 2^63


def unpack(words, dims):
    """(nz, ny, nx) bool from occupancy words (nz, ny, ceil(nx / 32)): bit ix % 32 of word ix // 32; the padding
    bits are dropped whatever they hold."""
    nx, ny, nz = (int(v) for v in dims)
    w = np.ascontiguousarray(words, np.uint32).reshape(nz, ny, (nx + 31) // 32)
    bits = np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little")
    return bits[..., :nx].astype(bool)


def pack(inside, dims, padding=0):
    """Occupancy words of an (nz, ny, nx) bool array; padding 1 sets every padding bit."""
    nx, ny, nz = (int(v) for v in dims)
    words = (nx + 31) // 32
    bits = np.full((nz, ny, words * 32), 1 if padding else 0, np.uint8)
    bits[..., :nx] = np.asarray(inside, bool).reshape(nz, ny, nx)
    return np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little")).view("<u4").reshape(nz, ny, words)


def _minplus(f, axis):
    """h(j) = min over all k of f(k) + (j - k)^2 along one axis, int64."""
    n = f.shape[axis]
    f = np.moveaxis(f, axis, -1)
    idx = np.arange(n, dtype=np.int64)
    cost = (idx[:, None] - idx[None, :]) ** 2  # [j, k]
    h = (f[..., None, :] + cost).min(axis=-1)
    return np.moveaxis(h, -1, axis)


def _to_set(member):
    """Squared distance of every point to the nearest member, int64; >= _BIG where there is none."""
    f = np.where(member, np.int64(0), _BIG)
    for axis in (2, 1, 0):
        f = _minplus(f, axis)
    return f


def d2(words, dims, max_cells=0):
    """The definition's d2: (nz, ny, nx) uint32."""
    inside = unpack(words, dims)
    if inside.size == 0:
        return np.zeros(inside.shape, np.uint32)
    far = np.where(inside, _to_set(~inside), _to_set(inside))
    out = np.where(far >= _BIG, np.int64(FAR), far)
    if max_cells:
        out = np.where(out > int(max_cells) * int(max_cells), np.int64(FAR), out)
    return out.astype(np.uint32)


def distance(words, dims, spacing, max_cells=0):
    """The definition's distance: (nz, ny, nx) float32, s * (sqrt((float)d2) * |spacing[0]|), +-inf for FAR."""
    s = np.abs(np.asarray(spacing, np.float32))
    assert s[0] == s[1] == s[2] != 0, spacing
    inside = unpack(words, dims)
    q = d2(words, dims, max_cells)
    with np.errstate(over="ignore"):
        d = (np.sqrt(q.astype(np.float32)) * s[0]).astype(np.float32)
    d[q == FAR] = np.float32(np.inf)
    return np.where(inside, -d, d).astype(np.float32)


def terrain_words(key, origin, spacing, dims, eye, landscape):
    """The terrain's own occupancy words on a lattice, from the checker of the field queries (cached under key)."""
    _, dens = FR.lattice(key, origin, spacing, dims, eye, landscape)
    return FR.occupancy_words(dens, dims)
