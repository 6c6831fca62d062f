"""The checker of the visibility fields (TEST INFRASTRUCTURE): the definition in include/frosttrace.h in numpy
int64, written from the header's words and not from the device's walker.  Every walk keeps its crossing counters
k_i and orders the next crossing times (2 k_i + 1) / (2 n_i) of the axes that still have one by cross-multiplying,
for all points at once; there are no running differences, no bit addresses and no reliance on how a finished axis
happens to compare.  A point observer's lines are walked from the points (they part at once, so the blocked ones end
early); the definition is symmetric, and tests/test_visibility_host.py pins the walk from both ends by a second
statement of the definition (an exact interval test per candidate cell with fractions.Fraction)."""
import numpy as np

import dist_ref as DR

POINT, DIRECTION = 0, 1
MAX_DIRECTION = 4095
MAX_OBSERVERS = 32


def observer_valid(o, dims):
    x, y, z, kind = (int(v) for v in o)
    nx, ny, nz = (int(v) for v in dims)
    if kind == POINT:
        return 0 <= x < nx and 0 <= y < ny and 0 <= z < nz
    if kind == DIRECTION:
        return max(abs(x), abs(y), abs(z)) <= MAX_DIRECTION and (x, y, z) != (0, 0, 0)
    return False


def _walk(start, delta, finite, dims, visit):
    """The walk of the definition for N lines at once.  start (N, 3) int64 lattice points, delta (N, 3) int64: axis i
    crosses at t = (2 k + 1) / (2 |delta_i|), k = 0 .. |delta_i| - 1 when finite, k = 0, 1, ... otherwise.  After
    every event visit(ids, pos, last) is called with the lines still walking (ids into the N), their positions and,
    for finite walks, whether the event was a line's last (its position is start + delta then); it returns the lines
    that go on.  A line whose position is no point of the lattice is dropped before the call when the walk is not
    finite, and reported through visit(ids, None, None) -- 'left the lattice'."""
    ids = np.arange(start.shape[0])
    n = np.abs(delta)
    s = np.sign(delta)
    k = np.zeros_like(n)
    pos = start.copy()
    lim = np.array([int(v) for v in dims], np.int64)
    moving = n.sum(axis=1) > 0
    ids, n, s, k, pos = ids[moving], n[moving], s[moving], k[moving], pos[moving]
    while ids.size:
        has = (k < n) if finite else (n > 0)
        num = 2 * k + 1
        cross = num[:, :, None] * n[:, None, :]  # [line, i, j] = (2 k_i + 1) n_j
        later = cross > cross.transpose(0, 2, 1)  # t_i > t_j (both n > 0 where it counts)
        # axis i crosses at the earliest time: it has a crossing, and t_i <= t_j for every axis j that has one
        first = has & ~(has[:, None, :] & later).any(axis=2)
        k = k + first
        pos = pos + s * first
        if finite:
            last = (k == n).all(axis=1)
        else:
            out = ((pos < 0) | (pos >= lim)).any(axis=1)
            if out.any():
                visit(ids[out], None, None)
                keep = ~out
                ids, n, s, k, pos = ids[keep], n[keep], s[keep], k[keep], pos[keep]
            if not ids.size:
                break
            last = np.zeros(ids.size, bool)
        go = visit(ids, pos, last)
        if not go.all():
            ids, n, s, k, pos = ids[go], n[go], s[go], k[go], pos[go]


def cells_between(o, p):
    """The cells between the lattice points o and p, in the walk's order from o (a list of (x, y, z))."""
    cells = []

    def visit(ids, pos, last):
        if not last[0]:
            cells.append(tuple(int(v) for v in pos[0]))
        return ~last

    _walk(np.array([o], np.int64), np.array([p], np.int64) - np.array([o], np.int64), True, (1, 1, 1), visit)
    return cells


def direction_cells(p, u, dims):
    """The cells a directional walk from p along u visits before it leaves the lattice, in order."""
    cells = []

    def visit(ids, pos, last):
        if pos is None:
            return None
        cells.append(tuple(int(v) for v in pos[0]))
        return np.ones(ids.size, bool)

    _walk(np.array([p], np.int64), np.array([u], np.int64), False, dims, visit)
    return cells


def _points(dims):
    nx, ny, nz = (int(v) for v in dims)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1).astype(np.int64)


def sees(blocked, dims, observer, max_range=0):
    """(nz, ny, nx) bool: the points that see one valid observer (x, y, z, kind).  blocked: (nz, ny, nx) bool."""
    nx, ny, nz = (int(v) for v in dims)
    pts = _points(dims)
    r2 = int(max_range) ** 2
    res = np.ones(pts.shape[0], bool)
    ob = np.array([int(v) for v in observer[:3]], np.int64)
    if int(observer[3]) == POINT:
        delta = ob - pts  # from the point to the observer
        near = np.ones(pts.shape[0], bool)
        if r2:
            near = (delta ** 2).sum(axis=1) <= r2
            res &= near
        sel = np.flatnonzero(near)

        def visit(ids, pos, last):
            hit = ~last & blocked[pos[:, 2], pos[:, 1], pos[:, 0]]  # the last position is the observer: not tested
            res[sel[ids[hit]]] = False
            return ~last & ~hit

        _walk(pts[sel], delta[sel], True, dims, visit)
    else:
        def visit(ids, pos, last):
            if pos is None:
                return None  # left the lattice unblocked: lit
            go = np.ones(ids.size, bool)
            if r2:
                go &= ((pos - pts[ids]) ** 2).sum(axis=1) <= r2  # beyond the range: the walk ends, lit
            hit = go & blocked[pos[:, 2], pos[:, 1], pos[:, 0]]
            res[ids[hit]] = False
            return go & ~hit

        _walk(pts, np.broadcast_to(ob, pts.shape).copy(), False, dims, visit)
    return res.reshape(nz, ny, nx)


def field(words, dims, observers, max_range=0):
    """The definition's result: (mask (nz, ny, nx) uint32, status [4]) for occupancy words in
    rt_terrain_sample_lattice's layout and (n, 4) observer records; an invalid record sees nothing."""
    nx, ny, nz = (int(v) for v in dims)
    blocked = DR.unpack(words, dims)
    obs = np.asarray(observers, np.int64).reshape(-1, 4)
    assert 1 <= obs.shape[0] <= MAX_OBSERVERS
    mask = np.zeros((nz, ny, nx), np.uint32)
    valid = 0
    for b, o in enumerate(obs):
        if not observer_valid(o, dims):
            continue
        valid += 1
        if mask.size:
            mask |= sees(blocked, dims, o, max_range).astype(np.uint32) << np.uint32(b)
    bits = int(np.unpackbits(mask.view(np.uint8)).sum())
    return mask, [int((mask != 0).sum()), bits, valid, 0]


def observers(points=(), directions=()):
    """(n, 4) int32 records: the point observers first, then the directions."""
    rows = [(int(x), int(y), int(z), POINT) for x, y, z in points] + [(int(x), int(y), int(z), DIRECTION) for x, y, z in directions]
    return np.array(rows, np.int32).reshape(-1, 4)
