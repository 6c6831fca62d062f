"""The checker of the path fields (TEST INFRASTRUCTURE): the definition in include/frosttrace.h as a heap Dijkstra
over the 26 moves with the 3-4-5 weights, in plain Python and numpy.  It knows no tiles, no sweeps and no flags, so
it shares nothing with the device's schedule but the definition.  Occupancy comes in as words in
rt_terrain_sample_lattice's layout; the passable set with a clearance comes from dist_ref.d2, the terrain's own
occupancy from field_ref's lattice helpers (dist_ref.terrain_words)."""
import heapq

import numpy as np

import dist_ref as DR

FAR = 0xFFFFFFFF
NONE = 255
STAY = 13
# code -> (dx, dy, dz, weight): c = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); 3 a face, 4 an edge, 5 a corner move
MOVES = []
for _dz in (-1, 0, 1):
    for _dy in (-1, 0, 1):
        for _dx in (-1, 0, 1):
            _k = abs(_dx) + abs(_dy) + abs(_dz)
            MOVES.append((_dx, _dy, _dz, (0, 3, 4, 5)[_k]))


def passable(words, dims, clearance=0):
    """(nz, ny, nx) bool: not blocked, and with a clearance R more than R cells from every blocked point (the
    distance field's d2 of an outside point above R * R, far included)."""
    blocked = DR.unpack(words, dims)
    free = ~blocked
    if clearance and blocked.size:
        d2 = DR.d2(words, dims).astype(np.int64)  # unbounded: the comparison below is the definition's
        free &= d2 > int(clearance) * int(clearance)
    return free


def cost(free, seeds, max_cost=0):
    """The definition's cost: (nz, ny, nx) uint32 from the passable set and flat seed indices."""
    nz, ny, nx = free.shape
    out = np.full(free.shape, FAR, np.uint32)
    if free.size == 0:
        return out
    ok = free.reshape(-1).tolist()
    best = [FAR] * free.size
    heap = []
    for s in np.asarray(seeds, np.int64).reshape(-1).tolist():
        if 0 <= s < free.size and ok[s] and best[s] != 0:
            best[s] = 0
            heap.append((0, s))
    heapq.heapify(heap)
    limit = int(max_cost) if max_cost else FAR - 1
    while heap:
        d, p = heapq.heappop(heap)
        if d != best[p]:
            continue
        x, r = p % nx, p // nx
        y, z = r % ny, r // ny
        for dx, dy, dz, w in MOVES:
            if not w:
                continue
            u, v, t = x + dx, y + dy, z + dz
            if not (0 <= u < nx and 0 <= v < ny and 0 <= t < nz):
                continue
            q = (t * ny + v) * nx + u
            nd = d + w
            if ok[q] and nd < best[q] and nd <= limit:
                best[q] = nd
                heapq.heappush(heap, (nd, q))
    return np.array(best, np.uint64).astype(np.uint32).reshape(free.shape)


def flow(c):
    """The definition's flow from a cost array alone: (nz, ny, nx) uint8."""
    c = np.asarray(c, np.uint32)
    nz, ny, nx = c.shape
    big = np.int64(1) << 40
    pad = np.full((nz + 2, ny + 2, nx + 2), big, np.int64)
    pad[1:-1, 1:-1, 1:-1] = np.where(c == FAR, big, c.astype(np.int64))
    out = np.full(c.shape, NONE, np.uint8)
    todo = (c != FAR) & (c != 0)
    out[c == 0] = STAY
    me = c.astype(np.int64)
    for code, (dx, dy, dz, w) in enumerate(MOVES):
        if code == STAY:
            continue
        q = pad[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
        hit = todo & (q + w == me)
        out[hit] = code
        todo &= ~hit
    return out


def field(words, dims, seeds, clearance=0, max_cost=0):
    """(cost, flow, reached) of the definition."""
    c = cost(passable(words, dims, clearance), seeds, max_cost)
    return c, flow(c), int((c != FAR).sum())


def index(dims, ix, iy, iz):
    return (int(iz) * int(dims[1]) + int(iy)) * int(dims[0]) + int(ix)


def serpentine(dims=(70, 9, 8)):
    """(nz, ny, nx) bool blocked: a wall across every x = 3 mod 4 with one gap at alternating corners."""
    nx, ny, nz = dims
    blocked = np.zeros((nz, ny, nx), bool)
    for k, x in enumerate(range(3, nx, 4)):
        blocked[:, :, x] = True
        if k % 2 == 0:
            blocked[0, 0, x] = False
        else:
            blocked[nz - 1, ny - 1, x] = False
    return blocked
