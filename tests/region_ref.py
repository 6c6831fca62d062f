"""The checker of the region fields (TEST INFRASTRUCTURE): the definition in include/frosttrace.h as a plain flood
fill with a stack, started at every member in raster order that no earlier fill reached, over numpy booleans.  The
label of a region is the index its fill started from, which is the region's smallest index because the starts come in
raster order.  It knows no tiles, no forest and no atomics, so it shares nothing with the device's union-find but the
definition.  Occupancy comes in as words in rt_terrain_sample_lattice's layout; the members are path_ref.passable
for the free state and dist_ref.unpack for the solid one."""
import numpy as np

import dist_ref as DR
import path_ref as PR

NONE = 0xFFFFFFFF


def moves(connectivity=26):
    """The links of a connectivity: (dx, dy, dz) of the 26 moves, or of the 6 face moves."""
    assert connectivity in (6, 26), connectivity
    return [(dx, dy, dz) for dx, dy, dz, w in PR.MOVES if w == 3 or (w and connectivity == 26)]


def members(words, dims, clearance=0, solid=False):
    """(nz, ny, nx) bool: the points that are labelled."""
    if solid:
        assert not clearance, "the solid state takes no clearance"
        return DR.unpack(words, dims)
    return PR.passable(words, dims, clearance)


def label(member, connectivity=26):
    """(labels, sizes, (regions, members, largest)) of an (nz, ny, nx) bool member array."""
    nz, ny, nx = member.shape
    ok = member.reshape(-1).tolist()
    lab = [NONE] * member.size
    size = [0] * member.size
    steps = moves(connectivity)
    counts = []
    for start in range(member.size):
        if not ok[start] or lab[start] != NONE:
            continue
        lab[start] = start
        got, stack = [start], [start]
        while stack:
            p = stack.pop()
            x, r = p % nx, p // nx
            y, z = r % ny, r // ny
            for dx, dy, dz in steps:
                u, v, t = x + dx, y + dy, z + dz
                if not (0 <= u < nx and 0 <= v < ny and 0 <= t < nz):
                    continue
                q = (t * ny + v) * nx + u
                if ok[q] and lab[q] == NONE:
                    lab[q] = start
                    got.append(q)
                    stack.append(q)
        for p in got:
            size[p] = len(got)
        counts.append(len(got))
    labels = np.array(lab, np.uint64).astype(np.uint32).reshape(member.shape)
    sizes = np.array(size, np.uint64).astype(np.uint32).reshape(member.shape)
    return labels, sizes, (len(counts), int(sum(counts)), max(counts) if counts else 0)


def field(words, dims, clearance=0, connectivity=26, solid=False):
    """(labels, sizes, status[1:4]) of the definition."""
    return label(members(words, dims, clearance, solid), connectivity)
