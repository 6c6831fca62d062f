#!/usr/bin/env python3
"""Measurements of the visibility field on the GPU: profiles/r18/visibility_field.{md,jsonl}.

The README's lattice: 256 x 64 x 256 nomadplains points of spacing 2 from (-256, 0, -256), the eye (0, 100, 0)
(4,194,304 points), the terrain's own occupancy.  The cases: one point observer at the free point nearest the
lattice's top centre ("lookout"); the sun at time of day 0.3 as one direction ("sun"); eight point observers at the
free points nearest a 4 x 2 grid of the top layer ("eight"); the sun with max_range 32 ("sun_r32").  The yardsticks
are rt_terrain_distance_field_device and rt_terrain_sample_lattice_device with occupancy only, existing calls,
measured in the same run beside every case of rt_terrain_visibility_field_device.

    python3 scripts/visibility_field_bench.py run OUT_DIR
        HIP events on the device's stream (ray_query_bench.py's method: back-to-back launches of >= 50 ms a window,
        warm-up first, 5 alternating repeats per pair).  The device form's mask and status are compared with the host
        form's.  The checker's CPU time for the lookout on the 64 x 32 x 64 sub-lattice under it goes in for scale.
        Appends one JSON line to OUT_DIR/visibility_field.jsonl.
    python3 scripts/visibility_field_bench.py passes CASE
        10 calls of the device form and nothing else, to run under
        `rocprofv3 --kernel-trace --stats --output-format csv -d OUT_DIR/kt_<CASE> -o run --`: per-kernel times.
    python3 scripts/visibility_field_bench.py report OUT_DIR [MD_DIR]
        MD_DIR/visibility_field.md (default OUT_DIR) from the line and the kernel statistics (no GPU)."""
import csv
import glob
import json
import os
import sys
import time

from distance_field_bench import DIMS, EYE, ORIGIN, SPACING, Distance, Occupancy

KERNELS = ("k_fieldlattice", "k_visibility")
CASES = ("lookout", "sun", "eight", "sun_r32")
TIME_OF_DAY = 0.3


def free_points(ter):
    """(nz, ny, nx) bool: the lattice's free points (the signed distance is positive there)."""
    import numpy as np
    sd = ter.distance_field(ORIGIN, SPACING, DIMS, eye=EYE, max_cells=1)
    return np.asarray(sd > 0)


def nearest_free(free, target):
    """The free point nearest the lattice point target = (ix, iy, iz): (ix, iy, iz)."""
    import numpy as np
    at = np.argwhere(free)
    k = ((at - np.array(target[::-1])) ** 2).sum(axis=1).argmin()
    z, y, x = (int(v) for v in at[k])
    return x, y, z


def case_observers(G, free, case):
    """(point observers, directions, max_range) of a case."""
    nx, ny, nz = DIMS
    sun = G.engine.lattice_direction(G.camera.sun_direction(TIME_OF_DAY), SPACING)
    if case == "lookout":
        return [nearest_free(free, (nx // 2, ny - 1, nz // 2))], [], 0
    if case == "sun":
        return [], [sun], 0
    if case == "eight":
        return [nearest_free(free, (nx * fx // 8, ny - 1, nz * fz // 4)) for fz in (1, 3) for fx in (1, 3, 5, 7)], [], 0
    assert case == "sun_r32", case
    return [], [sun], 32


class Visibility:
    """The device form; the terrain's own occupancy."""

    def __init__(self, torch, G, ter, points, dirs, max_range):
        n = DIMS[0] * DIMS[1] * DIMS[2]
        self.G, self.ter, self.max_range = G, ter, max_range
        self.bytes = G.engine.visibility_scratch_bytes(ORIGIN, SPACING, DIMS)
        self.scratch = torch.zeros(self.bytes, dtype=torch.uint8, device="cuda:0")
        ob = G.engine.pack_observers(points or None, dirs or None, DIMS)
        self.count = int(ob.shape[0])
        self.observers = torch.from_numpy(ob).to("cuda:0")
        self.mask = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        self.status = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

    def __call__(self):
        ok = self.ter.visibility_field_device(ORIGIN, SPACING, DIMS, self.observers.data_ptr(), self.count,
                                              self.scratch.data_ptr(), self.bytes, self.mask.data_ptr(),
                                              self.status.data_ptr(), eye=EYE, max_range=self.max_range)
        assert ok, self.G.lib().rt_last_error()


def run(out_dir):
    import ray_query_bench as RQ  # (sets the paths)
    import numpy as np
    import torch
    import gpgpuraytrace_amd as G
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import dist_ref as DR
    import vis_ref as VR
    assert torch.cuda.is_available(), "the measurements need the GPU"
    dev, ter = RQ.terrain("nomadplains")
    stream = torch.cuda.ExternalStream(dev.stream(), device="cuda:0")
    free = free_points(ter)
    row = {"dims": DIMS, "points": DIMS[0] * DIMS[1] * DIMS[2], "free": float(free.mean()),
           "scratch_bytes": G.engine.visibility_scratch_bytes(ORIGIN, SPACING, DIMS)}
    yard_occ, yard_dist = Occupancy(torch, G, ter), Distance(torch, G, ter, 0)
    same = True
    for case in CASES:
        points, dirs, max_range = case_observers(G, free, case)
        status = []
        t0 = time.perf_counter()
        mask = ter.visibility_field(ORIGIN, SPACING, DIMS, observers=points or None, directions=dirs or None, eye=EYE,
                                    max_range=max_range, status=status)
        host_s = time.perf_counter() - t0
        assert mask is not None, G.lib().rt_last_error()
        side = Visibility(torch, G, ter, points, dirs, max_range)
        side()
        dev.synchronize()
        ta, tb = RQ.pair(stream, yard_dist, side)
        tc, _ = RQ.pair(stream, yard_occ, side)
        dev.synchronize()
        same = same and np.array_equal(side.mask.cpu().numpy().view(np.uint32), mask.reshape(-1))
        same = same and [int(v) for v in side.status.cpu().numpy().view(np.uint32)] == status
        per_bit = [float(((mask >> np.uint32(k)) & 1).mean()) for k in range(side.count)]
        row[case] = {"observers": points, "directions": dirs, "max_range": max_range, "status": status, "host_form_s": host_s,
                     "share_any": status[0] / row["points"], "share_per_observer": per_bit,
                     "share_of_free_per_observer": [float(((mask >> np.uint32(k)) & 1)[free].mean()) for k in range(side.count)],
                     "ms": RQ.summary(tb), "distance_ms": RQ.summary(ta), "occupancy_ms": RQ.summary(tc)}
        print("%-8s %.4f ms (%.1f%%), distance field %.4f, occupancy %.4f, seen or lit %.3f" % (
            case, row[case]["ms"]["ms"], 100 * row[case]["ms"]["spread"], row[case]["distance_ms"]["ms"],
            row[case]["occupancy_ms"]["ms"], row[case]["share_any"]), flush=True)
        if case == "lookout":  # the checker, for scale: the 64 x 32 x 64 sub-lattice under the lookout
            x, y, z = points[0]
            box = (slice(max(0, min(DIMS[2] - 64, z - 32)), None), slice(max(0, min(DIMS[1] - 32, y - 16)), None), slice(max(0, min(DIMS[0] - 64, x - 32)), None))
            box = tuple(slice(s.start, s.start + w) for s, w in zip(box, (64, 32, 64)))
            sub = ~free[box]
            local = (x - box[2].start, y - box[1].start, z - box[0].start)
            t0 = time.perf_counter()
            ref, _ = VR.field(DR.pack(sub, (64, 32, 64)), (64, 32, 64), VR.observers([local]))
            row["checker_sub_lattice_s"] = time.perf_counter() - t0
            row["checker_sub_lattice_seen"] = int(ref.sum())
    row["same_bits"] = bool(same)
    assert same
    with open(os.path.join(out_dir, "visibility_field.jsonl"), "a") as f:
        f.write(json.dumps(row) + "\n")
    dev.destroy()


def passes(case):
    import ray_query_bench as RQ
    import torch
    import gpgpuraytrace_amd as G
    dev, ter = RQ.terrain("nomadplains")
    points, dirs, max_range = case_observers(G, free_points(ter), case)
    side = Visibility(torch, G, ter, points, dirs, max_range)
    for _ in range(10):
        side()
    dev.synchronize()
    dev.destroy()


def kernel_stats(out_dir, case):
    """name -> (calls, average ns) of the kernels from a rocprofv3 --stats run, or None."""
    files = glob.glob(os.path.join(out_dir, "kt_%s" % case, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None
    found = {}
    for r in csv.DictReader(open(files[0])):
        for k in KERNELS:
            if k in r["Name"]:
                calls, total = found.get(k, (0, 0.0))
                found[k] = (calls + int(r["Calls"]), total + float(r["TotalDurationNs"]))
    return {k: (c, t / c) for k, (c, t) in found.items()}


def report(out_dir, md_dir):
    d = [json.loads(ln) for ln in open(os.path.join(out_dir, "visibility_field.jsonl")) if ln.strip()][-1]
    L = ["# Visibility field: measurements (MI355X)", "",
         "`scripts/visibility_field_bench.py`: the README's %d x %d x %d nomadplains lattice of spacing 2 from (-256, 0, -256), "
         "eye (0, 100, 0): %d points (%.1f%% free), the terrain's own occupancy; scratch %.2f MiB.  The device forms on the "
         "device's stream, HIP events around back-to-back launches of >= 50 ms a window, warm-up first, 5 alternating repeats "
         "per pair; ms are medians per call, the spread is (max - min) / median of a side's repeats.  The device form's mask "
         "words and status were compared with the host form's in the run (equal)." % (
             tuple(d["dims"]) + (d["points"], 100 * d["free"], d["scratch_bytes"] / 2 ** 20)), "",
         "The cases: `lookout`, one point observer at the free point nearest the lattice's top centre; `sun`, the direction "
         "`lattice_direction(sun_direction(0.3), spacing)`; `eight`, eight point observers at the free points nearest a 4 x 2 "
         "grid of the top layer; `sun_r32`, the sun with max_range 32.", "",
         "| case | observers | max_range | points with a bit set | share of all points | share of the free points, per observer | "
         "host form, s |", "|---|---|---|---|---|---|---|"]
    for case in CASES:
        q = d[case]
        who = ", ".join("(%d, %d, %d)" % tuple(p) for p in q["observers"]) or ", ".join("u = (%d, %d, %d)" % tuple(u) for u in q["directions"])
        L.append("| %s | %s | %d | %d | %.1f%% | %s | %.3f |" % (
            case, who, q["max_range"], q["status"][0], 100 * q["share_any"],
            ", ".join("%.1f%%" % (100 * s) for s in q["share_of_free_per_observer"]), q["host_form_s"]))
    L += ["", "The yardsticks, measured beside each row: rt_terrain_distance_field_device (the terrain's own occupancy, "
          "max_cells 0, float field) and rt_terrain_sample_lattice_device with occupancy only.", "",
          "| rt_terrain_visibility_field_device | ms | distance field beside it, ms | occupancy pass beside it, ms |",
          "|---|---|---|---|"]
    for case in CASES:
        a, b, c = d[case]["ms"], d[case]["distance_ms"], d[case]["occupancy_ms"]
        L.append("| %s | %.4f (%.1f%%) | %.4f (%.1f%%) | %.4f (%.1f%%) |" % (
            case, a["ms"], 100 * a["spread"], b["ms"], 100 * b["spread"], c["ms"], 100 * c["spread"]))
    L += ["", "For scale: the checker (tests/vis_ref.py, numpy) took %.2f s for the lookout on the 64 x 32 x 64 sub-lattice "
          "under it (%d points seen).  The cells walked per point were not counted: there is no debug build that counts "
          "them." % (d["checker_sub_lattice_s"], d["checker_sub_lattice_seen"])]
    stats = {c: kernel_stats(out_dir, c) for c in CASES}
    if all(stats.values()):
        L += ["", "Per kernel, from `rocprofv3 --kernel-trace --stats` in runs of their own: 10 calls of the device form "
              "after the distance field that finds the free points (launches in the run; average ms a launch):", "",
              "| kernel | " + " | ".join(CASES) + " |", "|---|" + "---|" * len(CASES)]
        for k in KERNELS:
            L.append("| %s | %s |" % (k, " | ".join(
                "%d; %.4f" % (stats[c][k][0], stats[c][k][1] * 1e-6) if stats[c].get(k, (0, 0))[0] >= 10 else "-" for c in CASES)))
    else:
        L += ["", "Per-kernel times: not measured in this run."]
    L.append("")
    os.makedirs(md_dir, exist_ok=True)
    with open(os.path.join(md_dir, "visibility_field.md"), "w") as f:
        f.write("\n".join(L))
    print("\n".join(L))


if __name__ == "__main__":
    what = sys.argv[1]
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if what == "run":
        os.makedirs(sys.argv[2], exist_ok=True)
        run(sys.argv[2])
    elif what == "passes":
        passes(sys.argv[2])
    else:
        report(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else sys.argv[2])
