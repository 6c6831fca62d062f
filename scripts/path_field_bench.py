#!/usr/bin/env python3
"""Measurements of the path field on the GPU: profiles/r17/path_field.{md,jsonl}.

The README's lattice: 256 x 64 x 256 nomadplains points of spacing 2 from (-256, 0, -256), the eye (0, 100, 0)
(4,194,304 points), one seed at the free point nearest the lattice's centre.  The yardsticks are
rt_terrain_distance_field_device and rt_terrain_sample_lattice_device with occupancy only, existing calls, measured
in the same run beside every form of rt_terrain_path_field_device.

    python3 scripts/path_field_bench.py run OUT_DIR
        HIP events on the device's stream (ray_query_bench.py's method: back-to-back launches of >= 50 ms a window,
        warm-up first, 5 alternating repeats per pair): clearance 0 and 2, with and without the flow; the device form
        runs the host form's working sweeps + 8 (a margin: the count varies a little with the schedule).  The device
        form's words are compared with the host form's.  The checker's CPU time on the 64 x 32 x 64 sub-lattice round
        the seed goes in for scale.  Appends one JSON line to OUT_DIR/path_field.jsonl.
    python3 scripts/path_field_bench.py passes CLEARANCE
        10 calls of the terrain's own field with the flow and nothing else, to run under
        `rocprofv3 --kernel-trace --stats --output-format csv -d OUT_DIR/kt<CLEARANCE> -o run --`: per-kernel times.
    python3 scripts/path_field_bench.py report OUT_DIR [MD_DIR]
        MD_DIR/path_field.md (default OUT_DIR) from the line and the kernel statistics (no GPU)."""
import csv
import glob
import json
import os
import sys
import time

from distance_field_bench import DIMS, EYE, ORIGIN, SPACING, Distance, Occupancy

KERNELS = ("k_fieldlattice", "k_distrows", "k_distcolumns", "k_distfinish", "k_pathinit", "k_pathseed", "k_pathsweep",
           "k_pathfinish")
FAR = 0xFFFFFFFF
# the device form's sweeps beyond the host form's working ones: how many sweeps a field takes depends on which halo
# reads met a neighbour's store, so it varies a little from call to call; the run checks that the field converged
SWEEP_MARGIN = 8
CNT_VISITS = 6  # rtq::PATH_CNT_VISITS of the 16 counter words that end the scratch block


def passable(ter, clearance):
    """(nz, ny, nx) bool from the distance field: in free space and, with a clearance, beyond it (the signed distance
    at max_cells = clearance is +inf exactly there)."""
    import numpy as np
    sd = ter.distance_field(ORIGIN, SPACING, DIMS, eye=EYE, max_cells=max(clearance, 1))
    return np.isposinf(sd) if clearance else sd > 0


def centre_seed(ok):
    """The passable point nearest the lattice's centre: (ix, iy, iz)."""
    import numpy as np
    nz, ny, nx = ok.shape
    at = np.argwhere(ok)
    k = ((at - np.array([nz // 2, ny // 2, nx // 2])) ** 2).sum(axis=1).argmin()
    z, y, x = (int(v) for v in at[k])
    return x, y, z


class Path:
    """The device form; the terrain's own occupancy."""

    def __init__(self, torch, G, ter, seed, clearance, flow, sweeps):
        n = DIMS[0] * DIMS[1] * DIMS[2]
        self.G, self.ter, self.clearance, self.sweeps = G, ter, clearance, sweeps
        self.bytes = G.engine.path_scratch_bytes(ORIGIN, SPACING, DIMS, clearance)
        self.scratch = torch.zeros(self.bytes, dtype=torch.uint8, device="cuda:0")
        self.seeds = torch.tensor([(seed[2] * DIMS[1] + seed[1]) * DIMS[0] + seed[0]], dtype=torch.int32, device="cuda:0")
        self.cost = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        self.flow = torch.zeros(n, dtype=torch.uint8, device="cuda:0") if flow else None
        self.status = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

    def __call__(self):
        ok = self.ter.path_field_device(ORIGIN, SPACING, DIMS, self.seeds.data_ptr(), 1, self.scratch.data_ptr(), self.bytes,
                                        self.cost.data_ptr(), self.status.data_ptr(),
                                        flow_ptr=self.flow.data_ptr() if self.flow is not None else 0, eye=EYE,
                                        clearance=self.clearance, max_sweeps=self.sweeps)
        assert ok, self.G.lib().rt_last_error()

    def visits(self):
        return int(self.scratch[-64:].cpu().numpy().view("<u4")[CNT_VISITS])


def sub_lattice(ok, seed):
    """The 64 x 32 x 64 box of the lattice round the seed, clipped to the lattice: slices (z, y, x)."""
    out = []
    for c, n, want in ((seed[2], ok.shape[0], 64), (seed[1], ok.shape[1], 32), (seed[0], ok.shape[2], 64)):
        lo = max(0, min(n - want, c - want // 2))
        out.append(slice(lo, lo + want))
    return tuple(out)


def run(out_dir):
    import ray_query_bench as RQ  # (sets the paths)
    import numpy as np
    import torch
    import gpgpuraytrace_amd as G
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import path_ref as PR
    assert torch.cuda.is_available(), "the measurements need the GPU"
    dev, ter = RQ.terrain("nomadplains")
    stream = torch.cuda.ExternalStream(dev.stream(), device="cuda:0")
    row = {"dims": DIMS, "points": DIMS[0] * DIMS[1] * DIMS[2]}
    yard_occ, yard_dist = Occupancy(torch, G, ter), Distance(torch, G, ter, 0)
    same = True
    for r in (0, 2):
        ok = passable(ter, r)
        seed = centre_seed(ok)
        status = []
        t0 = time.perf_counter()
        cost, flow = ter.path_field(ORIGIN, SPACING, DIMS, [seed], eye=EYE, clearance=r, flow=True, status=status)
        host_s = time.perf_counter() - t0
        assert status[0] == 1, status
        sweeps = status[1] + SWEEP_MARGIN
        finite = cost[cost != FAR]
        route = G.engine.follow_flow(flow, tuple(int(v) for v in np.argwhere(cost == finite.max())[0][::-1]))
        row["r%d" % r] = {"seed": seed, "scratch_bytes": G.engine.path_scratch_bytes(ORIGIN, SPACING, DIMS, r),
                          "working_sweeps": int(status[1]), "device_sweeps": int(sweeps), "reached": int(status[2]),
                          "largest_cost": int(finite.max()), "longest_route_points": int(len(route)),
                          "longest_route_world": float(finite.max()) * SPACING[0] / 3.0, "host_form_s": host_s}
        for with_flow in (True, False):
            side = Path(torch, G, ter, seed, r, with_flow, sweeps)
            side()
            dev.synchronize()
            row["r%d" % r]["tile_visits"] = side.visits()
            ta, tb = RQ.pair(stream, yard_dist, side)
            tc, _ = RQ.pair(stream, yard_occ, side)
            dev.synchronize()
            same = same and np.array_equal(side.cost.cpu().numpy().view(np.uint32), cost.reshape(-1))
            st = [int(v) for v in side.status.cpu().numpy().view(np.uint32)]
            same = same and [st[0], st[2], st[3]] == [1, status[2], 0]  # (the working sweeps depend on the schedule)
            if with_flow:
                same = same and np.array_equal(side.flow.cpu().numpy(), flow.reshape(-1))
            key = "r%d_%s" % (r, "flow" if with_flow else "cost")
            row[key + "_ms"], row[key + "_distance_ms"], row[key + "_occupancy_ms"] = RQ.summary(tb), RQ.summary(ta), RQ.summary(tc)
            print("%-12s %.4f ms (%.1f%%), distance field %.4f, occupancy %.4f" % (
                key, row[key + "_ms"]["ms"], 100 * row[key + "_ms"]["spread"], row[key + "_distance_ms"]["ms"],
                row[key + "_occupancy_ms"]["ms"]), flush=True)
        if r == 0:  # the checker, for scale: a heap Dijkstra on the CPU over the sub-lattice round the seed
            box = sub_lattice(ok, seed)
            free = ok[box]
            local = ((seed[2] - box[0].start) * free.shape[1] + seed[1] - box[1].start) * free.shape[2] + seed[0] - box[2].start
            t0 = time.perf_counter()
            ref = PR.cost(free, [local])
            row["checker_sub_lattice_s"] = time.perf_counter() - t0
            row["checker_sub_lattice_reached"] = int((ref != FAR).sum())
    row["same_bits"] = bool(same)
    assert same
    with open(os.path.join(out_dir, "path_field.jsonl"), "a") as f:
        f.write(json.dumps(row) + "\n")
    dev.destroy()


def passes(clearance):
    import ray_query_bench as RQ
    import torch
    import gpgpuraytrace_amd as G
    dev, ter = RQ.terrain("nomadplains")
    seed = centre_seed(passable(ter, clearance))
    status = []
    ter.path_field(ORIGIN, SPACING, DIMS, [seed], eye=EYE, clearance=clearance, status=status)
    side = Path(torch, G, ter, seed, clearance, True, status[1] + SWEEP_MARGIN)
    for _ in range(10):
        side()
    dev.synchronize()
    dev.destroy()


def kernel_stats(out_dir, clearance):
    """name -> (calls, average ns) of the kernels from a rocprofv3 --stats run, or None."""
    files = glob.glob(os.path.join(out_dir, "kt%d" % clearance, "**", "*kernel_stats.csv"), recursive=True)
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
    d = [json.loads(ln) for ln in open(os.path.join(out_dir, "path_field.jsonl")) if ln.strip()][-1]
    L = ["# Path field: measurements (MI355X)", "",
         "`scripts/path_field_bench.py`: the README's %d x %d x %d nomadplains lattice of spacing 2 from (-256, 0, -256), "
         "eye (0, 100, 0): %d points, the terrain's own occupancy, one seed at the passable point nearest the lattice's "
         "centre.  The device forms on the device's stream, HIP events around back-to-back launches of >= 50 ms a window, "
         "warm-up first, 5 alternating repeats per pair; ms are medians per call, the spread is (max - min) / median of a "
         "side's repeats.  The device form runs the host form's working sweeps + 8; its cost words, flow bytes and status "
         "were compared with the host form's in the run (equal)." % (tuple(d["dims"]) + (d["points"],)), "",
         "| clearance | seed | working sweeps | sweep launches | active tile visits | reached points | largest cost | "
         "longest route, world units | scratch MiB | host form, s |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in (0, 2):
        q = d["r%d" % r]
        L.append("| %d | (%d, %d, %d) | %d | %d | %d | %d | %d | %.1f | %.1f | %.3f |" % (
            r, q["seed"][0], q["seed"][1], q["seed"][2], q["working_sweeps"], q["device_sweeps"], q["tile_visits"], q["reached"],
            q["largest_cost"], q["longest_route_world"], q["scratch_bytes"] / 2 ** 20, q["host_form_s"]))
    L += ["", "The yardsticks, measured beside each row: rt_terrain_distance_field_device (the terrain's own occupancy, "
          "max_cells 0, float field) and rt_terrain_sample_lattice_device with occupancy only.", "",
          "| rt_terrain_path_field_device | clearance | ms | distance field beside it, ms | occupancy pass beside it, ms |",
          "|---|---|---|---|---|"]
    for r in (0, 2):
        for tag, key in (("cost and flow", "r%d_flow"), ("cost alone", "r%d_cost")):
            a, b, c = d[key % r + "_ms"], d[key % r + "_distance_ms"], d[key % r + "_occupancy_ms"]
            L.append("| %s | %d | %.4f (%.1f%%) | %.4f (%.1f%%) | %.4f (%.1f%%) |" % (
                tag, r, a["ms"], 100 * a["spread"], b["ms"], 100 * b["spread"], c["ms"], 100 * c["spread"]))
    L += ["", "For scale: the checker (tests/path_ref.py, a heap Dijkstra in Python) took %.2f s on the 64 x 32 x 64 "
          "sub-lattice round the seed (%d points reached)." % (d["checker_sub_lattice_s"], d["checker_sub_lattice_reached"])]
    stats = {r: kernel_stats(out_dir, r) for r in (0, 2)}
    if all(stats.values()):
        L += ["", "Per kernel, from `rocprofv3 --kernel-trace --stats` in runs of their own: 10 calls of the device form with "
              "the flow, after the distance field that chooses the seed and the one host-form call that gives the sweep "
              "count (launches in the run; average ms a launch; a kernel with fewer than 10 launches ran for those two "
              "only):", "", "| kernel | clearance 0 | clearance 2 |", "|---|---|---|"]
        for k in KERNELS:
            L.append("| %s | %s |" % (k, " | ".join(
                "%d; %.4f" % (stats[r][k][0], stats[r][k][1] * 1e-6) if stats[r].get(k, (0, 0))[0] >= 10 else "-" for r in (0, 2))))
    else:
        L += ["", "Per-kernel times: not measured in this run."]
    L.append("")
    os.makedirs(md_dir, exist_ok=True)
    with open(os.path.join(md_dir, "path_field.md"), "w") as f:
        f.write("\n".join(L))
    print("\n".join(L))


if __name__ == "__main__":
    what = sys.argv[1]
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if what == "run":
        os.makedirs(sys.argv[2], exist_ok=True)
        run(sys.argv[2])
    elif what == "passes":
        passes(int(sys.argv[2]))
    else:
        report(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else sys.argv[2])
