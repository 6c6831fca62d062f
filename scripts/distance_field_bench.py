#!/usr/bin/env python3
"""Measurements of the distance field on the GPU: profiles/r16/distance_field.{md,jsonl}.

The README's lattice: 256 x 64 x 256 nomadplains points of spacing 2 from (-256, 0, -256), the eye (0, 100, 0)
(4,194,304 points).  The yardstick is rt_terrain_sample_lattice_device with occupancy only (k_fieldlattice), an
existing call, measured in the same run beside every form of rt_terrain_distance_field_device.

    python3 scripts/distance_field_bench.py run OUT_DIR
        HIP events on the device's stream (ray_query_bench.py's method: back-to-back launches of >= 50 ms a window,
        warm-up first, 5 alternating repeats per pair): the occupancy pass against the distance field of the terrain's
        own occupancy (the occupancy pass and the three distance passes) and of a given occupancy (the three passes),
        each with max_cells 0 and 8; the device form's words compared with the host form's.  Appends one JSON line
        to OUT_DIR/distance_field.jsonl.
    python3 scripts/distance_field_bench.py passes MAX_CELLS
        40 calls of the terrain's own field and nothing else, to run under
        `rocprofv3 --kernel-trace --stats --output-format csv -d OUT_DIR/kt<MAX_CELLS> -o run --`: per-kernel times.
    python3 scripts/distance_field_bench.py report OUT_DIR [MD_DIR]
        MD_DIR/distance_field.md (default OUT_DIR) from the line and the kernel statistics (no GPU)."""
import csv
import glob
import json
import os
import sys

DIMS, ORIGIN, SPACING, EYE = (256, 64, 256), (-256.0, 0.0, -256.0), (2.0, 2.0, 2.0), (0.0, 100.0, 0.0)
KERNELS = ("k_fieldlattice", "k_distrows", "k_distcolumns", "k_distfinish")


class Occupancy:
    """The yardstick: the lattice's occupancy words alone into a device array."""

    def __init__(self, torch, G, ter):
        self.G, self.ter = G, ter
        self.occ = torch.zeros(DIMS[0] * DIMS[1] * DIMS[2] // 32, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

    def __call__(self):
        ok = self.ter.sample_lattice_device(ORIGIN, SPACING, DIMS, 0, self.occ.data_ptr(), eye=EYE)
        assert ok, self.G.lib().rt_last_error()


class Distance:
    """The device form into a float32 field; occ: a device array of occupancy words, or None for the terrain's own."""

    def __init__(self, torch, G, ter, max_cells, occ=None):
        self.G, self.ter, self.max_cells, self.occ = G, ter, max_cells, occ
        self.bytes = G.engine.distance_scratch_bytes(ORIGIN, SPACING, DIMS)
        self.scratch = torch.zeros(self.bytes, dtype=torch.uint8, device="cuda:0")
        self.dist = torch.zeros(DIMS[0] * DIMS[1] * DIMS[2], dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()

    def __call__(self):
        ok = self.ter.distance_field_device(ORIGIN, SPACING, DIMS, self.scratch.data_ptr(), self.bytes, 0,
                                            self.dist.data_ptr(), self.occ.data_ptr() if self.occ is not None else 0,
                                            eye=EYE, max_cells=self.max_cells)
        assert ok, self.G.lib().rt_last_error()


def run(out_dir):
    import ray_query_bench as RQ  # (sets the paths)
    import numpy as np
    import torch
    import gpgpuraytrace_amd as G
    assert torch.cuda.is_available(), "the measurements need the GPU"
    dev, ter = RQ.terrain("nomadplains")
    stream = torch.cuda.ExternalStream(dev.stream(), device="cuda:0")
    host = {mc: ter.distance_field(ORIGIN, SPACING, DIMS, eye=EYE, max_cells=mc) for mc in (0, 8)}
    assert host[0] is not None, G.lib().rt_last_error()
    d2 = ter.distance_field(ORIGIN, SPACING, DIMS, eye=EYE, squared=True)
    finite = d2[d2 != 0xFFFFFFFF]
    row = {"dims": DIMS, "points": int(d2.size), "scratch_bytes": G.engine.distance_scratch_bytes(ORIGIN, SPACING, DIMS),
           "inside": float((host[0] < 0).mean()), "largest_d2": int(finite.max()), "mean_abs_cells": float(np.sqrt(finite).mean()),
           "free_radius_3": float((host[0] >= 3.0).mean()), "beyond_8_cells": float(np.isinf(host[8]).mean())}
    yard = Occupancy(torch, G, ter)
    yard()
    dev.synchronize()
    same = True
    for mc in (0, 8):
        own, given = Distance(torch, G, ter, mc), Distance(torch, G, ter, mc, yard.occ)
        ta, tb = RQ.pair(stream, yard, own)
        tc, td = RQ.pair(stream, yard, given)
        dev.synchronize()
        for side in (own, given):
            same = same and np.array_equal(side.dist.cpu().numpy().view(np.uint32), host[mc].reshape(-1).view(np.uint32))
        row["occupancy_ms_%d" % mc], row["own_ms_%d" % mc] = RQ.summary(ta), RQ.summary(tb)
        row["occupancy_again_ms_%d" % mc], row["given_ms_%d" % mc] = RQ.summary(tc), RQ.summary(td)
        for k in ("occupancy_ms_%d" % mc, "own_ms_%d" % mc, "given_ms_%d" % mc):
            print("%-22s %.4f ms (%.1f%%)" % (k, row[k]["ms"], 100 * row[k]["spread"]), flush=True)
    row["same_bits"] = bool(same)
    assert same
    with open(os.path.join(out_dir, "distance_field.jsonl"), "a") as f:
        f.write(json.dumps(row) + "\n")
    dev.destroy()


def passes(max_cells):
    import ray_query_bench as RQ
    import torch
    import gpgpuraytrace_amd as G
    dev, ter = RQ.terrain("nomadplains")
    own = Distance(torch, G, ter, max_cells)
    for _ in range(40):
        own()
    dev.synchronize()
    dev.destroy()


def kernel_stats(out_dir, max_cells):
    """name -> (calls, average ns) of the four kernels from a rocprofv3 --stats run, or None."""
    files = glob.glob(os.path.join(out_dir, "kt%d" % max_cells, "**", "*kernel_stats.csv"), recursive=True)
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
    d = [json.loads(ln) for ln in open(os.path.join(out_dir, "distance_field.jsonl")) if ln.strip()][-1]
    L = ["# Distance field: measurements (MI355X)", "",
         "`scripts/distance_field_bench.py`: the README's %d x %d x %d nomadplains lattice of spacing 2 from (-256, 0, -256), "
         "eye (0, 100, 0): %d points, %.1f%% inside, largest finite d2 %d, mean |distance| %.2f cells, %.1f%% of the points "
         "free for an agent of radius 3, %.1f%% beyond 8 cells; scratch %.1f MiB.  The device forms on the device's "
         "stream, HIP events around back-to-back launches of >= 50 ms a window, warm-up first, 5 alternating repeats per "
         "pair; ms are medians per call, the spread is (max - min) / median of a side's repeats.  The device form's "
         "floats were compared bit for bit with the host form's in the run (equal)."
         % (tuple(d["dims"]) + (d["points"], 100 * d["inside"], d["largest_d2"], d["mean_abs_cells"],
                               100 * d["free_radius_3"], 100 * d["beyond_8_cells"], d["scratch_bytes"] / 2 ** 20)), "",
         "The yardstick is rt_terrain_sample_lattice_device with occupancy only (k_fieldlattice), measured beside each row.",
         "", "| call | max_cells | ms | yardstick beside it, ms | times the yardstick |", "|---|---|---|---|---|"]
    for mc in (0, 8):
        for tag, key, beside in (("rt_terrain_distance_field_device, the terrain's own occupancy (4 kernels)", "own_ms_%d", "occupancy_ms_%d"),
                                 ("the same with the occupancy given (3 kernels)", "given_ms_%d", "occupancy_again_ms_%d")):
            a, b = d[key % mc], d[beside % mc]
            L.append("| %s | %d | %.4f (%.1f%%) | %.4f (%.1f%%) | %.2f |" % (tag, mc, a["ms"], 100 * a["spread"], b["ms"],
                                                                          100 * b["spread"], a["ms"] / b["ms"]))
    stats = {mc: kernel_stats(out_dir, mc) for mc in (0, 8)}
    if all(stats.values()):
        L += ["", "Per kernel, from `rocprofv3 --kernel-trace --stats` over 40 calls of the terrain's own field in runs of "
              "their own (average ms a launch):", "", "| kernel | pass | max_cells 0 | max_cells 8 |", "|---|---|---|---|"]
        for k, what in zip(KERNELS, ("occupancy", "x: rows, from the occupancy words", "y: columns, both sets",
                                     "z: columns, the other set; max_cells, sqrt, store")):
            L.append("| %s | %s | %s |" % (k, what, " | ".join(
                "%.4f" % (stats[mc][k][1] * 1e-6) if k in stats[mc] else "-" for mc in (0, 8))))
    else:
        L += ["", "Per-kernel times: not measured in this run."]
    L.append("")
    os.makedirs(md_dir, exist_ok=True)
    with open(os.path.join(md_dir, "distance_field.md"), "w") as f:
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
