#!/usr/bin/env python3
"""Measurements of the region field on the GPU: profiles/r21/region_field.{md,jsonl}.

The README's lattice: 256 x 64 x 256 nomadplains points of spacing 2 from (-256, 0, -256), the eye (0, 100, 0)
(4,194,304 points), the terrain's own occupancy.  For scale, measured in the same run: rt_terrain_path_field_device
from one seed at the free point nearest the lattice's centre (which marks that seed's region alone) and
rt_terrain_distance_field_device.

    python3 scripts/region_field_bench.py run OUT_DIR
        HIP events on the device's stream (ray_query_bench.py's method: back-to-back launches of >= 50 ms a window,
        warm-up first, 5 alternating repeats per pair): the free regions at 26 and at 6, the free regions at
        clearance 2, the solid regions with sizes; labels alone (three launches) beside labels, sizes and status
        (four).  The device form's words are compared with the host form's, and the labels with scipy.ndimage.label
        on the downloaded members where scipy is installed.  Appends one JSON line to OUT_DIR/region_field.jsonl.
    python3 scripts/region_field_bench.py passes CONFIG
        10 calls of one configuration (free26, free6, clear2, solid) with sizes and status and nothing else, to run
        under `rocprofv3 --kernel-trace --stats --output-format csv -d OUT_DIR/kt_CONFIG -o run --`: per-kernel times.
    python3 scripts/region_field_bench.py report OUT_DIR [MD_DIR]
        MD_DIR/region_field.md (default OUT_DIR) from the line and the kernel statistics (no GPU)."""
import csv
import glob
import json
import os
import sys
import time

from distance_field_bench import DIMS, EYE, ORIGIN, SPACING, Distance
from path_field_bench import SWEEP_MARGIN, Path, centre_seed, passable

KERNELS = ("k_fieldlattice", "k_distrows", "k_distcolumns", "k_distfinish", "k_regionlocal", "k_regionmerge",
           "k_regionflatten", "k_regionfinish")
NONE = 0xFFFFFFFF
# name -> (clearance, connectivity, solid)
CONFIGS = {"free26": (0, 26, False), "free6": (0, 6, False), "clear2": (2, 26, False), "solid": (0, 26, True)}
TITLES = {"free26": "free, 26", "free6": "free, 6", "clear2": "free, 26, clearance 2", "solid": "solid, 26"}


class Region:
    """The device form; the terrain's own occupancy."""

    def __init__(self, torch, G, ter, config, counted):
        n = DIMS[0] * DIMS[1] * DIMS[2]
        self.G, self.ter = G, ter
        self.clearance, self.connectivity, self.solid = CONFIGS[config]
        self.bytes = G.engine.region_scratch_bytes(ORIGIN, SPACING, DIMS, self.clearance)
        self.scratch = torch.zeros(self.bytes, dtype=torch.uint8, device="cuda:0")
        self.label = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        self.size = torch.zeros(n, dtype=torch.int32, device="cuda:0") if counted else None
        self.status = torch.zeros(4, dtype=torch.int32, device="cuda:0") if counted else None
        torch.cuda.synchronize()

    def __call__(self):
        ok = self.ter.region_field_device(ORIGIN, SPACING, DIMS, self.scratch.data_ptr(), self.bytes, self.label.data_ptr(),
                                          self.size.data_ptr() if self.size is not None else 0,
                                          self.status.data_ptr() if self.status is not None else 0, eye=EYE,
                                          clearance=self.clearance, connectivity=self.connectivity, solid=self.solid)
        assert ok, self.G.lib().rt_last_error()


def scipy_labels(member, connectivity):
    """The definition by scipy.ndimage.label (it numbers regions by first raster occurrence), or None without scipy."""
    try:
        import numpy as np
        import scipy.ndimage as ndi
    except ImportError:
        return None
    numbered, count = ndi.label(member, structure=ndi.generate_binary_structure(3, 3 if connectivity == 26 else 1))
    flat = numbered.reshape(-1)
    first = np.full(count + 1, NONE, np.uint32)
    idx = np.flatnonzero(flat)
    first[flat[idx][::-1]] = idx[::-1].astype(np.uint32)
    return first[numbered]


def run(out_dir):
    import ray_query_bench as RQ  # (sets the paths)
    import numpy as np
    import torch
    import gpgpuraytrace_amd as G
    assert torch.cuda.is_available(), "the measurements need the GPU"
    dev, ter = RQ.terrain("nomadplains")
    stream = torch.cuda.ExternalStream(dev.stream(), device="cuda:0")
    row = {"dims": DIMS, "points": DIMS[0] * DIMS[1] * DIMS[2]}
    yard_dist = Distance(torch, G, ter, 0)
    # the path field from the centre seed, for scale: as path_field_bench.py runs it
    seed = centre_seed(passable(ter, 0))
    pstatus = []
    pcost = ter.path_field(ORIGIN, SPACING, DIMS, [seed], eye=EYE, status=pstatus)
    assert pstatus[0] == 1, pstatus
    yard_path = Path(torch, G, ter, seed, 0, False, pstatus[1] + SWEEP_MARGIN)
    row["path"] = {"seed": seed, "working_sweeps": int(pstatus[1]), "launches": int(pstatus[1] + SWEEP_MARGIN + 3),
                   "reached": int(pstatus[2])}
    same = True
    for config, (clearance, conn, solid) in CONFIGS.items():
        status = []
        t0 = time.perf_counter()
        lab, sz = ter.region_field(ORIGIN, SPACING, DIMS, eye=EYE, clearance=clearance, connectivity=conn, solid=solid,
                                   sizes=True, status=status)
        host_s = time.perf_counter() - t0
        assert status[0] == 1, status
        t0 = time.perf_counter()
        ref = scipy_labels(lab != NONE, conn)
        scipy_s = time.perf_counter() - t0
        if ref is not None:
            same = same and np.array_equal(ref, lab)
        roots = np.flatnonzero(lab.reshape(-1) == np.arange(lab.size, dtype=np.uint32))
        counts = np.sort(sz.reshape(-1)[roots])[::-1]
        row[config] = {"scratch_bytes": G.engine.region_scratch_bytes(ORIGIN, SPACING, DIMS, clearance), "regions": int(status[1]),
                       "members": int(status[2]), "largest": int(status[3]), "sizes_top": [int(v) for v in counts[:5]],
                       "below_50": int((counts < 50).sum()), "host_form_s": host_s,
                       "scipy_label_s": scipy_s if ref is not None else None}
        if config == "free26":  # the seed's region is what the path field reaches
            same = same and np.array_equal(pcost != NONE, lab == lab[seed[2], seed[1], seed[0]])
        for counted in (True, False):
            side = Region(torch, G, ter, config, counted)
            side()
            dev.synchronize()
            ta, tb = RQ.pair(stream, yard_path, side)
            tc, _ = RQ.pair(stream, yard_dist, side)
            dev.synchronize()
            same = same and np.array_equal(side.label.cpu().numpy().view(np.uint32), lab.reshape(-1))
            if counted:
                same = same and np.array_equal(side.size.cpu().numpy().view(np.uint32), sz.reshape(-1))
                same = same and [int(v) for v in side.status.cpu().numpy().view(np.uint32)] == status
            key = "%s_%s" % (config, "counted" if counted else "labels")
            row[key + "_ms"], row[key + "_path_ms"], row[key + "_distance_ms"] = RQ.summary(tb), RQ.summary(ta), RQ.summary(tc)
            print("%-16s %.4f ms (%.1f%%), path field %.4f, distance field %.4f" % (
                key, row[key + "_ms"]["ms"], 100 * row[key + "_ms"]["spread"], row[key + "_path_ms"]["ms"],
                row[key + "_distance_ms"]["ms"]), flush=True)
    row["same_bits"] = bool(same)
    assert same
    with open(os.path.join(out_dir, "region_field.jsonl"), "a") as f:
        f.write(json.dumps(row) + "\n")
    dev.destroy()


def passes(config):
    import ray_query_bench as RQ
    import torch
    import gpgpuraytrace_amd as G
    dev, ter = RQ.terrain("nomadplains")
    side = Region(torch, G, ter, config, True)
    for _ in range(10):
        side()
    dev.synchronize()
    dev.destroy()


def kernel_stats(out_dir, config):
    """name -> (calls, average ns) of the kernels from a rocprofv3 --stats run, or None."""
    files = glob.glob(os.path.join(out_dir, "kt_" + config, "**", "*kernel_stats.csv"), recursive=True)
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
    d = [json.loads(ln) for ln in open(os.path.join(out_dir, "region_field.jsonl")) if ln.strip()][-1]
    p = d["path"]
    L = ["# Region field: measurements (MI355X)", "",
         "`scripts/region_field_bench.py`: the README's %d x %d x %d nomadplains lattice of spacing 2 from (-256, 0, -256), "
         "eye (0, 100, 0): %d points, the terrain's own occupancy.  The device forms on the device's stream, HIP events "
         "around back-to-back launches of >= 50 ms a window, warm-up first, 5 alternating repeats per pair; ms are medians "
         "per call, the spread is (max - min) / median of a side's repeats.  The device form's label, size and status words "
         "were compared with the host form's in the run, the labels with scipy.ndimage.label on the downloaded members "
         "where scipy was installed, and the region of the path field's seed with the points that field reaches (all "
         "equal)." % (tuple(d["dims"]) + (d["points"],)), "",
         "| members, links | regions | member points | largest region | regions below 50 points | largest five | scratch MiB | "
         "host form, s | scipy.ndimage.label on the host, s |", "|---|---|---|---|---|---|---|---|---|"]
    for c in CONFIGS:
        q = d[c]
        L.append("| %s | %d | %d | %d | %d | %s | %.1f | %.3f | %s |" % (
            TITLES[c], q["regions"], q["members"], q["largest"], q["below_50"], ", ".join(str(v) for v in q["sizes_top"]),
            q["scratch_bytes"] / 2 ** 20, q["host_form_s"], "%.3f" % q["scipy_label_s"] if q["scipy_label_s"] is not None else "-"))
    L += ["", "For scale, measured beside each row: rt_terrain_path_field_device, the cost alone at clearance 0 from the seed "
          "(%d, %d, %d) (the free point nearest the centre; %d working sweeps, %d launches; it marks that seed's region "
          "alone, %d points) and rt_terrain_distance_field_device (max_cells 0, float field).  Every figure includes the "
          "occupancy pass over the terrain." % (p["seed"][0], p["seed"][1], p["seed"][2], p["working_sweeps"], p["launches"],
                                                p["reached"]), "",
          "| rt_terrain_region_field_device | outputs | ms | path field beside it, ms | distance field beside it, ms |",
          "|---|---|---|---|---|"]
    for c in CONFIGS:
        for tag, key in (("labels, sizes, status", "counted"), ("labels alone", "labels")):
            a, b, e = (d["%s_%s_%s" % (c, key, s)] for s in ("ms", "path_ms", "distance_ms"))
            L.append("| %s | %s | %.4f (%.1f%%) | %.4f (%.1f%%) | %.4f (%.1f%%) |" % (
                TITLES[c], tag, a["ms"], 100 * a["spread"], b["ms"], 100 * b["spread"], e["ms"], 100 * e["spread"]))
    stats = {c: kernel_stats(out_dir, c) for c in CONFIGS}
    if all(stats.values()):
        L += ["", "Per kernel, from `rocprofv3 --kernel-trace --stats` in runs of their own: 10 calls of the device form "
              "with sizes and status (launches in the run; average ms a launch):", "",
              "| kernel | " + " | ".join(TITLES[c] for c in CONFIGS) + " |", "|---|" + "---|" * len(CONFIGS)]
        for k in KERNELS:
            L.append("| %s | %s |" % (k, " | ".join(
                "%d; %.4f" % (stats[c][k][0], stats[c][k][1] * 1e-6) if k in stats[c] else "-" for c in CONFIGS)))
    else:
        L += ["", "Per-kernel times: not measured in this run."]
    L.append("")
    os.makedirs(md_dir, exist_ok=True)
    with open(os.path.join(md_dir, "region_field.md"), "w") as f:
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
