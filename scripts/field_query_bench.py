#!/usr/bin/env python3
"""Measurements of the field queries on the GPU: profiles/r12/field_query.{md,jsonl} (driver: field_query_bench.sh).

A 256 x 128 x 256 nomadplains lattice of spacing 1 around the reset pose's eye (0, 100, 0), x and z from -128 to
127, y from 0 to 127 (8,388,608 points), the eye that one, three ways:
    (a) rt_debug_noise(density = 1) over the same points uploaded: the only route to the field before.  Its kernel
        time comes from the kernel trace (`trace` below); `run` also brackets the whole call (upload, kernel,
        download) with HIP events;
    (b) k_fieldpoints: rt_terrain_sample_field_device over the same points packed on the device;
    (c) k_fieldlattice: rt_terrain_sample_lattice_device, no coordinates.

    [RT_LIB_VARIANT=NAME] python3 scripts/field_query_bench.py run OUT_DIR
        (b) against (c) with HIP events (ray_query_bench.py's method: back-to-back launches of >= 50 ms a window,
        warm-up first, 5 alternating repeats), the results compared bit for bit; the default build also times (c)
        with occupancy and both with normals, and (a)'s whole call.  NAME is a build of `make variant` with
        -DRT_FIELD_ROWS=n (the strip's rows) or -DRT_FIELD_COLUMN=0 (no column reuse).  Appends one JSON line to
        OUT_DIR/field_query.jsonl.
    rocprofv3 --kernel-trace --stats ... -- python3 scripts/field_query_bench.py trace
        (a), (b) and (c) three times each in one process, for the trace's per-kernel times.
    python3 scripts/field_query_bench.py report OUT_DIR [--resources FILE] [--stats kernel_stats.csv]
        OUT_DIR/field_query.md from the lines (no GPU)."""
import csv
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
DIMS, ORIGIN, SPACING, EYE = (256, 128, 256), (-128.0, 0.0, -128.0), (1.0, 1.0, 1.0), (0.0, 100.0, 0.0)
ROWS_DEFAULT = 8  # rt_rayquery.h kFieldRows


def setup():
    import ray_query_bench as RQ  # (applies RT_LIB_VARIANT, sets the paths)
    import numpy as np
    import torch
    import field_ref as FR
    import gpgpuraytrace_amd as G
    assert torch.cuda.is_available(), "the measurements need the GPU"
    dev, ter = RQ.terrain("nomadplains")
    p = FR.lattice_points(ORIGIN, SPACING, DIMS)
    return RQ, np, torch, G, dev, ter, p


class Field:
    """A device-form field query with its buffers: points (b) or the lattice (c)."""

    def __init__(self, torch, G, ter, points=None, normals=False, occupancy=False):
        n = DIMS[0] * DIMS[1] * DIMS[2]
        self.G, self.ter, self.normals, self.n = G, ter, normals, n
        self.pts = torch.from_numpy(G.pack_points(points)).to("cuda:0") if points is not None else None
        self.res = torch.zeros((n, 4) if normals else (n,), dtype=torch.float32, device="cuda:0")
        self.occ = torch.zeros(n // 32, dtype=torch.int32, device="cuda:0") if occupancy else None
        torch.cuda.synchronize()

    def __call__(self):
        if self.pts is not None:
            ok = self.ter.sample_field_device(self.pts.data_ptr(), self.n, self.res.data_ptr(), eye=EYE, normals=self.normals)
        else:
            ok = self.ter.sample_lattice_device(ORIGIN, SPACING, DIMS, self.res.data_ptr(),
                                                self.occ.data_ptr() if self.occ is not None else 0, eye=EYE,
                                                normals=self.normals)
        assert ok, self.G.lib().rt_last_error()


def debug_noise(np, G, ter, p, out):
    """(a): the diagnostic over host arrays; the compute's Eye must be the query's (it takes no eye)."""
    from gpgpuraytrace_amd._native import check
    check(G.lib().rt_debug_noise(ter.camera_compute._h, p.ctypes.data, out.ctypes.data, len(p), 1), "rt_debug_noise")


def run(out_dir):
    RQ, np, torch, G, dev, ter, p = setup()
    variant = os.environ.get("RT_LIB_VARIANT", "")
    stream = torch.cuda.ExternalStream(dev.stream(), device="cuda:0")
    row = {"variant": variant, "dims": DIMS, "points": len(p)}
    b, c = Field(torch, G, ter, p), Field(torch, G, ter)
    tb, tc = RQ.pair(stream, b, c)
    dev.synchronize()
    rb, rc = b.res.cpu().numpy(), c.res.cpu().numpy()
    row["same_bits"] = bool(np.array_equal(rb.view(np.uint32), rc.view(np.uint32)))
    row["inside"] = float(np.mean(rc > 0))
    row["points_ms"], row["lattice_ms"] = RQ.summary(tb), RQ.summary(tc)
    print("%-8s points %.4f ms  lattice %.4f ms  same %s" % (variant or "default", row["points_ms"]["ms"],
                                                              row["lattice_ms"]["ms"], row["same_bits"]), flush=True)
    assert row["same_bits"]
    if not variant:
        del b
        co = Field(torch, G, ter, occupancy=True)
        tc2, tco = RQ.pair(stream, c, co)
        row["lattice_again_ms"], row["lattice_occupancy_ms"] = RQ.summary(tc2), RQ.summary(tco)
        dev.synchronize()
        words = co.occ.cpu().numpy().view(np.uint32)
        want = np.packbits((rc > 0).astype(np.uint8), bitorder="little").view("<u4")
        row["occupancy_same"] = bool(np.array_equal(words, want))
        assert row["occupancy_same"]
        del c, co
        bn, cn = Field(torch, G, ter, p, normals=True), Field(torch, G, ter, normals=True)
        tbn, tcn = RQ.pair(stream, bn, cn)
        dev.synchronize()
        row["normals_same_bits"] = bool(np.array_equal(bn.res.cpu().numpy().view(np.uint32), cn.res.cpu().numpy().view(np.uint32)))
        row["points_normals_ms"], row["lattice_normals_ms"] = RQ.summary(tbn), RQ.summary(tcn)
        assert row["normals_same_bits"]
        del bn, cn
        # (a): the whole blocking call between two events on the device's stream (upload + kernel + download)
        out = np.empty(len(p), np.float32)
        debug_noise(np, G, ter, p, out)
        ts = []
        for _ in range(3):
            ts.append(RQ.timed(stream, lambda: debug_noise(np, G, ter, p, out), 1))
        row["debug_noise_call_ms"] = RQ.summary(ts)
        row["debug_noise_same_bits"] = bool(np.array_equal(out.view(np.uint32), rc.view(np.uint32)))
        assert row["debug_noise_same_bits"]
        print("debug_noise whole call %.2f ms" % row["debug_noise_call_ms"]["ms"], flush=True)
    with open(os.path.join(out_dir, "field_query.jsonl"), "a") as f:
        f.write(json.dumps(row) + "\n")
    dev.destroy()


def trace():
    RQ, np, torch, G, dev, ter, p = setup()
    b, c = Field(torch, G, ter, p), Field(torch, G, ter)
    out = np.empty(len(p), np.float32)
    for _ in range(3):
        debug_noise(np, G, ter, p, out)
        b()
        c()
        dev.synchronize()
    dev.destroy()


def kernel_stats(path):
    """rocprofv3 --stats' per-kernel rows: name -> (calls, average ns)."""
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            for key in ("k_debug_noise", "k_fieldpoints", "k_fieldlattice"):
                if key in name:
                    out[key] = (int(r["Calls"]), float(r["AverageNs"]))
    return out


def report(out_dir, resources, stats):
    rows = [json.loads(ln) for ln in open(os.path.join(out_dir, "field_query.jsonl")) if ln.strip()]
    by = {r["variant"]: r for r in rows}
    d = by[""]
    n = d["points"]
    L = ["# Field queries: measurements (MI355X)", "",
         "`scripts/field_query_bench.sh`: a %d x %d x %d nomadplains lattice of spacing 1 around the reset pose's eye "
         "(0, 100, 0), y from 0 to 127: %d points, %.1f%% of them inside.  The device forms on the device's stream, HIP "
         "events around back-to-back launches of >= 50 ms a window, warm-up first, 5 alternating repeats per pair; ms "
         "are medians per call, the spread is (max - min) / median of a side's repeats.  Every pair's results were "
         "compared bit for bit in the run (equal)." % (DIMS + (n, 100 * d["inside"])), ""]
    L += ["## 1. The three routes (density only)", "", "| route | kernel | ms | points/s |", "|---|---|---|---|"]
    if stats:
        calls, ns = stats["k_debug_noise"]
        L.append("| (a) rt_debug_noise over the uploaded points, kernel only (kernel trace, mean of %d) | k_debug_noise | %.3f | %.3g |"
                 % (calls, ns / 1e6, n / (ns / 1e9)))
    if "debug_noise_call_ms" in d:
        L.append("| (a) the whole blocking call: upload, kernel, download (HIP events) | k_debug_noise | %.1f | %.3g |"
                 % (d["debug_noise_call_ms"]["ms"], n / (d["debug_noise_call_ms"]["ms"] / 1e3)))
    for tag, key, kern in (("(b) points from memory", "points_ms", "k_fieldpoints"),
                           ("(c) lattice, %d rows a strip, column reuse" % ROWS_DEFAULT, "lattice_ms", "k_fieldlattice")):
        L.append("| %s (HIP events) | %s | %.4f (%.1f%%) | %.3g |" % (tag, kern, d[key]["ms"], 100 * d[key]["spread"],
                                                                     n / (d[key]["ms"] / 1e3)))
    if stats:
        for key in ("k_fieldpoints", "k_fieldlattice"):
            L.append("| the same in the kernel trace (mean of %d) | %s | %.3f | |" % (stats[key][0], key, stats[key][1] / 1e6))
    L += ["", "(c) takes %.4f of (b)'s time." % (d["lattice_ms"]["ms"] / d["points_ms"]["ms"]), ""]
    L += ["## 2. The lattice kernel by strip shape and column reuse", "",
          "Each build timed against (b) in its own process (the pair alternating), so the ratio is the comparable figure.", "",
          "| build | rows a strip | column reuse | (c) ms | (b) ms beside it | (c) / (b) |", "|---|---|---|---|---|---|"]

    def shape(v):
        if v == "":
            return ROWS_DEFAULT, "yes"
        if v == "nocol":
            return ROWS_DEFAULT, "no"
        return int(v[1:]), "yes" if int(v[1:]) > 1 else "none possible (one row)"

    for v in sorted(by, key=lambda v: (shape(v)[0], shape(v)[1])):
        r = by[v]
        L.append("| %s | %d | %s | %.4f (%.1f%%) | %.4f (%.1f%%) | %.4f |" % (
            v or "default", shape(v)[0], shape(v)[1], r["lattice_ms"]["ms"], 100 * r["lattice_ms"]["spread"],
            r["points_ms"]["ms"], 100 * r["points_ms"]["spread"], r["lattice_ms"]["ms"] / r["points_ms"]["ms"]))
    best = min(by, key=lambda v: by[v]["lattice_ms"]["ms"])
    faster = d["lattice_ms"]["ms"] < d["points_ms"]["ms"]
    L += ["", "Choice: the lattice is kept as a kernel of its own only if (c) is faster than (b) here: it %s (%.4f against "
          "%.4f ms), so it %s.  The fastest strip measured is %d rows with the column reuse (%s build); the plan's "
          "rows (rt_rayquery.h kFieldRows) are %d.  (b)'s first repeat of five is the slow one in every process, "
          "which is its spread; the medians do not move with it." % (
              "is" if faster else "is not", d["lattice_ms"]["ms"], d["points_ms"]["ms"],
              "stays" if faster else "would be replaced by point generation in front of k_fieldpoints", shape(best)[0],
              best or "default", ROWS_DEFAULT)]
    L += ["", "## 3. Occupancy and normals (default build)", "", "| query | ms |", "|---|---|"]
    for tag, key in (("(c) density", "lattice_again_ms"), ("(c) density + occupancy", "lattice_occupancy_ms"),
                     ("(b) normal + density", "points_normals_ms"), ("(c) normal + density", "lattice_normals_ms")):
        if key in d:
            L.append("| %s | %.4f (%.1f%%) |" % (tag, d[key]["ms"], 100 * d[key]["spread"]))
    L.append("")
    if resources:
        L += ["## Resource usage (scripts/resource_usage.py, gfx950)", "", "```"] + resources + ["```", ""]
    with open(os.path.join(out_dir, "field_query.md"), "w") as f:
        f.write("\n".join(L))
    print("\n".join(L))


if __name__ == "__main__":
    what = sys.argv[1]
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if what == "trace":
        trace()
    elif what == "run":
        os.makedirs(sys.argv[2], exist_ok=True)
        run(sys.argv[2])
    else:
        res, st = [], None
        if "--resources" in sys.argv:
            res = [ln.rstrip() for ln in open(sys.argv[sys.argv.index("--resources") + 1]) if "k_field" in ln or "k_debug_noise" in ln]
        if "--stats" in sys.argv:
            st = kernel_stats(sys.argv[sys.argv.index("--stats") + 1])
        report(sys.argv[2], res, st)
