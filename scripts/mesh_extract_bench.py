#!/usr/bin/env python3
"""Measurements of the mesh extraction on the GPU: profiles/r14/mesh_extract.{md,jsonl}.

The README's lattice: 256 x 64 x 256 nomadplains points of spacing 2 from (-256, 0, -256), the eye (0, 100, 0)
(4,194,304 points).  rt_terrain_extract_mesh_device (the density and occupancy pass, then k_meshcount, k_meshscan,
k_meshemit and k_meshnormals) against rt_terrain_sample_lattice_device alone (the same density and occupancy pass
into buffers of its own), so the difference is what passes 2-5 cost on top of pass 1.

    python3 scripts/mesh_extract_bench.py run OUT_DIR
        HIP events on the device's stream (ray_query_bench.py's method: back-to-back launches of >= 50 ms a window,
        warm-up first, 5 alternating repeats per pair): the lattice against the extraction with normals, without
        normals, and as a counting call; the device form's arrays compared bit for bit with the host form's.
        Appends one JSON line to OUT_DIR/mesh_extract.jsonl.
    python3 scripts/mesh_extract_bench.py report OUT_DIR [MD_DIR]
        MD_DIR/mesh_extract.md (default OUT_DIR) from the lines (no GPU)."""
import json
import os
import sys

DIMS, ORIGIN, SPACING, EYE = (256, 64, 256), (-256.0, 0.0, -256.0), (2.0, 2.0, 2.0), (0.0, 100.0, 0.0)


class Lattice:
    """Pass 1 alone: the lattice's densities and occupancy words into device arrays."""

    def __init__(self, torch, G, ter):
        n = DIMS[0] * DIMS[1] * DIMS[2]
        self.G, self.ter = G, ter
        self.res = torch.zeros(n, dtype=torch.float32, device="cuda:0")
        self.occ = torch.zeros(n // 32, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

    def __call__(self):
        ok = self.ter.sample_lattice_device(ORIGIN, SPACING, DIMS, self.res.data_ptr(), self.occ.data_ptr(), eye=EYE)
        assert ok, self.G.lib().rt_last_error()


class Extract:
    """The device form with arrays of the mesh's exact size (nv, nt), or a counting call (0, 0)."""

    def __init__(self, torch, G, ter, nv, nt, normals):
        self.G, self.ter, self.nv, self.nt = G, ter, nv, nt
        self.bytes = G.engine.mesh_scratch_bytes(ORIGIN, SPACING, DIMS)
        self.scratch = torch.zeros(self.bytes, dtype=torch.uint8, device="cuda:0")
        self.v = torch.zeros((max(nv, 1), 4), dtype=torch.float32, device="cuda:0")
        self.n = torch.zeros((max(nv, 1), 4), dtype=torch.float32, device="cuda:0") if normals else None
        self.t = torch.zeros((max(nt, 1), 3), dtype=torch.int32, device="cuda:0")
        self.counts = torch.zeros(2, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

    def __call__(self):
        ok = self.ter.extract_mesh_device(ORIGIN, SPACING, DIMS, self.scratch.data_ptr(), self.bytes,
                                          self.v.data_ptr() if self.nv else 0,
                                          self.n.data_ptr() if self.n is not None and self.nv else 0, self.nv,
                                          self.t.data_ptr() if self.nt else 0, self.nt, self.counts.data_ptr(), eye=EYE)
        assert ok, self.G.lib().rt_last_error()


def run(out_dir):
    import ray_query_bench as RQ  # (sets the paths)
    import numpy as np
    import torch
    import gpgpuraytrace_amd as G
    assert torch.cuda.is_available(), "the measurements need the GPU"
    dev, ter = RQ.terrain("nomadplains")
    stream = torch.cuda.ExternalStream(dev.stream(), device="cuda:0")
    host = ter.extract_mesh(ORIGIN, SPACING, DIMS, eye=EYE)
    assert host is not None, G.lib().rt_last_error()
    hv, hn, ht, hc = host
    nv, nt = len(hv), len(ht)
    cells = (DIMS[0] - 1) * (DIMS[1] - 1) * (DIMS[2] - 1)
    row = {"dims": DIMS, "points": DIMS[0] * DIMS[1] * DIMS[2], "cells": cells, "vertices": nv, "triangles": nt,
           "scratch_bytes": G.engine.mesh_scratch_bytes(ORIGIN, SPACING, DIMS)}
    lat, full = Lattice(torch, G, ter), Extract(torch, G, ter, nv, nt, True)
    ta, tb = RQ.pair(stream, lat, full)
    dev.synchronize()
    got_v, got_n, got_t = (x.cpu().numpy() for x in (full.v, full.n, full.t))
    row["same_bits"] = bool(
        full.counts.cpu().numpy().tolist() == [nv, nt]
        and np.array_equal(got_v[:, :3].view(np.uint32), hv.view(np.uint32))
        and np.array_equal(got_v[:, 3].view(np.uint32), hc) and np.array_equal(got_n.view(np.uint32), hn.view(np.uint32))
        and np.array_equal(got_t.view(np.uint32), ht))
    assert row["same_bits"]
    row["lattice_ms"], row["extract_normals_ms"] = RQ.summary(ta), RQ.summary(tb)
    bare = Extract(torch, G, ter, nv, nt, False)
    ta2, tc = RQ.pair(stream, lat, bare)
    row["lattice_again_ms"], row["extract_ms"] = RQ.summary(ta2), RQ.summary(tc)
    count = Extract(torch, G, ter, 0, 0, False)
    ta3, td = RQ.pair(stream, lat, count)
    row["lattice_third_ms"], row["count_ms"] = RQ.summary(ta3), RQ.summary(td)
    for k in ("lattice_ms", "extract_normals_ms", "extract_ms", "count_ms"):
        print("%-20s %.4f ms (%.1f%%)" % (k, row[k]["ms"], 100 * row[k]["spread"]), flush=True)
    with open(os.path.join(out_dir, "mesh_extract.jsonl"), "a") as f:
        f.write(json.dumps(row) + "\n")
    dev.destroy()


def report(out_dir, md_dir):
    d = [json.loads(ln) for ln in open(os.path.join(out_dir, "mesh_extract.jsonl")) if ln.strip()][-1]

    def share(key, beside):
        return (d[key]["ms"] - d[beside]["ms"]) / d[beside]["ms"]

    L = ["# Mesh extraction: measurements (MI355X)", "",
         "`scripts/mesh_extract_bench.py`: the README's %d x %d x %d nomadplains lattice of spacing 2 from (-256, 0, -256), "
         "eye (0, 100, 0): %d points, %d cells, of which %d (%.2f%%) carry a vertex; %d triangles; scratch %.1f MiB.  The "
         "device forms on the device's stream, HIP events around back-to-back launches of >= 50 ms a window, warm-up "
         "first, 5 alternating repeats per pair; ms are medians per call, the spread is (max - min) / median of a "
         "side's repeats.  The device form's arrays were compared bit for bit with the host form's in the run (equal)."
         % (tuple(d["dims"]) + (d["points"], d["cells"], d["vertices"], 100.0 * d["vertices"] / d["cells"],
                               d["triangles"], d["scratch_bytes"] / 2 ** 20)), "",
         "| call | passes | ms | pass 1 beside it, ms | over pass 1 |", "|---|---|---|---|---|"]
    for tag, passes, key, beside in (
            ("rt_terrain_extract_mesh_device, normals", "1-5", "extract_normals_ms", "lattice_ms"),
            ("the same without normals", "1-4", "extract_ms", "lattice_again_ms"),
            ("the same as a counting call (capacities 0)", "1-3", "count_ms", "lattice_third_ms")):
        L.append("| %s | %s | %.4f (%.1f%%) | %.4f (%.1f%%) | %+.1f%% |" % (
            tag, passes, d[key]["ms"], 100 * d[key]["spread"], d[beside]["ms"], 100 * d[beside]["spread"],
            100 * share(key, beside)))
    L += ["", "Pass 1 is rt_terrain_sample_lattice_device alone (k_fieldlattice: densities and occupancy words).  "
          "Passes 2-5 (k_meshcount, k_meshscan, k_meshemit, k_meshnormals) cost %.1f%% of pass 1; without the normal "
          "pass, passes 2-4 cost %.1f%%; counting alone, passes 2-3 cost %.1f%%." % (
              100 * share("extract_normals_ms", "lattice_ms"), 100 * share("extract_ms", "lattice_again_ms"),
              100 * share("count_ms", "lattice_third_ms")), ""]
    os.makedirs(md_dir, exist_ok=True)
    with open(os.path.join(md_dir, "mesh_extract.md"), "w") as f:
        f.write("\n".join(L))
    print("\n".join(L))


if __name__ == "__main__":
    what = sys.argv[1]
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if what == "run":
        os.makedirs(sys.argv[2], exist_ok=True)
        run(sys.argv[2])
    else:
        report(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else sys.argv[2])
