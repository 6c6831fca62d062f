#!/usr/bin/env python3
"""Measurements of point shading on the GPU: profiles/r15/shade_points.{md,jsonl}.

The README's lattice: 256 x 64 x 256 nomadplains points of spacing 2 from (-256, 0, -256), the eye (0, 100, 0).
rt_terrain_extract_mesh_device writes its vertices and normals; rt_terrain_shade_points_device reads those two arrays
as they are.

    python3 scripts/shade_points_bench.py run OUT_DIR
        HIP events on the device's stream (ray_query_bench.py's method: back-to-back launches of >= 50 ms a window,
        warm-up first, 5 alternating repeats per pair): the extraction against the point query at K = 0, 1 and 4,
        and the point query at K = 0 against rt_terrain_shade_rays_device for rays from the eye to the same
        vertices; the device form's arrays compared bit for bit with the host form's.  Appends one JSON line to
        OUT_DIR/shade_points.jsonl.
    RT_LIB_VARIANT=pqN python3 scripts/shade_points_bench.py util OUT_DIR
        a build with -DRT_QUERY_UTIL -DRT_POINTQ_REFILL=N (make variant): time and lane utilisation of
        k_shadepoints' march steps at K = 0, 1 and 4, and the lanes of its visits that claim points (the colour's
        FBM); appends one JSON line to OUT_DIR/shade_points_util.jsonl.
    python3 scripts/shade_points_bench.py report OUT_DIR [MD_DIR] [--resources NEW PARENT]
        MD_DIR/shade_points.md (default OUT_DIR) from the lines (no GPU); --resources: scripts/resource_usage.py's
        output for this tree and for its parent, compared kernel by kernel."""
import json
import os
import sys

DIMS, ORIGIN, SPACING, EYE = (256, 64, 256), (-256.0, 0.0, -256.0), (2.0, 2.0, 2.0), (0.0, 100.0, 0.0)
KS, SEED = (0, 1, 4), 1


class Mesh:
    """The extraction with normals into arrays of the mesh's exact size; its vertices and normals stay on the
    device for the point queries."""

    def __init__(self, torch, G, ter, nv, nt):
        self.G, self.ter, self.nv, self.nt = G, ter, nv, nt
        self.bytes = G.engine.mesh_scratch_bytes(ORIGIN, SPACING, DIMS)
        self.scratch = torch.zeros(self.bytes, dtype=torch.uint8, device="cuda:0")
        self.v = torch.zeros((nv, 4), dtype=torch.float32, device="cuda:0")
        self.n = torch.zeros((nv, 4), dtype=torch.float32, device="cuda:0")
        self.t = torch.zeros((nt, 3), dtype=torch.int32, device="cuda:0")
        self.counts = torch.zeros(2, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

    def __call__(self):
        ok = self.ter.extract_mesh_device(ORIGIN, SPACING, DIMS, self.scratch.data_ptr(), self.bytes, self.v.data_ptr(),
                                          self.n.data_ptr(), self.nv, self.t.data_ptr(), self.nt, self.counts.data_ptr(),
                                          eye=EYE)
        assert ok, self.G.lib().rt_last_error()


class Points:
    """The point query on a mesh's device arrays: results and pixels."""

    def __init__(self, torch, G, ter, mesh, k):
        self.G, self.ter, self.mesh, self.k = G, ter, mesh, k
        self.res = torch.zeros((mesh.nv, 4), dtype=torch.float32, device="cuda:0")
        self.pix = torch.zeros(mesh.nv, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

    def __call__(self):
        ok = self.ter.shade_points_device(self.mesh.v.data_ptr(), self.mesh.n.data_ptr(), self.mesh.nv, self.res.data_ptr(),
                                          self.pix.data_ptr(), eye=EYE, ao_samples=self.k, seed=SEED)
        assert ok, self.G.lib().rt_last_error()


class Rays:
    """rt_terrain_shade_rays_device for unit rays from the eye to the vertices: results and pixels."""

    def __init__(self, torch, np, G, ter, verts):
        self.G, self.ter, self.n = G, ter, len(verts)
        d = verts.astype(np.float64) - np.array(EYE, np.float64)
        d /= np.linalg.norm(d, axis=1)[:, None]
        o = np.tile(np.array(EYE, np.float32), (self.n, 1))
        self.rays = torch.from_numpy(G.pack_rays(o, d.astype(np.float32))).to("cuda:0")
        self.res = torch.zeros((self.n, 8), dtype=torch.float32, device="cuda:0")
        self.pix = torch.zeros(self.n, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

    def __call__(self):
        ok = self.ter.shade_rays_device(self.rays.data_ptr(), self.n, self.res.data_ptr(), self.pix.data_ptr(), eye=EYE)
        assert ok, self.G.lib().rt_last_error()


def _setup():
    import ray_query_bench as RQ  # (sets the paths and the library variant)
    import numpy as np
    import torch
    import gpgpuraytrace_amd as G
    assert torch.cuda.is_available(), "the measurements need the GPU"
    dev, ter = RQ.terrain("nomadplains")
    stream = torch.cuda.ExternalStream(dev.stream(), device="cuda:0")
    host = ter.extract_mesh(ORIGIN, SPACING, DIMS, eye=EYE)
    assert host is not None, G.lib().rt_last_error()
    mesh = Mesh(torch, G, ter, len(host[0]), len(host[2]))
    mesh()
    dev.synchronize()
    return RQ, np, torch, G, dev, ter, stream, host, mesh


def run(out_dir):
    RQ, np, torch, G, dev, ter, stream, host, mesh = _setup()
    hv, hn = host[0], host[1]
    row = {"dims": DIMS, "vertices": mesh.nv, "triangles": mesh.nt, "seed": SEED}
    same = True
    for k in KS:
        q = Points(torch, G, ter, mesh, k)
        ta, tb = RQ.pair(stream, mesh, q)
        dev.synchronize()
        want = ter.shade_points(hv, hn, eye=EYE, ao_samples=k, seed=SEED, rgba8=True)
        assert want is not None, G.lib().rt_last_error()
        same = same and bool(np.array_equal(q.res.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
                             and np.array_equal(q.pix.cpu().numpy().view(np.uint32), want[1]))
        row["extract_beside_k%d_ms" % k], row["points_k%d_ms" % k] = RQ.summary(ta), RQ.summary(tb)
        print("K = %d  extract %.4f ms, points %.4f ms (%.1f%%)" % (k, row["extract_beside_k%d_ms" % k]["ms"],
                                                                   row["points_k%d_ms" % k]["ms"],
                                                                   100 * row["points_k%d_ms" % k]["spread"]), flush=True)
        row["mean_ao_k%d" % k] = float(want[0][:, 3].mean())
    row["same_bits"] = same
    assert same
    rays = Rays(torch, np, G, ter, hv)
    tc, td = RQ.pair(stream, Points(torch, G, ter, mesh, 0), rays)
    dev.synchronize()
    row["points_k0_beside_rays_ms"], row["shade_rays_ms"] = RQ.summary(tc), RQ.summary(td)
    row["shade_rays_hits"] = int((rays.res.cpu().numpy()[:, 7] > 0).sum())
    print("K = 0  points %.4f ms, shade_rays to the same vertices %.4f ms (%d of %d rays hit)" % (
        row["points_k0_beside_rays_ms"]["ms"], row["shade_rays_ms"]["ms"], row["shade_rays_hits"], mesh.nv), flush=True)
    with open(os.path.join(out_dir, "shade_points.jsonl"), "a") as f:
        f.write(json.dumps(row) + "\n")
    dev.destroy()


def util(out_dir):
    import ctypes as C
    RQ, np, torch, G, dev, ter, stream, host, mesh = _setup()
    L = G.lib()
    L.rt_debug_query_util.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    for k in KS:
        q = Points(torch, G, ter, mesh, k)
        s = RQ.summary([RQ.timed(stream, q, RQ.reps_for(stream, q)) for _ in range(RQ.REPEATS)])
        buf = (C.c_ulonglong * 4)()
        assert L.rt_debug_query_util(buf, 1) == 4
        q()
        dev.synchronize()
        assert L.rt_debug_query_util(buf, 1) == 4
        s.update({"variant": os.environ.get("RT_LIB_VARIANT", ""), "k": k, "n": mesh.nv, "wave_steps": int(buf[0]),
                  "lane_steps": int(buf[1]), "claim_visits": int(buf[2]), "claim_lanes": int(buf[3]),
                  "march_utilisation": buf[1] / (64.0 * max(buf[0], 1)),
                  "claim_utilisation": buf[3] / (64.0 * max(buf[2], 1))})
        print(json.dumps(s), flush=True)
        with open(os.path.join(out_dir, "shade_points_util.jsonl"), "a") as f:
            f.write(json.dumps(s) + "\n")
    dev.destroy()


def _resources(new, parent):
    """Lines of the comparison and of the new kernel from two outputs of scripts/resource_usage.py."""
    def table(path):
        return {ln.split(" vgpr=")[0].strip(): ln.split(" vgpr=")[1].strip() for ln in open(path) if " vgpr=" in ln}
    a, b = table(new), table(parent)
    changed = [k for k in b if a.get(k) != b[k]]
    added = [k for k in a if k not in b]
    L = ["## Registers and code size", "",
         "`scripts/resource_usage.py` for this tree and for its parent: %d kernels in the parent, %d of them with other "
         "figures here (VGPRs, SGPRs, spills, scratch, occupancy, LDS, code bytes)%s; %d new:" % (
             len(b), len(changed), "" if changed else ": every earlier kernel is byte-identical in size and registers",
             len(added)), "", "```"]
    L += ["%-34s vgpr=%s" % (k, a[k]) for k in added]
    L += ["```", "", "k_shadequery beside it:", "", "```"]
    L += ["%-34s vgpr=%s" % (k, a[k]) for k in a if "k_shadequery" in k]
    L += ["```", ""]
    for k in changed:
        L.append("CHANGED %s: %s -> %s" % (k, b[k], a[k]))
    return L


def report(out_dir, md_dir, resources):
    d = [json.loads(ln) for ln in open(os.path.join(out_dir, "shade_points.jsonl")) if ln.strip()][-1]
    L = ["# Point shading: measurements (MI355X)", "",
         "`scripts/shade_points_bench.py`: the README's %d x %d x %d nomadplains lattice of spacing 2 from (-256, 0, -256), "
         "eye (0, 100, 0): %d vertices, %d triangles.  `rt_terrain_shade_points_device` reads "
         "`rt_terrain_extract_mesh_device`'s vertices and normals arrays as they are and writes results and pixels; seed "
         "%d.  The device forms on the device's stream, HIP events around back-to-back launches of >= 50 ms a window, "
         "warm-up first, 5 alternating repeats per pair; ms are medians per call, the spread is (max - min) / median of "
         "a side's repeats.  The device form's results and pixels were compared bit for bit with the host form's in the "
         "run (equal)." % (tuple(d["dims"]) + (d["vertices"], d["triangles"], d["seed"])), "",
         "| K | shade_points_device, ms | extract_mesh_device (normals) beside it, ms | ns a point | mean ao |",
         "|---|---|---|---|---|"]
    for k in KS:
        p, e = d["points_k%d_ms" % k], d["extract_beside_k%d_ms" % k]
        L.append("| %d | %.4f (%.1f%%) | %.4f (%.1f%%) | %.1f | %.3f |" % (
            k, p["ms"], 100 * p["spread"], e["ms"], 100 * e["spread"], 1e6 * p["ms"] / d["vertices"], d["mean_ao_k%d" % k]))
    p, r = d["points_k0_beside_rays_ms"], d["shade_rays_ms"]
    L += ["", "At K = 0 against the only route there was: `rt_terrain_shade_rays_device` for unit rays from the eye to the "
          "same vertices (default range and stepmod; %d of the %d rays end in a hit, on a refined sample near the vertex, "
          "and the colour carries the view's fog and sky blends): %.4f ms (%.1f%%) against %.4f ms (%.1f%%) for the point "
          "query beside it, %.2fx.  The difference is the primary march, getNormal and the sky." % (
              d["shade_rays_hits"], d["vertices"], r["ms"], 100 * r["spread"], p["ms"], 100 * p["spread"],
              r["ms"] / p["ms"]), ""]
    up = os.path.join(out_dir, "shade_points_util.jsonl")
    if os.path.exists(up):
        rows = [json.loads(ln) for ln in open(up) if ln.strip()]
        last = {}
        for r_ in rows:  # a variant measured in several passes: its repeats pooled
            key = (r_["variant"], r_["k"])
            runs = last[key]["runs_ms"] + r_["runs_ms"] if key in last else r_["runs_ms"]
            med = sorted(runs)[len(runs) // 2] if len(runs) % 2 else sum(sorted(runs)[len(runs) // 2 - 1:len(runs) // 2 + 1]) / 2
            last[key] = dict(r_, runs_ms=runs, ms=med, spread=(max(runs) - min(runs)) / med)
        names = sorted({v for v, _ in last}, key=lambda v: int("".join(c for c in v if c.isdigit()) or 0))
        L += ["## The refill threshold (RT_POINTQ_REFILL) and the lanes' utilisation", "",
              "Builds with `-DRT_QUERY_UTIL -DRT_POINTQ_REFILL=N` (`make variant NAME=pqN`), the same query: ms per call "
              "(the median of every pass's 5 repeats, the passes over the builds in ascending and then descending order; the "
              "counters' atomics included, so compare the rows with each other, not with the table above), "
              "the live lanes over the waves' march steps, and the lanes of the visits that claim points (where the "
              "colour's FBM runs).", "",
              "| N | " + " | ".join("K = %d: ms | march lanes | claim lanes" % k for k in KS) + " |",
              "|---|" + "---|---|---|" * len(KS)]
        for v in names:
            cells = []
            for k in KS:
                r_ = last.get((v, k))
                cells.append("%.4f (%.1f%%) | %.1f%% | %.1f%%" % (r_["ms"], 100 * r_["spread"], 100 * r_["march_utilisation"],
                                                                 100 * r_["claim_utilisation"]) if r_ else "- | - | -")
            L.append("| %s | %s |" % ("".join(c for c in v if c.isdigit()), " | ".join(cells)))
        k = KS[-1]
        at = {v: last[(v, k)] for v in names if (v, k) in last}
        if "pq32" in at:
            best = min(at, key=lambda v: at[v]["ms"])
            noise = max(at["pq32"]["spread"], at[best]["spread"])
            near = [v[2:] for v in names if v in at and at[v]["ms"] <= at[best]["ms"] * (1 + noise)]
            L += ["", "At K = %d the fastest build is N = %s; N = 32 (RT_SHADEQ_REFILL's value, where this started) is %+.1f%% "
                  "from it, against a spread of %.1f%% on the larger of the two sides, and N = %s lie within that spread of "
                  "the fastest.  %s.  At K = 0 a point "
                  "has one march and the threshold only decides when the next points' colour is taken; the rows do not "
                  "differ beyond their spreads.  A lane holds its point through 1 + K marches of unlike length (a shadow "
                  "ray to 100, AO rays to 25, each ending at its first hit), which is what the march lanes' share shows.  "
                  "The per-ray shape (each (point, k) its own work item, occ an atomic) was not measured." % (
                      k, best[2:], 100 * (at["pq32"]["ms"] / at[best]["ms"] - 1), 100 * noise, ", ".join(near),
                      "No value beats 32 by more than that, so RT_POINTQ_REFILL stays 32" if "32" in near
                      else "RT_POINTQ_REFILL follows the fastest (rt_variants.h)")]
        L.append("")
    if resources:
        L += _resources(*resources)
    os.makedirs(md_dir, exist_ok=True)
    with open(os.path.join(md_dir, "shade_points.md"), "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    what = sys.argv[1]
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if what in ("run", "util"):
        os.makedirs(sys.argv[2], exist_ok=True)
        (run if what == "run" else util)(sys.argv[2])
    else:
        args = sys.argv[2:]
        res = None
        if "--resources" in args:
            i = args.index("--resources")
            res = (args[i + 1], args[i + 2])
            args = args[:i]
        report(args[0], args[1] if len(args) > 1 else args[0], res)
