#!/usr/bin/env python3
"""Measurements of the surface queries (rt_terrain_trace_surface_device) on the GPU: profiles/r10/surface_query.{md,json}.

    python3 scripts/surface_query_bench.py bars OUT_DIR [--resources FILE]
        1. time per query at n = 1, 1024, 65,536 and 2^20 nomadplains rays in both shapes, each beside
           rt_terrain_trace_rays_device on the same rays in the same shape (the baseline: the existing kernel),
           and the time per march iteration (the query's own step counts, which the GPU tests hold equal to the
           checker's, plus 3 density samples per hit for the normal);
        2. both forced shapes by n (the auto rule's crossing);
        3. one pick (n = 1, segments) in microseconds.
    RT_LIB_VARIANT=NAME python3 scripts/surface_query_bench.py util OUT_DIR
        a build with -DRT_QUERY_UTIL (make variant): lane utilisation of the lane shape's march steps and of its
        normal evaluations at n = 2^20; appends one JSON line to OUT_DIR/surface_query_util.jsonl.

Rays: F0's 1024 prepass rays (tests/ray_fixture.py) with their origins moved over a 32 x 32 grid of pitch 8 and
F0's own directions (shifted_rays says why not dir = origin - eye); n = 1 is F0's centre ray.  Timing as
ray_query_bench.py: the device form
on the device's stream, HIP events around back-to-back launches of >= 50 ms a window, warm-up first, 5 repeats a
pair with the two sides alternating."""
import json
import os
import sys

import ray_query_bench as RQ  # (applies RT_LIB_VARIANT, sets the paths)

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpgpuraytrace_amd as G  # noqa: E402
import ray_fixture as RF  # noqa: E402

MAIN = (1, 1024, 65536, 1 << 20)
CROSSING = (64, 4096, 16384, 32768, 131072, 196608, 262144)
EYE = RF.eye("F0")


def shifted_rays(n):
    """n rays: F0's centre ray, or the first n of ceil(n / 1024) copies of F0's rays with their ORIGINS moved by
    (8 a, 0, 8 b), camera k = 32 b + a on a 32 x 32 grid, and F0's own direction vectors.  (Moving the origin
    alone and forming dir = origin - eye, as ray_query_bench.py's 24 cameras do, makes |dir| grow with the
    shift; |dir| enters the first step, and from a few hundred units on the rays leave the range in a handful
    of iterations: no workload.)  The LOD eye stays F0's, so the far cameras see fewer octaves."""
    sx, sy = (v.astype(np.float64)[:, None] for v in RF.screen_coords())
    if n == 1:
        sx, sy = sx[528:529], sy[528:529]
    e, t, r0, r1, r2 = RF.camera("F0")
    o0 = t + (r2 + (sy * r1 + sx * r0))
    d0 = o0 - e
    cams = (n + 1023) // 1024
    assert cams <= 1024
    o = np.concatenate([o0 + np.array([8.0 * (k % 32), 0.0, 8.0 * (k // 32)]) for k in range(cams)])[:n]
    d = np.concatenate([d0] * cams)[:n]
    return o.astype(np.float32), d.astype(np.float32)


class Surface:
    """A device-form surface query with its buffers."""

    def __init__(self, ter, o, d, mode):
        self.ter, self.n, self.mode = ter, len(o), mode
        self.rays = torch.from_numpy(G.pack_rays(o, d)).to("cuda:0")
        self.res = torch.zeros((self.n, 8), dtype=torch.float32, device="cuda:0")
        self.steps = torch.zeros(self.n, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

    def __call__(self):
        ok = self.ter.trace_surface_device(self.rays.data_ptr(), self.n, self.res.data_ptr(), eye=EYE, mode=self.mode)
        assert ok, G.lib().rt_last_error()

    def iterations(self, dev):
        """(march iterations, hits) of the query, from its own step counts."""
        assert self.ter.trace_surface_device(self.rays.data_ptr(), self.n, self.res.data_ptr(), self.steps.data_ptr(),
                                             eye=EYE, mode=self.mode)
        dev.synchronize()
        return int(self.steps.cpu().numpy().astype(np.int64).sum()), int((self.res.cpu().numpy()[:, 7] > 0).sum())


def prepass_iterations(dev, ter, q):
    st = torch.zeros(q.n, dtype=torch.int32, device="cuda:0")
    assert ter.trace_rays_device(q.rays.data_ptr(), q.n, q.res.data_ptr(), st.data_ptr(), eye=EYE, mode=q.mode)
    dev.synchronize()
    return int(st.cpu().numpy().astype(np.int64).sum())


def bars(out):
    dev, ter = RQ.terrain("nomadplains")
    stream = torch.cuda.ExternalStream(dev.stream(), device="cuda:0")
    rows = []
    for n in MAIN:
        o, d = shifted_rays(n)
        row = {"n": n}
        bits = {}
        for mode in ("segments", "lanes"):
            qs, qr = Surface(ter, o, d, mode), RQ.Query(ter, o, d, EYE, mode)
            ts, tr = RQ.pair(stream, qs, qr)
            iters, hits = qs.iterations(dev)
            bits[mode] = qs.res.cpu().numpy().view(np.uint32)
            pre = prepass_iterations(dev, ter, qr)
            s, r = RQ.summary(ts), RQ.summary(tr)
            s.update({"iterations": iters, "hits": hits, "ns_per_iteration": s["ms"] * 1e6 / max(iters + 3 * hits, 1)})
            r.update({"iterations": pre, "ns_per_iteration": r["ms"] * 1e6 / max(pre, 1)})
            row[mode] = {"surface": s, "trace_rays": r}
            print("n=%8d %-8s surface %.4f ms (%.4f ns/it)  trace_rays %.4f ms (%.4f ns/it)" % (
                n, mode, s["ms"], s["ns_per_iteration"], r["ms"], r["ns_per_iteration"]), flush=True)
        assert np.array_equal(bits["segments"], bits["lanes"]), n
        rows.append(row)
    out["main"] = rows
    cross = [{"n": r["n"], "segments": r["segments"]["surface"], "lanes": r["lanes"]["surface"]} for r in rows]
    for n in CROSSING:
        o, d = shifted_rays(n)
        qs, ql = Surface(ter, o, d, "segments"), Surface(ter, o, d, "lanes")
        ts, tl = RQ.pair(stream, qs, ql)
        cross.append({"n": n, "segments": RQ.summary(ts), "lanes": RQ.summary(tl)})
        print("n=%8d segments %.4f ms  lanes %.4f ms" % (n, cross[-1]["segments"]["ms"], cross[-1]["lanes"]["ms"]), flush=True)
    out["crossing"] = sorted(cross, key=lambda r: r["n"])
    dev.destroy()


def util(out_dir):
    L = G.lib()
    L.rt_debug_query_util.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    n = 1 << 20
    o, d = shifted_rays(n)
    dev, ter = RQ.terrain("nomadplains")
    stream = torch.cuda.ExternalStream(dev.stream(), device="cuda:0")
    q = Surface(ter, o, d, "lanes")
    r = RQ.reps_for(stream, q)
    s = RQ.summary([RQ.timed(stream, q, r) for _ in range(RQ.REPEATS)])
    buf = (C.c_ulonglong * 4)()
    assert L.rt_debug_query_util(buf, 1) == 4
    q()
    dev.synchronize()
    assert L.rt_debug_query_util(buf, 1) == 4
    s.update({"variant": os.environ.get("RT_LIB_VARIANT", ""), "wave_steps": int(buf[0]), "lane_steps": int(buf[1]),
              "normal_wave_calls": int(buf[2]), "normal_lanes": int(buf[3]),
              "march_utilisation": buf[1] / (64.0 * max(buf[0], 1)),
              "normal_utilisation": buf[3] / (64.0 * max(buf[2], 1)),
              # a normal evaluation is 3 density samples of the wave, a march step 1
              "normal_share_of_wave_samples": 3.0 * buf[2] / max(buf[0] + 3.0 * buf[2], 1)})
    print(json.dumps(s), flush=True)
    with open(os.path.join(out_dir, "surface_query_util.jsonl"), "a") as f:
        f.write(json.dumps(s) + "\n")
    dev.destroy()


def markdown(out, resources):
    lines = ["# Surface queries: measurements (MI355X)", "",
             "`scripts/surface_query_bench.py bars`: the device form, HIP events around back-to-back launches of >= 50 ms "
             "a window, warm-up first, 5 alternating repeats per pair; ms are medians per call, the spread is "
             "(max - min) / median of a side's repeats.  Rays: F0's prepass rays, their origins moved over a 32 x 32 grid "
             "of pitch 8 with F0's own directions and F0's eye as the LOD eye; n = 1 is F0's centre ray.  `trace_rays` is rt_terrain_trace_rays_device on the same rays in "
             "the same shape and process: the baseline (the existing kernel).  Iterations are the queries' own step "
             "counts; a surface query's count adds 3 density samples per hit for the normal.", "",
             "## 1. Time per query and per march iteration (nomadplains)", "",
             "| n | shape | surface ms | trace_rays ms | surface iterations (+3/hit) | surface ns/iteration | trace_rays ns/iteration |",
             "|---|---|---|---|---|---|---|"]
    for r in out["main"]:
        for mode in ("segments", "lanes"):
            s, t = r[mode]["surface"], r[mode]["trace_rays"]
            lines.append("| %d | %s | %.4f (%.1f%%) | %.4f (%.1f%%) | %d | %.4f | %.4f |" % (
                r["n"], mode, s["ms"], 100 * s["spread"], t["ms"], 100 * t["spread"], s["iterations"] + 3 * s["hits"],
                s["ns_per_iteration"], t["ns_per_iteration"]))
    big = out["main"][-1]["lanes"]
    ratio = big["surface"]["ns_per_iteration"] / big["trace_rays"]["ns_per_iteration"]
    out["lanes_ns_per_iteration_ratio_2p20"] = ratio
    lines += ["", "Lanes at 2^20 rays: the surface query's time per iteration is %.3f x the ray query's." % ratio, "",
              "## 2. Both shapes by n (the auto rule's crossing)", "",
              "| n | segments ms | lanes ms | faster |", "|---|---|---|---|"]
    for r in out["crossing"]:
        s, l = r["segments"]["ms"], r["lanes"]["ms"]
        lines.append("| %d | %.4f (%.1f%%) | %.4f (%.1f%%) | %s |" % (
            r["n"], s, 100 * r["segments"]["spread"], l, 100 * r["lanes"]["spread"], "segments" if s < l else "lanes"))
    pick = out["main"][0]["segments"]
    lines += ["", "## 3. One pick (n = 1, segments)", "",
              "%.1f us a surface query (%d iterations), %.1f us the same ray through trace_rays (%d iterations)." % (
                  1e3 * pick["surface"]["ms"], pick["surface"]["iterations"], 1e3 * pick["trace_rays"]["ms"],
                  pick["trace_rays"]["iterations"]), ""]
    if resources:
        lines += ["## Resource usage (scripts/resource_usage.py, gfx950)", "", "```"] + resources + ["```", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    what, out_dir = sys.argv[1], sys.argv[2]
    os.makedirs(out_dir, exist_ok=True)
    assert torch.cuda.is_available(), "the measurements need the GPU"
    if what == "util":
        util(out_dir)
    else:
        res = []
        if "--resources" in sys.argv:
            res = [ln.rstrip() for ln in open(sys.argv[sys.argv.index("--resources") + 1])
                   if "k_query" in ln and "SurfPolicy" in ln]
        out = {}
        bars(out)
        md = markdown(out, res)
        with open(os.path.join(out_dir, "surface_query.json"), "w") as f:
            json.dump(out, f, indent=1)
        with open(os.path.join(out_dir, "surface_query.md"), "w") as f:
            f.write(md)
        print(md)
