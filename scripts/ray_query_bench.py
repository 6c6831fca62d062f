#!/usr/bin/env python3
"""Measurements of the ray queries (rt_terrain_trace_rays_device) on the GPU: profiles/r08/ray_query.{md,json}.

    python3 scripts/ray_query_bench.py bars OUT_DIR [--resources FILE]
        1. the query of 24 fixture-style cameras' 24,576 rays (auto mode) against their prepass through
           rt_terrain_prepass_batch -- the only route to those hits before -- with the results compared bit for bit;
        2. both forced shapes at n = 1 .. 2^20 on nomadplains (the auto rule's crossing);
        3. n = 2^20 on every landscape, in rays/s.
    RT_LIB_VARIANT=rqN python3 scripts/ray_query_bench.py util OUT_DIR
        a build with -DRT_QUERY_UTIL -DRT_RAYQ_REFILL=N (make variant): time and lane utilisation of the lane shape
        at n = 2^20 on nomadplains, the rays in grid order and under a seeded permutation; appends one JSON line
        each to OUT_DIR/ray_query_util.jsonl.

The device form on the device's stream, HIP events around R back-to-back launches (R sized so that a window lasts
>= 50 ms), every shape warmed up first, 5 repeats per pair with the two sides alternating; the spread of a side is
(max - min) / median of its repeats.  --resources embeds scripts/resource_usage.py's lines for the ray queries'
kernels."""
import json
import math
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import with_variant  # noqa: E402

with_variant.apply()
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpgpuraytrace_amd as G  # noqa: E402
import ray_fixture as RF  # noqa: E402  (the exact cameras; no oracle call here)
from gpgpuraytrace_amd import engine as E  # noqa: E402

REPEATS, WINDOW_MS = 5, 50.0
SIZES = (1, 64, 1024, 4096, 16384, 65536, 131072, 196608, 262144, 1 << 20)  # (two more around the crossing)


class FixedCamera:
    def __init__(self, consts):
        self.c = consts
        self.width, self.height = consts["width"], consts["height"]

    def view_inverse_hlsl(self):
        return np.asarray(self.c["view_inverse"], np.float32)

    def projection_hlsl(self):
        return np.asarray(self.c["projection"], np.float32)

    def eye(self):
        return np.asarray(self.c["eye"], np.float32)


def grid_rays(n):
    """A grid of n rays through F0's camera (screen coordinates -1 .. 1), sqrt(n) x sqrt(n) where n is a square,
    else the most nearly square a x b = n; not exact, not compared with the oracle."""
    e, t, r0, r1, r2 = RF.camera("F0")
    a = next(k for k in range(int(math.isqrt(n)), 0, -1) if n % k == 0)
    lin = lambda m: np.linspace(-1.0, 1.0, m) if m > 1 else np.zeros(1)  # noqa: E731
    sx, sy = np.meshgrid(lin(n // a), lin(a))
    o = t + r2 + sy.reshape(-1, 1) * r1 + sx.reshape(-1, 1) * r0
    return o.astype(np.float32), (o - e).astype(np.float32)


def timed(stream, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def reps_for(stream, fn):
    fn()
    fn()  # warm-up: code objects, allocations, the constants' upload
    t = timed(stream, fn, 1)
    return max(1, min(400, int(math.ceil(WINDOW_MS / max(t, 1e-3)))))


def pair(stream, fa, fb):
    """5 alternating repeats of two sides -> (times_a, times_b) in ms per call."""
    ra, rb = reps_for(stream, fa), reps_for(stream, fb)
    ta, tb = [], []
    for _ in range(REPEATS):
        ta.append(timed(stream, fa, ra))
        tb.append(timed(stream, fb, rb))
    return ta, tb


def summary(ts):
    med = float(np.median(ts))
    return {"ms": med, "spread": float((max(ts) - min(ts)) / med), "runs_ms": [float(t) for t in ts]}


class Query:
    """A device-form query with its buffers."""

    def __init__(self, ter, o, d, eye, mode="auto"):
        self.ter, self.n, self.eye, self.mode = ter, len(o), eye, mode
        self.rays = torch.from_numpy(G.pack_rays(o, d)).to("cuda:0")
        self.res = torch.zeros((self.n, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()

    def __call__(self):
        ok = self.ter.trace_rays_device(self.rays.data_ptr(), self.n, self.res.data_ptr(), eye=self.eye, mode=self.mode)
        assert ok, G.lib().rt_last_error()


def terrain(land, size=64):
    dev = G.DeviceFactory.construct(G.DeviceAPI.HIP, size, size, gpu=0)
    assert dev is not None, G.lib().rt_last_error()
    ter = G.Terrain(dev, land)
    ter.create()
    assert ter.reload(), G.lib().rt_last_error()
    ter.set_camera(FixedCamera(RF.consts("F0")))
    ter.set_time_of_day(0.3)
    ter.update_shaders()
    return dev, ter


def bar1(out):
    """24 cameras, one eye: F0 with T moved by multiples of (8, 0, 8)."""
    B = 24
    shifts = [(8 * k, 0, 8 * k) for k in range(B)]
    ring = E.FrameRing(RF.SIZE, RF.SIZE, depth=1, gpu=0, theme="nomadplains", camera=FixedCamera(RF.consts("F0")),
                       time_of_day=0.3, batch=B)
    ters = [t for _, t in ring.slots[:B]]
    for t, s in zip(ters, shifts):
        t.set_camera(FixedCamera(RF.consts("F0", s)))
        t.update_terrain()
    cam = torch.zeros((B * 1024, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(ring.slots[0][0].stream(), device="cuda:0")
    parts = [RF.rays("F0", s) for s in shifts]
    o, d = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    q = Query(ters[0], o, d, RF.eye("F0"), "auto")
    ql = Query(ters[0], o, d, RF.eye("F0"), "lanes")

    def prepass():
        E.prepass_batch(ters, 0, B, cam.data_ptr())

    tp, tq = pair(stream, prepass, q)
    _, tl = pair(stream, prepass, ql)
    ring.synchronize()
    same = bool(np.array_equal(cam.cpu().numpy().view(np.uint32), q.res.cpu().numpy().view(np.uint32)))
    same_l = bool(np.array_equal(cam.cpu().numpy().view(np.uint32), ql.res.cpu().numpy().view(np.uint32)))
    assert same and same_l, "the query's results differ from the prepass's CameraResults"
    sp, sq, sl = summary(tp), summary(tq), summary(tl)
    margin = max(sp["spread"], sq["spread"])
    out["bar1"] = {"rays": B * 1024, "prepass_batch": sp, "query_auto": sq, "query_lanes": sl, "results_equal": same,
                   "met": bool(sq["ms"] <= sp["ms"] * (1.0 + margin)), "margin": margin,
                   "baseline_rays_per_s": B * 1024 / (sp["ms"] * 1e-3)}
    ring.destroy()


def table2(out):
    dev, ter = terrain("nomadplains")
    stream = torch.cuda.ExternalStream(dev.stream(), device="cuda:0")
    rows = []
    for n in SIZES:
        o, d = grid_rays(n)
        qs, ql = Query(ter, o, d, RF.eye("F0"), "segments"), Query(ter, o, d, RF.eye("F0"), "lanes")
        ts, tl = pair(stream, qs, ql)
        dev.synchronize()
        same = bool(np.array_equal(qs.res.cpu().numpy().view(np.uint32), ql.res.cpu().numpy().view(np.uint32)))
        assert same, n
        rows.append({"n": n, "segments": summary(ts), "lanes": summary(tl)})
        print("n=%8d segments %.4f ms  lanes %.4f ms" % (n, rows[-1]["segments"]["ms"], rows[-1]["lanes"]["ms"]), flush=True)
    out["threshold"] = rows
    dev.destroy()


def throughput3(out):
    n = 1 << 20
    o, d = grid_rays(n)
    rows = {}
    for land in RF.LANDSCAPES:
        dev, ter = terrain(land)
        stream = torch.cuda.ExternalStream(dev.stream(), device="cuda:0")
        q = Query(ter, o, d, RF.eye("F0"), "auto")
        r = reps_for(stream, q)
        s = summary([timed(stream, q, r) for _ in range(REPEATS)])
        s["rays_per_s"] = n / (s["ms"] * 1e-3)
        st = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        assert ter.trace_rays_device(q.rays.data_ptr(), n, q.res.data_ptr(), st.data_ptr(), eye=RF.eye("F0"))
        dev.synchronize()
        s["steps_total"] = int(st.cpu().numpy().astype(np.int64).sum())
        s["steps_per_s"] = s["steps_total"] / (s["ms"] * 1e-3)
        s["hits"] = float((q.res.cpu().numpy()[:, 3] < 5000.0).mean())
        rows[land] = s
        print("%-12s n=2^20 %.3f ms  %.3e rays/s  %.3e steps/s" % (land, s["ms"], s["rays_per_s"], s["steps_per_s"]), flush=True)
        dev.destroy()
    out["throughput"] = rows


def util(out_dir):
    L = G.lib()
    L.rt_debug_query_util.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    n = 1 << 20
    o, d = grid_rays(n)
    perm = np.random.default_rng(20).permutation(n)
    dev, ter = terrain("nomadplains")
    stream = torch.cuda.ExternalStream(dev.stream(), device="cuda:0")
    # the grid in row order (neighbouring rays, alike in length, share a wave) and under a seeded permutation
    # (a wave's rays are as unlike as the query's)
    for order, (oo, dd) in (("grid", (o, d)), ("shuffled", (o[perm], d[perm]))):
        q = Query(ter, oo, dd, RF.eye("F0"), "lanes")
        r = reps_for(stream, q)
        s = summary([timed(stream, q, r) for _ in range(REPEATS)])
        buf = (C.c_ulonglong * 4)()  # (slots 2 and 3 stay 0: no normals)
        assert L.rt_debug_query_util(buf, 1) == 4
        q()
        dev.synchronize()
        assert L.rt_debug_query_util(buf, 1) == 4
        s.update({"variant": os.environ.get("RT_LIB_VARIANT", ""), "order": order, "wave_steps": int(buf[0]),
                  "lane_steps": int(buf[1]), "utilisation": buf[1] / (64.0 * buf[0])})
        print(json.dumps(s), flush=True)
        with open(os.path.join(out_dir, "ray_query_util.jsonl"), "a") as f:
            f.write(json.dumps(s) + "\n")
    dev.destroy()


def markdown(out, resources):
    b = out["bar1"]
    lines = ["# Ray queries: measurements (MI355X)", "",
             "`scripts/ray_query_bench.py bars`: the device form, HIP events around back-to-back launches of >= 50 ms "
             "a window, warm-up first, 5 alternating repeats per pair; ms are medians per call, the spread is "
             "(max - min) / median of a side's repeats.", "",
             "## 1. The 24,576 rays of 24 cameras: query against rt_terrain_prepass_batch", "",
             "| route | ms | spread |", "|---|---|---|",
             "| rt_terrain_prepass_batch, n = 24 (baseline) | %.4f | %.1f%% |" % (b["prepass_batch"]["ms"], 100 * b["prepass_batch"]["spread"]),
             "| query, auto | %.4f | %.1f%% |" % (b["query_auto"]["ms"], 100 * b["query_auto"]["spread"]),
             "| query, forced lanes | %.4f | %.1f%% |" % (b["query_lanes"]["ms"], 100 * b["query_lanes"]["spread"]), "",
             "Results equal the prepass's CameraResults bit for bit: %s.  Bar (auto no slower than the baseline beyond "
             "the spread, %.1f%%): **%s**.  Baseline rate: %.3e rays/s." % (
                 b["results_equal"], 100 * b["margin"], "met" if b["met"] else "MISSED", b["baseline_rays_per_s"]), "",
             "## 2. Both shapes by n (nomadplains, a near-square grid of n rays through F0's camera)", "",
             "| n | segments ms | lanes ms | faster |", "|---|---|---|---|"]
    for r in out["threshold"]:
        s, l = r["segments"]["ms"], r["lanes"]["ms"]
        lines.append("| %d | %.4f (%.1f%%) | %.4f (%.1f%%) | %s |" % (
            r["n"], s, 100 * r["segments"]["spread"], l, 100 * r["lanes"]["spread"], "segments" if s < l else "lanes"))
    lines += ["", "The auto rule (rt_rayquery.h kAutoSegmentsMax) sits at the crossing: segments up to 131,072 rays.",
              "", "## 3. Throughput at n = 2^20 (auto: the lane shape)", "",
              "| landscape | ms | rays/s | march steps/s | hits |", "|---|---|---|---|---|"]
    for land, s in out["throughput"].items():
        lines.append("| %s | %.3f | %.3e | %.3e | %.0f%% |" % (land, s["ms"], s["rays_per_s"], s["steps_per_s"], 100 * s["hits"]))
    np_rate = out["throughput"]["nomadplains"]["rays_per_s"]
    out["bar3_met"] = bool(np_rate >= b["baseline_rays_per_s"])
    lines += ["", "Bar (nomadplains at least the baseline's %.3e rays/s): **%s** (%.3e rays/s)." % (
        b["baseline_rays_per_s"], "met" if out["bar3_met"] else "MISSED", np_rate), ""]
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
                   if "k_query" in ln and "RayPolicy" in ln]
        out = {}
        bar1(out)
        table2(out)
        throughput3(out)
        md = markdown(out, res)
        with open(os.path.join(out_dir, "ray_query.json"), "w") as f:
            json.dump(out, f, indent=1)
        with open(os.path.join(out_dir, "ray_query.md"), "w") as f:
            f.write(md)
        print(md)
