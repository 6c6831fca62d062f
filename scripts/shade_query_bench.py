#!/usr/bin/env python3
"""Measurements of the shaded queries (rt_terrain_shade_rays_device) on the GPU: profiles/r11/shade_query.{md,json}.

    python3 scripts/shade_query_bench.py bars OUT_DIR [--resources FILE]
        time per query at n = 4,096 (the F0-F3 fixture rays), 65,536 (surface_query_bench.py's shifted rays) and
        2,073,600 nomadplains rays.  The largest is the pixel rays of the 1920x1080 reset-pose frame with ranges
        from that frame's own CellDistance, timed beside one rt_terrain_render of the same frame (AA 1, no AO) in
        the same process, the two sides alternating: the render is the yardstick.  Also the share of the query's
        pixels that equal the frame's (the rays are formed in numpy, so a few differ in the last bit of a
        direction), and the query's march iterations from its own step counts.
    RT_LIB_VARIANT=NAME python3 scripts/shade_query_bench.py util OUT_DIR
        a build with -DRT_QUERY_UTIL (make variant): lane utilisation of k_shadequery's march steps and of its
        shading visits for the largest query; appends one JSON line to OUT_DIR/shade_query_util.jsonl.

Timing as ray_query_bench.py: the device form on the device's stream, HIP events around back-to-back launches of
>= 50 ms a window, warm-up first, 5 repeats a pair with the two sides alternating."""
import json
import os
import sys

import ray_query_bench as RQ  # (applies RT_LIB_VARIANT, sets the paths)

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpgpuraytrace_amd as G  # noqa: E402
import ray_fixture as RF  # noqa: E402
import surface_query_bench as SQ  # noqa: E402

W, H = 1920, 1080
f32 = np.float32


class Shade:
    """A device-form shaded query with its buffers; rg: per-ray ranges or None."""

    def __init__(self, ter, o, d, eye, rg=None):
        self.ter, self.n, self.eye, self.ranged = ter, len(o), eye, rg is not None
        self.rays = torch.from_numpy(G.pack_rays(o, d, rg)).to("cuda:0")
        self.res = torch.zeros((self.n, 8), dtype=torch.float32, device="cuda:0")
        self.pix = torch.zeros(self.n, dtype=torch.int32, device="cuda:0")
        self.steps = torch.zeros((self.n, 2), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

    def __call__(self):
        ok = self.ter.shade_rays_device(self.rays.data_ptr(), self.n, self.res.data_ptr(), self.pix.data_ptr(),
                                        ray_range=self.ranged, eye=self.eye)
        assert ok, G.lib().rt_last_error()

    def iterations(self, dev):
        """(primary iterations, shadow iterations, hits) of the query, from its own step counts."""
        assert self.ter.shade_rays_device(self.rays.data_ptr(), self.n, self.res.data_ptr(), self.pix.data_ptr(),
                                          self.steps.data_ptr(), ray_range=self.ranged, eye=self.eye)
        dev.synchronize()
        st = self.steps.cpu().numpy().astype(np.int64)
        return int(st[:, 0].sum()), int(st[:, 1].sum()), int((self.res.cpu().numpy()[:, 7] > 0).sum())


def frame_terrain():
    """The 1920x1080 reset-pose frame of the benchmark: nomadplains, AA 1, no AO, time of day 0.3."""
    dev = G.DeviceFactory.construct(G.DeviceAPI.HIP, W, H, gpu=0)
    assert dev is not None, G.lib().rt_last_error()
    ter = G.Terrain(dev, "nomadplains")
    ter.create()
    assert ter.reload(), G.lib().rt_last_error()
    cam = G.Camera(W, H)
    ter.set_camera(cam)
    ter.set_time_of_day(0.3)
    ter.update_shaders()
    return dev, ter, cam


def pixel_rays(cam, cells):
    """getPixelRay (tracing.hlsl:124-134) for every pixel in float32 numpy, and tracescreen.hlsl's range per pixel:
    (CellDistance[cell].x, 5000).  Row-major over the frame."""
    m = cam.view_inverse_hlsl().astype(f32)
    proj = cam.projection_hlsl().astype(f32)
    eye = cam.eye()[:3].astype(f32)
    px, py = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    px, py = px.ravel(), py.ravel()
    sx = (((px + f32(0.5)) * (f32(1) / f32(W)) - f32(0.5)) * f32(2)) * proj[1, 1]
    sy = (((py + f32(0.5)) * (f32(1) / f32(H)) - f32(0.5)) * f32(2)) * proj[0, 0]
    o = (m[3, :3] + (m[2, :3] + (sy[:, None] * m[1, :3] + sx[:, None] * m[0, :3]))).astype(f32)
    d = (o - eye).astype(f32)
    cell = (np.floor(py / f32(H) * f32(32)) * f32(32) + np.floor(px / f32(W) * f32(32))).astype(np.int64)
    rg = np.stack([cells[cell, 0], np.full(len(cell), 5000, f32)], axis=1).astype(f32)
    return o, d, rg, eye


def device_cells(dev, ter):
    out = np.empty((1024, 2), np.float32)
    dev.synchronize()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data, ter.var_cell_distance.device_pointer(), out.nbytes, 2) == 0
    return out


def frame_query(dev, ter, cam):
    """The largest query: the frame's own pixel rays and ranges; also the frame's pixels for the comparison."""
    ter.render_device()
    dev.present()
    img8 = dev.readback().view(np.uint32).reshape(-1)
    o, d, rg, eye = pixel_rays(cam, device_cells(dev, ter))
    return Shade(ter, o, d, eye, rg), img8


def bars(out):
    dev, ter, cam = frame_terrain()
    stream = torch.cuda.ExternalStream(dev.stream(), device="cuda:0")
    rows = []
    fo, fd = RF.query(RF.F_SET)
    so, sd = SQ.shifted_rays(65536)
    big, img8 = frame_query(dev, ter, cam)
    queries = [("F0-F3 fixture rays", Shade(ter, fo, fd, RF.eye("F0"))), ("shifted F0 rays", Shade(ter, so, sd, RF.eye("F0"))),
               ("1920x1080 pixel rays, CellDistance ranges", big)]

    def render():
        ter.render_device()

    for what, q in queries:
        if q is big:
            tq, tr = RQ.pair(stream, q, render)
        else:
            tq, tr = [RQ.timed(stream, q, RQ.reps_for(stream, q)) for _ in range(RQ.REPEATS)], None
        prim, shad, hits = q.iterations(dev)
        s = RQ.summary(tq)
        s.update({"n": q.n, "rays": what, "primary_iterations": prim, "shadow_iterations": shad, "hits": hits,
                  "ns_per_iteration": s["ms"] * 1e6 / max(prim + shad, 1)})
        if tr is not None:
            s["render"] = RQ.summary(tr)
            s["ratio_to_render"] = s["ms"] / s["render"]["ms"]
            s["pixels_equal_to_frame"] = float(np.mean(q.pix.cpu().numpy().view(np.uint32) == img8))
        rows.append(s)
        print(json.dumps({k: v for k, v in s.items() if k != "runs_ms"}), flush=True)
    out["queries"] = rows
    dev.destroy()


def util(out_dir):
    L = G.lib()
    L.rt_debug_query_util.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    dev, ter, cam = frame_terrain()
    stream = torch.cuda.ExternalStream(dev.stream(), device="cuda:0")
    q, _ = frame_query(dev, ter, cam)
    s = RQ.summary([RQ.timed(stream, q, RQ.reps_for(stream, q)) for _ in range(RQ.REPEATS)])
    buf = (C.c_ulonglong * 4)()
    assert L.rt_debug_query_util(buf, 1) == 4
    q()
    dev.synchronize()
    assert L.rt_debug_query_util(buf, 1) == 4
    s.update({"variant": os.environ.get("RT_LIB_VARIANT", ""), "n": q.n, "wave_steps": int(buf[0]), "lane_steps": int(buf[1]),
              "shading_visits": int(buf[2]), "shading_lanes": int(buf[3]),
              "march_utilisation": buf[1] / (64.0 * max(buf[0], 1)),
              "shading_utilisation": buf[3] / (64.0 * max(buf[2], 1))})
    print(json.dumps(s), flush=True)
    with open(os.path.join(out_dir, "shade_query_util.jsonl"), "a") as f:
        f.write(json.dumps(s) + "\n")
    dev.destroy()


def markdown(out, resources):
    lines = ["# Shaded queries: measurements (MI355X)", "",
             "`scripts/shade_query_bench.py bars`: the device form (results and rgba8, no step counts), HIP events around "
             "back-to-back launches of >= 50 ms a window, warm-up first, 5 repeats; ms are medians per call, the spread "
             "is (max - min) / median of the repeats.  Nomadplains, time of day 0.3.  Iterations are the queries' own "
             "step counts (primary + shadow marches).", "",
             "| n | rays | ms | primary iterations | shadow iterations | hits | ns / iteration |", "|---|---|---|---|---|---|---|"]
    for s in out["queries"]:
        lines.append("| %d | %s | %.4f (%.1f%%) | %d | %d | %d | %.4f |" % (
            s["n"], s["rays"], s["ms"], 100 * s["spread"], s["primary_iterations"], s["shadow_iterations"], s["hits"],
            s["ns_per_iteration"]))
    big = out["queries"][-1]
    lines += ["", "## The largest query beside the frame it reproduces", "",
              "One `rt_terrain_render` of the same 1920x1080 frame (AA 1, no AO), alternating with the query in the same "
              "process: %.4f ms (%.1f%%).  The query takes %.4f ms: %.2f x the render.  %.4f%% of the query's pixels equal "
              "the frame's (its rays are formed in numpy)." % (
                  big["render"]["ms"], 100 * big["render"]["spread"], big["ms"], big["ratio_to_render"],
                  100 * big["pixels_equal_to_frame"]), ""]
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
            res = [ln.rstrip() for ln in open(sys.argv[sys.argv.index("--resources") + 1]) if "k_shadequery" in ln]
        out = {}
        bars(out)
        md = markdown(out, res)
        with open(os.path.join(out_dir, "shade_query.json"), "w") as f:
            json.dump(out, f, indent=1)
        with open(os.path.join(out_dir, "shade_query.md"), "w") as f:
            f.write(md)
        print(md)
