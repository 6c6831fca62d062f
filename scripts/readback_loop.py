"""The per-frame-consumer loops, timed: C3 as bench.py's single_frame_serial companion configures it (1920x1080
nomadplains, 512-step cap, shadow + 1 AO ray) with a moving camera, one frame per call, on the plain device and
on RT_DEVICE_DEFERRED devices at 1 and 2 frames to a launch.

  L0  render + present, no consumer
  L1  render + present + a blocking rt_device_readback every frame (the per-frame consumer before the ring)
  L2  render + present + rt_readback_submit, then wait + release of ticket n-2 (a ring of depth 3)
  R1  the recording loop, synchronous recorder
  R2  the recording loop, rt_recorder_set_async(3)
  L2w, R2w (2 frames to a launch only)  L2 with a ring of 6 and ticket n-5, R2 with rt_recorder_set_async(6): at K
      frames to a launch a frame's trace is launched up to 2K-1 renders after its own, and the launch after it one
      more group later, so a consumer that lags fewer frames waits on a frame not launched yet (which launches it)
      or leaves the GPU nothing queued

5 warm-up and 40 timed frames per loop, the loops alternated in one process for three rounds; each timed window
ends with every frame delivered and a device synchronise.  Writes readback_ring.json and readback_ring.md into
--out (the recordings go to --out/_rec and are removed).
Usage: python scripts/readback_loop.py [--out profiles/r07] [--frames 40] [--rounds 3]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

os.environ["GPU_MAX_HW_QUEUES"] = os.environ.get("RT_BENCH_HW_QUEUES", "8")  # as bench.py, before HIP starts
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H, MAX_STEPS, AO, WARM = 1920, 1080, 512, 1, 5
KINDS = (("plain", 0), ("deferred_k1", 1), ("deferred_k2", 2))
LOOPS = ("L0", "L1", "L2", "R1", "R2")
WIDE = ("L2w", "R2w")  # deferred_k2 only
RING = {"L2": (3, 2), "L2w": (6, 5)}  # loop: (ring depth, frames the consumer lags)
ASYNC = {"R1": 0, "R2": 3, "R2w": 6}  # loop: rt_recorder_set_async depth


def loops_of(name):
    return LOOPS + (WIDE if name == "deferred_k2" else ())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r07")
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    import gpgpuraytrace_amd as G
    os.makedirs(os.path.join(a.out, "_rec"), exist_ok=True)
    n_all = WARM + a.frames
    base = G.Camera(W, H)
    euler = G.camera.INITIAL_ROTATION_EULER
    path = [G.Camera(W, H, position=base.position + i * 2.0 * np.asarray(base.front, float),
                     euler=(euler[0], euler[1] + 0.01 * i, euler[2])) for i in range(n_all)]

    def make(k, stats=False):
        dev = G.DeviceFactory.construct(G.DeviceAPI.HIP, W, H, stats=stats, deferred=k > 0)
        assert dev is not None, G.lib().rt_last_error()
        if k > 0:
            dev.defer_batch(k)
        ter = G.Terrain(dev, "nomadplains", max_steps=MAX_STEPS, ao_samples=AO)
        ter.create()
        assert ter.reload(), G.lib().rt_last_error()
        ter.set_camera(path[0])
        ter.set_time_of_day(0.3)
        return dev, ter

    # primary + shadow rays of the timed frames (an instrumented render of each camera, untimed)
    sdev, ster = make(0, stats=True)
    ps = 0
    for i, cam in enumerate(path):
        ster.set_camera(cam)
        ster.update_terrain()
        ster.render_device()
        hits = sdev.stats(reset=True)["hits"]
        if i >= WARM:
            ps += W * H + hits + 1024
    sdev.destroy()

    devs = {name: make(k) for name, k in KINDS}

    def run(name, loop, rnd):
        dev, ter = devs[name]
        ring = rec = None
        rec_path = os.path.join(a.out, "_rec", f"{name}_{loop}.rgb32")
        if loop in RING:
            ring = dev.readback_ring("rgba8", depth=RING[loop][0])
        if loop in ASYNC:
            rec = G.RecorderFactory.construct(dev, 25, True, rec_path, async_depth=ASYNC[loop])
            rec.start()
        tickets = []

        def frame(i):
            ter.set_camera(path[i])
            ter.update_terrain()
            ter.render_device()
            dev.present()
            if loop == "L1":
                dev.readback()
            elif ring:
                tickets.append(ring.submit())
                if len(tickets) > RING[loop][1]:
                    ring.wait(tickets[0])
                    ring.release(tickets.pop(0))

        def deliver():
            while tickets:
                ring.wait(tickets[0])
                ring.release(tickets.pop(0))
            if rec:
                assert rec.info()["frames"] > 0
            dev.synchronize()

        for i in range(WARM):
            frame(i)
        deliver()
        f0, p0 = dev.deferred_fused(), dev.prestream_renders()
        t0 = time.perf_counter()
        for i in range(WARM, n_all):
            frame(i)
        deliver()
        dt = time.perf_counter() - t0
        out = {"device": name, "loop": loop, "round": rnd, "ms_per_frame": dt / a.frames * 1e3,
               "primary_plus_shadow_mrays": ps / dt / 1e6, "deferred_fused": dev.deferred_fused() - f0,
               "prestream_renders": dev.prestream_renders() - p0}
        if rec:
            out["frames_recorded"] = rec.info()["frames"]
            rec.stop()
            rec.destroy()
            for p in (rec_path, rec_path + ".txt"):
                os.remove(p)
        if ring:
            ring.destroy()
        return out

    runs = []
    for rnd in range(a.rounds):
        for name, _ in KINDS:
            for loop in loops_of(name):
                runs.append(run(name, loop, rnd))
                print(json.dumps(runs[-1]), flush=True)

    # HIP-event times on the plain device: the snapshot (a submit between two events on the device stream) and
    # the D2H of one frame into pinned memory (the ring's copy, on a stream of its own)
    dev, ter = devs["plain"]
    ring = dev.readback_ring("rgba8", depth=1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    e1.record()  # (torch creates the HIP events at their first record)
    torch.cuda.synchronize()
    snap_ms, d2h_ms = [], []
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    pinned = torch.empty(W * H * 4, dtype=torch.uint8).pin_memory()
    fb = dev.framebuffer_pointer()
    side = torch.cuda.Stream()
    for _ in range(12):
        dev.record_event(e0.cuda_event)
        t = ring.submit()
        dev.record_event(e1.cuda_event)
        ring.wait(t)
        ring.release(t)
        dev.synchronize()
        snap_ms.append(e0.elapsed_time(e1))
        with torch.cuda.stream(side):
            e0.record(side)
            assert hip.hipMemcpyAsync(pinned.data_ptr(), fb, W * H * 4, 2, side.cuda_stream) == 0
            e1.record(side)
        side.synchronize()
        d2h_ms.append(e0.elapsed_time(e1))
    ring.destroy()
    for d, _ in devs.values():
        d.destroy()

    def med(name, loop, key):
        return statistics.median(r[key] for r in runs if r["device"] == name and r["loop"] == loop)

    table = {n: {lp: {"ms_per_frame": round(med(n, lp, "ms_per_frame"), 4),
                      "primary_plus_shadow_mrays": round(med(n, lp, "primary_plus_shadow_mrays"), 1),
                      "deferred_fused": int(med(n, lp, "deferred_fused")),
                      "prestream_renders": int(med(n, lp, "prestream_renders"))} for lp in loops_of(n)}
             for n, _ in KINDS}
    ratio = table["plain"]["L0"]["ms_per_frame"] / table["plain"]["L2"]["ms_per_frame"]
    bars = {"plain_L2_over_L0": round(ratio, 4), "plain_L2_at_least_0.95_L0": ratio >= 0.95,
            "plain_L2_over_L1": round(table["plain"]["L1"]["ms_per_frame"] / table["plain"]["L2"]["ms_per_frame"], 4)}
    for n in ("deferred_k1", "deferred_k2"):
        bars[n + "_L2_fused_equals_L0"] = table[n]["L2"]["deferred_fused"] == table[n]["L0"]["deferred_fused"]
    events = {"snapshot_ms_median": round(statistics.median(snap_ms[2:]), 4),
              "d2h_ms_median": round(statistics.median(d2h_ms[2:]), 4), "frame_bytes": W * H * 4}
    result = {"workload": f"C3 {W}x{H} nomadplains, {MAX_STEPS}-step cap, shadow + {AO} AO ray, moving camera",
              "frames": a.frames, "warmup": WARM, "rounds": a.rounds,
              "hip_hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"]), "table": table, "bars": bars, "events": events,
              "runs": runs}
    with open(os.path.join(a.out, "readback_ring.json"), "w") as f:
        json.dump(result, f, indent=1)
    lines = ["# Readback ring: the per-frame-consumer loops", "", result["workload"] + f"; {WARM} warm-up + {a.frames} "
             f"timed frames per loop, median of {a.rounds} alternated rounds (scripts/readback_loop.py).", "",
             "| device | loop | ms/frame | primary + shadow Mray/s | deferred_fused | prestream_renders |",
             "|---|---|---|---|---|---|"]
    for n, _ in KINDS:
        for lp in loops_of(n):
            r = table[n][lp]
            lines.append(f"| {n} | {lp} | {r['ms_per_frame']:.4f} | {r['primary_plus_shadow_mrays']:.1f} | "
                         f"{r['deferred_fused']} | {r['prestream_renders']} |")
    lines += ["", f"HIP events, plain device: snapshot (submit between two events on the device stream) "
              f"{events['snapshot_ms_median']} ms, D2H of one {W * H * 4} B frame into pinned memory "
              f"{events['d2h_ms_median']} ms.", "", "Bars:", ""]
    lines.append(f"- plain device, L2 >= 0.95 x L0: **{'met' if bars['plain_L2_at_least_0.95_L0'] else 'missed'}** "
                 f"(L2 runs at {bars['plain_L2_over_L0']:.3f} x L0; {bars['plain_L2_over_L1']:.3f} x L1)")
    for n in ("deferred_k1", "deferred_k2"):
        lines.append(f"- {n}, L2's deferred_fused equals L0's: **{'met' if bars[n + '_L2_fused_equals_L0'] else 'missed'}** "
                     f"({table[n]['L2']['deferred_fused']} against {table[n]['L0']['deferred_fused']})")
    with open(os.path.join(a.out, "readback_ring.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    os.rmdir(os.path.join(a.out, "_rec"))
    print(json.dumps({"bars": bars, "events": events}))


if __name__ == "__main__":
    main()
