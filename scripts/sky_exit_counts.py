#!/usr/bin/env python3
"""What the sky exit (rt_variants.h RT_SKY_EXIT) leaves out of the bench frame: the instrumented (STATS)
kernels' primary march steps and noise3d calls of one C3 frame (1920x1080, reset pose, 512-step cap, 1 AO ray).

The product's STATS kernels march every ray out, so the default build prints the oracle's counts.  A diagnostic
build whose STATS kernels take the exit too prints what the product kernel executes:

    make -C gpgpuraytrace_amd/csrc variant NAME=skystats FLAGS="-DRT_SKY_EXIT_STATS=1"
    python3 scripts/sky_exit_counts.py                       # all steps
    RT_LIB_VARIANT=skystats python3 scripts/sky_exit_counts.py   # executed steps

The difference is the skipped share; the roofline fraction bench.py --full reports (built from the STATS noise
count) scales by executed / all noise calls."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import with_variant  # noqa: E402

with_variant.apply()
import gpgpuraytrace_amd as G  # noqa: E402

W, H = 1920, 1080
dev = G.DeviceFactory.construct(G.DeviceAPI.HIP, W, H, gpu=0, stats=True)
ter = G.Terrain(dev, "nomadplains", max_steps=512, ao_samples=1)
ter.create()
assert ter.reload()
ter.set_camera(G.Camera(W, H))
ter.set_time_of_day(0.3)
ter.update_shaders()
ter.camera_compute.run(2, 2, 1)
dev.synchronize()
pre = dev.stats(reset=True)
ter.render_device()
dev.synchronize()
st = dev.stats(reset=True)
out = {"variant": os.environ.get("RT_LIB_VARIANT", "") or "default"}
for key in ("primary_steps", "shadow_steps", "ao_steps", "hits", "noise_calls"):
    if key in st:
        out[key] = int(st[key]) - (int(pre.get(key, 0)) if key == "noise_calls" else 0)
out["prepass_noise_calls"] = int(pre.get("noise_calls", 0))
print(json.dumps(out))
dev.destroy()
