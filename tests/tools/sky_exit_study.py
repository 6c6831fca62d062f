#!/usr/bin/env python3
"""Diagnostic: how much of the primary march k_trace's sky exit leaves out (tests/tools/sky_exit_study.c), counted
on the CPU with the oracle at a BASELINE config.

Renders every --row-step-th row with the oracle instrumented per primary march sample and counts the steps, and
their noise3d calls, of rays that miss, of the steps the exit skips (the ray does not descend and the sample lies
above the ceiling: from the first such sample every later one is, rt_shader.h sky_exit), and what a ceiling per
octave count (the bound with the octave weights' prefix sum up to the sample's count) would skip.

  python tests/tools/sky_exit_study.py [--config c3] [--row-step 36] [--ceil 256]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402

SO = os.path.join(ROOT, "tests", "tools", "_build", "libsky_exit_study.so")
NOISE_BOUND = 1.05


def build():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(ROOT, "tests", "tools", "sky_exit_study.c")
    subprocess.run(["gcc", "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fopenmp",
                    "-shared", "-o", SO, src, "-lm"], check=True)


def ceilings():
    """ceiling[n] for octave counts n = 0..17: pow(35 (1 + 30 B P_n), 0.78) (1 + 1e-3), P_n the prefix sum."""
    rcp = np.array([0.0] + [1.0 / np.float32(1.96 ** n) for n in range(1, 18)], np.float64)
    expo = float(np.float32(0.68) + np.float32(0.1))
    return (35.0 * (1.0 + 30.0 * NOISE_BOUND * np.cumsum(rcp))) ** expo * (1.0 + 1e-3)


def ray_dir_y(c, W, H):
    M = np.asarray(c["view_inverse"], np.float64).reshape(4, 4)
    P = np.asarray(c["projection"], np.float64).reshape(4, 4)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    sx = ((px + 0.5) / W - 0.5) * 2.0 * P[1, 1]
    sy = ((py + 0.5) / H - 0.5) * 2.0 * P[0, 0]
    return sx * M[0, 1] + sy * M[1, 1] + M[2, 1] + M[3, 1] - float(c["eye"][1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--row-step", type=int, default=36)
    ap.add_argument("--ceil", type=float, default=256.0)
    ap.add_argument("--pose", default="reset")
    a = ap.parse_args()
    import gpgpuraytrace_amd as G
    W, H, ms, ao = {"c2": (1280, 720, 256, 0), "c3": (1920, 1080, 512, 1), "c5": (3840, 2160, 1024, 4),
                    "ref": (1920, 1080, 0, 0)}[a.config]
    build()
    L = C.CDLL(SO)
    L.st_config.argtypes = [C.c_int64]
    L.st_pixel_len.argtypes = [C.c_int64]
    L.st_pixel_len.restype = C.c_int64
    L.st_pixel_data.argtypes = [C.c_int64]
    L.st_pixel_data.restype = C.c_void_p
    fp = C.POINTER(C.c_float)
    L.ro_noise_generate.argtypes = [C.POINTER(O.Noise), C.c_uint32, C.c_int]
    L.ro_camerarays.argtypes = [C.POINTER(O.Noise), C.POINTER(O.Frame), fp, C.POINTER(O.Stats)]
    L.ro_set_target_depths.argtypes = [fp, fp]
    L.ro_tracescreen.argtypes = [C.POINTER(O.Noise), C.POINTER(O.Frame), fp, fp, C.POINTER(C.c_uint8), fp,
                                 C.POINTER(O.Stats)]
    nz = O.Noise()
    L.ro_noise_generate(C.byref(nz), 300, O.RAND_MSVC)
    euler = G.camera.INITIAL_ROTATION_EULER if a.pose == "reset" else G.camera.LOOKDOWN_ROTATION_EULER
    consts = G.frame_constants(W, H, euler=euler)
    L.st_config(W * H)
    cr = np.zeros(4096, np.float32)
    cd = np.zeros(2048, np.float32)
    fr = O.make_frame(consts, landscape=0, max_steps=ms, ao=0, rows=(0, 0, 1))
    L.ro_camerarays(C.byref(nz), C.byref(fr), cr.ctypes.data_as(fp), None)
    L.ro_set_target_depths(cr.ctypes.data_as(fp), cd.ctypes.data_as(fp))
    rgba = np.zeros((H, W, 4), np.float32)
    fr = O.make_frame(consts, landscape=0, max_steps=ms, ao=0, rows=(0, H, a.row_step))
    L.ro_tracescreen(C.byref(nz), C.byref(fr), cd.ctypes.data_as(fp), rgba.ctypes.data_as(fp), None, None, None)

    diry = ray_dir_y(consts, W, H)
    ceil_n = ceilings()
    print(f"ceiling {ceil_n[17]:.2f} for 17 octaves, {ceil_n[2]:.2f} for 2; the kernel's literal {a.ceil}")
    tot = {k: 0 for k in ("rays", "steps", "noise", "miss_steps", "skip_steps", "skip_noise", "skip_rays",
                          "oct_steps", "oct_noise", "y200", "y150")}
    for y in range(0, H, a.row_step):
        for x in range(W):
            i = y * W + x
            n = L.st_pixel_len(i)
            if n == 0:
                continue
            s = np.ctypeslib.as_array(C.cast(L.st_pixel_data(i), fp), (n,)).reshape(-1, 3)
            tot["rays"] += 1
            tot["steps"] += len(s)
            tot["noise"] += int(s[:, 2].sum())
            if not s[-1, 1] > 0:
                tot["miss_steps"] += len(s)
            tot["y200"] += int((s[:, 0] > 200).sum())
            tot["y150"] += int((s[:, 0] > 150).sum())
            if diry[y, x] >= 0:
                above = np.nonzero(s[:, 0] > a.ceil)[0]
                if above.size:
                    k = above[0]
                    assert (s[k:, 0] > a.ceil).all() and not (s[k:, 1] > 0).any()  # monotone, never a hit again
                    tot["skip_rays"] += 1
                    tot["skip_steps"] += len(s) - k
                    tot["skip_noise"] += int(s[k:, 2].sum())
                above = np.nonzero(s[:, 0] > ceil_n[(s[:, 2] - 1).astype(int)])[0]
                if above.size:
                    k = above[0]
                    assert not (s[k:, 1] > 0).any()
                    tot["oct_steps"] += len(s) - k
                    tot["oct_noise"] += int(s[k:, 2].sum())
    st, nn = max(1, tot["steps"]), max(1, tot["noise"])
    print(f"{a.config} {a.pose}, rows 0::{a.row_step}: {tot['rays']} primary rays")
    print(f"primary march steps            {tot['steps']:>12}")
    print(f"  of rays that miss            {tot['miss_steps']:>12}  {100.0 * tot['miss_steps'] / st:5.1f}%")
    print(f"  skipped by the exit          {tot['skip_steps']:>12}  {100.0 * tot['skip_steps'] / st:5.1f}%"
          f"  ({tot['skip_rays']} rays)")
    print(f"  with a ceiling per octaves   {tot['oct_steps']:>12}  {100.0 * tot['oct_steps'] / st:5.1f}%")
    print(f"  samples above y 200 / 150    {tot['y200']:>12}  {100.0 * tot['y200'] / st:5.1f}% / "
          f"{100.0 * tot['y150'] / st:5.1f}%")
    print(f"noise3d calls of the march     {tot['noise']:>12}")
    print(f"  in the skipped steps         {tot['skip_noise']:>12}  {100.0 * tot['skip_noise'] / nn:5.1f}%"
          f"  ({tot['skip_noise'] / max(1, tot['skip_steps']) - 1:.2f} octaves a step)")
    print(f"  with a ceiling per octaves   {tot['oct_noise']:>12}  {100.0 * tot['oct_noise'] / nn:5.1f}%")


if __name__ == "__main__":
    main()
