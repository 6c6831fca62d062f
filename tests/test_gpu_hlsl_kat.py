"""GPU known-answer tests against tests/hlsl_ref.py, the float64 restatement of the HLSL: the device's noise3d,
getDensity, getNormal and shaded colours on the point sets and within the bounds of tests/test_hlsl_kat.py (the
device repeats the oracle's bits at these inputs, so it makes exactly the oracle's error).  What the other GPU
tests cannot see -- a misreading of the HLSL shared by rt_shader.h and the oracle -- fails here."""
import numpy as np
import pytest

import golden_index as GI
import hlsl_ref as H
import ray_fixture as RF
import shade_ref as SH
import test_hlsl_kat as K
from test_gpu_parity import FixedCamera, make

pytestmark = pytest.mark.gpu


def _debug_noise(ter, p, mode):
    import gpgpuraytrace_amd as G
    p = np.ascontiguousarray(p, np.float32)
    out = np.empty(len(p), np.float32)
    assert G.lib().rt_debug_noise(ter.compute._h, p.ctypes.data, out.ctypes.data, len(p), mode) == 0
    return out


def test_noise3d_device():
    dev, ter = make(GI.consts(64, 48, "reset"))
    got = _debug_noise(ter, K.noise_points(), 0)
    dev.destroy()
    assert K.worst_noise(got) <= K.bound("noise3d")


@pytest.mark.parametrize("land", K.LANDS)
def test_density_device(land):
    """Both eyes of the CPU test: the golden reset pose's (0, 100, 0), then (13, 92, -9.5) set as the camera's."""
    consts = dict(GI.consts(64, 48, "reset"))
    assert tuple(consts["eye"][:3]) == K.EYES[0]
    dev, ter = make(consts, land=land)
    got = [_debug_noise(ter, K.density_points(), 1)]
    consts["eye"] = np.array(list(K.EYES[1]) + [consts["eye"][3]], np.float32)
    ter.set_camera(FixedCamera(consts))
    ter.update_terrain()  # writes the Eye variables
    got.append(_debug_noise(ter, K.density_points(), 1))
    dev.destroy()
    if land == "nomadplains":  # the only density that reads Eye
        assert not np.array_equal(got[0], got[1])
    for eye, g in zip(K.EYES, got):
        assert K.worst_density(land, eye, g) <= K.bound("density", land), eye


@pytest.mark.parametrize("land", K.LANDS)
def test_normals_and_colours_device(land):
    """The 4096 fixture rays through the surface query and the shaded query.  Normals: the restatement fed with
    the device's own pos and density.  Colours: traceSample's composite fed with the device's pos, density, pd.w
    and normal, and the checker's shadow class and fcolord (march outputs, which test_parity_with_the_checker
    holds the device to bit for bit)."""
    o, d = RF.query(RF.F_SET)
    consts = dict(GI.consts(64, 48, "reset"))
    consts["sun"] = SH.SUN
    dev, ter = make(consts, land, float_output=False)
    surf = ter.trace_surface(o, d, eye=K.F_EYE)
    got = ter.shade_rays(o, d, eye=K.F_EYE, rgba8=True)
    dev.check()
    dev.destroy()
    assert surf is not None and got is not None
    res, px = got
    pd, dens = res[:, [4, 5, 6, 3]], res[:, 7]
    assert np.array_equal(surf[:, :4].view(np.uint32), pd.view(np.uint32))  # the two queries' positions
    assert np.array_equal(surf[:, 7].view(np.uint32), dens.view(np.uint32))
    s = K.shaded(land)
    assert np.array_equal(np.flatnonzero(dens > 0), s.hit)
    h = s.hit
    assert K.worst_normal(land, surf[h, :3], surf[h, 7], surf[h, 4:7]) <= K.bound("normal", land)
    hit, miss, ref, keep = K.composite(s, pd, dens, surf[:, 4:7], res[:, :3])
    assert hit <= K.bound("composite", land)
    assert miss <= K.bound("miss", land)
    codes = np.stack([(px >> sh) & 0xFF for sh in (0, 8, 16)], axis=1).astype(np.int64)
    assert np.abs(codes - H.unorm8(ref))[keep].max() <= 1
    assert np.all(px >> 24 == 0xFF)
