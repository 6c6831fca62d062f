"""GPU known-answer tests of the AO extension and the AA resolve against tests/hlsl_ref.py's float64 reading of
DESIGN.md section 9 and tracescreen.hlsl:63-75: the device's own ao_dir (rt_debug_math op 15), shade_points' AO
factor and step sum, and whole frames, through the restatement, the sets and the bounds of tests/test_ao_kat.py.
rt_shader.h's ao_dir / ao_factor and the oracle's were typed from the same paragraph, and every other GPU test compares
the two; a misreading they share fails here.

A frame is rebuilt sample by sample from the device's own queries: shade_rays gives each sample's colour and hit,
trace_surface its normal, op 15 the AO directions at the keys (x, y, a, k); the occlusion along them is
stage_ref.trace_ray's with hlsl_ref.ao_ray's arguments (the march itself is tests/test_gpu_march_kat.py's subject),
and hlsl_ref.resolve puts the pixel together."""
import numpy as np
import pytest

import hlsl_ref as H
import point_ref as PR
import ray_fixture as RF
import stage_ref as ST
import test_ao_kat as A
from test_gpu_parity import _device_cells, make
from test_gpu_shade_query import _make

pytestmark = pytest.mark.gpu

F_EYE = A.F_EYE
FRAME_LAND = "greenrocks"  # fog live, and the census of test_ao_kat.test_resolve_census


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _op15(dev, normals, keys):
    """rt_debug_math op 15: the device's ao_dir for normals (n, 3) and keys (n, 4) uint32."""
    import gpgpuraytrace_amd as G
    nr = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    keys = np.ascontiguousarray(keys, np.uint32).reshape(-1, 4)
    assert len(keys) == len(nr)
    out = np.empty((len(nr), 3), np.float32)
    assert G.lib().rt_debug_math(dev._h, 15, nr.ctypes.data, keys.ctypes.data, out.ctypes.data, len(nr)) == 0, \
        G.lib().rt_last_error()
    return out


def test_ao_dir_device():
    import gpgpuraytrace_amd as G
    dev = G.DeviceFactory.construct(G.DeviceAPI.HIP, 8, 8)
    normals, keys, _, _ = A.dir_inputs()
    got = _op15(dev, normals, keys)
    dev.check()
    dev.destroy()
    assert np.array_equal(_bits(got), _bits(A.oracle_dirs()))
    A.assert_directions(got)


def _own_dist(p):
    """The distance shade_points gives its AO rays' precision: |p - Eye| by the oracle's len3."""
    return PR.norm_len((np.asarray(p, np.float32) - F_EYE[None, :]).astype(np.float32))[:, 3].copy()


@pytest.mark.parametrize("land", ["nomadplains", "greenrocks"])
def test_shade_points_is_the_composition(land):
    """Camera F0's hits as the device finds them (shade_rays' positions, trace_surface's normals): shade_points'
    AO factor and AO step sum for K = 1, 4, 16 against the composition along the device's own directions."""
    o, d = RF.rays("F0")
    dev, ter = _make(land)
    shaded = ter.shade_rays(o, d, eye=F_EYE)
    surf = ter.trace_surface(o, d, eye=F_EYE)
    assert shaded is not None and surf is not None
    hit = np.flatnonzero(shaded[:, 7] > 0)
    assert len(hit) >= 512
    p, nrm = np.ascontiguousarray(shaded[hit, 4:7]), np.ascontiguousarray(surf[hit, 4:7])
    dist = _own_dist(p)
    for samples in A.AO_COUNTS:
        got = ter.shade_points(p, nrm, eye=F_EYE, ao_samples=samples, seed=A.SEED, steps=True)
        assert got is not None
        res, st = got
        occ, steps = A.compose(land, p, nrm, dist, lambda k: A.point_keys(len(p), A.SEED, k), samples,
                               dirs=lambda nr, keys: _op15(dev, nr, keys))
        err = np.abs(res[:, 3].astype(np.float64) - H.ao_factor(occ, samples)).max()
        print(land, samples, "factor %.3g" % err, np.bincount(occ, minlength=samples + 1))
        assert np.array_equal(A.decode_occ(res[:, 3], samples), occ)
        assert err <= A.FACTOR_BOUND
        assert np.array_equal(st[:, 1].astype(np.int64), steps)
    dev.check()
    dev.destroy()


class _Frame:
    """A rendered frame of test_ao_kat's camera and what the device's queries say of its samples."""

    def __init__(self, land, aa, ao, float_output=True):
        self.land, self.aa, self.ao = land, aa, ao
        self.dev, self.ter = dev, ter = make(A.frame_consts(), land, aa=aa, ao=ao, float_output=float_output)
        ter.render_device()
        dev.present()
        self.img = dev.readback_float() if float_output else None
        self.img8 = dev.readback()
        p, d, rg, self.keys = A.sample_rays(aa, _device_cells(ter))
        res = ter.shade_rays(p, d, ranges=rg, eye=F_EYE, max_steps=ter.max_steps)
        surf = ter.trace_surface(p, d, ranges=rg, eye=F_EYE, max_steps=ter.max_steps)
        assert res is not None and surf is not None
        assert np.array_equal(_bits(res[:, 4:8]), _bits(np.concatenate([surf[:, :3], surf[:, 7:8]], axis=1)))
        self.colours, self.hit = res[:, :3], res[:, 7] > 0
        self.rows = np.flatnonzero(self.hit)
        self.p, self.normals = np.ascontiguousarray(res[self.rows, 4:7]), np.ascontiguousarray(surf[self.rows, 4:7])
        self.dist = np.ascontiguousarray(res[self.rows, 3])

    def keys_of(self, k):
        return np.concatenate([self.keys[self.rows], np.full((len(self.rows), 1), k, np.uint32)], axis=1)

    def occluded(self, dist=None):
        """The hits' counts of occluded AO rays along the device's directions at the keys (x, y, a, k)."""
        occ, _ = A.compose(self.land, self.p, self.normals, self.dist if dist is None else dist, self.keys_of, self.ao,
                           dirs=lambda nr, keys: _op15(self.dev, nr, keys))
        return occ

    def restated(self):
        factors = np.ones(len(self.hit))
        if self.ao:
            factors[self.rows] = H.ao_factor(self.occluded(), self.ao)
        return A.restate_pixels(self.aa, self.ao, self.colours, factors, self.hit)

    def close(self):
        self.dev.check()
        self.dev.destroy()


@pytest.mark.parametrize("aa,ao", A.RESOLVE_CASES)
def test_frames(aa, ao):
    f = _Frame(FRAME_LAND, aa, ao)
    ref = f.restated()
    f.close()
    over_hit, over_miss = A.resolve_census(f.colours, f.hit)
    assert over_hit >= 8 and over_miss >= 8
    A.assert_resolved(aa, ref, f.img, f.img8)


def test_key_convention():
    """The (1, 4) frame: shade_points for row y with seed = y and point i = pixel x = i's hit has the key
    (i, seed, 0, k) = the frame's (x, y, 0, k).  Its ao is the composition's factor for that pixel bit for bit, and
    where its own distance gives the AO rays the frame's precision, ao times the saturated colour is the pixel.
    (shade_points takes |p - Eye| for the distance, the frame the march's rr.pd.w; the precision is 8 for both below
    a distance of about 134, which two thirds of nomadplains' hits are and none of greenrocks'.)"""
    f = _Frame("nomadplains", 1, 4)
    own = _own_dist(f.p)
    want = np.zeros(len(f.hit), np.float32)
    want[f.rows] = H.ao_factor(f.occluded(own), 4).astype(np.float32)
    same_precision = np.zeros(len(f.hit), bool)
    same_precision[f.rows] = _bits(ST.shadow_precision(own)) == _bits(ST.shadow_precision(f.dist))
    points, normals = np.zeros((len(f.hit), 3), np.float32), np.zeros((len(f.hit), 3), np.float32)
    points[:], normals[:] = f.p[0], f.normals[0]  # a miss gets any point; its answer is not read
    points[f.rows], normals[f.rows] = f.p, f.normals
    got = np.zeros(len(f.hit), np.float32)
    for y in range(A.FRAME):
        row = slice(y * A.FRAME, (y + 1) * A.FRAME)
        assert np.array_equal(f.keys[row, 0], np.arange(A.FRAME)) and (f.keys[row, 1] == y).all()
        res = f.ter.shade_points(points[row], normals[row], eye=F_EYE, ao_samples=4, seed=y)
        assert res is not None
        got[row] = res[:, 3]
    f.close()
    assert np.array_equal(_bits(got[f.hit]), _bits(want[f.hit]))
    assert (want[f.hit] < 1).sum() >= 64
    live = f.hit & same_precision
    assert live.sum() >= 256
    sat = np.clip(f.colours, np.float32(0), np.float32(1))
    pixel = (sat * got[:, None]).astype(np.float32)
    assert np.array_equal(_bits(pixel[live]), _bits(f.img.reshape(-1, 4)[live, :3]))


@pytest.mark.parametrize("aa,ao", [(1, 4), (4, 1)])
def test_rgba8_only_device(aa, ao):
    """The paths that finish hit pixels inside k_trace: the codes under the same tie rule."""
    f = _Frame(FRAME_LAND, aa, ao, float_output=False)
    ref = f.restated()
    f.close()
    _, wrong8, ties = A.resolve_check(aa, ref, None, f.img8)
    print("A %d K %d: %d wrong codes, ties %.4f" % (aa, ao, wrong8, ties))
    assert wrong8 == 0
    assert ties < A.MAX_TIES
