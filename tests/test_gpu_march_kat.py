"""GPU known-answer tests of the march against hlsl_ref.march, the float64 restatement of traceRay
(tracing.hlsl:47-105): the device's own trajectory -- the surface query capped at max_steps = 1..64 -- through the
restatement, the sets, the bounds and the census of tests/test_march_kat.py.  rt_shader.h's march_begin and
march_step_with were written from the same reading of the loop as the oracle's trace_ray, and every other GPU test
compares the two; a misreading they share fails here.  The fog accumulation, which the surface query does not
report, is seen through the shaded query's miss colour."""
import numpy as np
import pytest

import golden_index as GI
import shade_ref as SH
import test_hlsl_kat as K
import test_march_kat as M
from test_gpu_parity import make

pytestmark = pytest.mark.gpu


def _surface_trajectory(ter, case):
    rg = np.stack([case.dist0, case.enddist], axis=1)

    def run(k):
        got = ter.trace_surface(case.p, case.dir, ranges=rg, eye=K.F_EYE, max_steps=k, steps=True)
        assert got is not None
        res, st = got
        return res[:, :4].copy(), res[:, 7].copy(), st, None
    return M.observe(run)


def _assert_march(case, t):
    M.check_prefix(t)
    M.assert_within(case, t)
    M.assert_density(case, t)


@pytest.mark.parametrize("land", K.LANDS)
def test_primary_march_device(land):
    """Sets near and far, 64 capped launches of 256 rays each."""
    near, far = (M.primary(land, which, calcfog=False) for which in ("near", "far"))
    dev, ter = make(GI.consts(64, 48, "reset"), land)
    tn, tf = _surface_trajectory(ter, near), _surface_trajectory(ter, far)
    dev.check()
    dev.destroy()
    _assert_march(near, tn)
    _assert_march(far, tf)
    M.census(land, tn, tf)


def test_primary_march_device_recording():
    case = M.primary("nomadplains", "near", recording=1)
    dev, ter = make(GI.consts(64, 48, "reset"), "nomadplains", recording=True)
    t = _surface_trajectory(ter, case)
    dev.check()
    dev.destroy()
    _assert_march(case, t)
    plain = M.oracle_trajectory(M.shapes("nomadplains")["primary near"])
    assert not np.array_equal(t.pd, plain.pd)  # the RECORDING constants walk other steps


def test_fog_accumulation_device():
    """greenrocks, far set: the shaded query capped at k is a miss wherever the k-th density is <= 0, and its
    colour is lerp(lerp(sky, f.rgb, f.w), sky, skyAmount) with the march's f; the restated f is teacher-forced on
    the device's own densities from the surface query, whose positions the shaded query repeats bit for bit."""
    case = M.shapes("greenrocks")["primary far fog"]
    rg = np.stack([case.dist0, case.enddist], axis=1)
    consts = dict(GI.consts(64, 48, "reset"))
    consts["sun"] = SH.SUN
    dev, ter = make(consts, "greenrocks", float_output=False)
    t = _surface_trajectory(ter, case)
    shaded = []
    for k in range(1, M.STEPS + 1):
        res = ter.shade_rays(case.p, case.dir, ranges=rg, eye=K.F_EYE, max_steps=k)
        assert res is not None
        shaded.append(res)
    dev.check()
    dev.destroy()
    worst, live = M.fog_colour_check(t, shaded)
    print("fog colour %.3g, %d rows with f.w > 1e-3" % (worst, live))
    assert live >= 1000
    assert worst <= M.fog_colour_bound()
