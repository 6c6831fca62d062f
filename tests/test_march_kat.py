"""Known-answer tests of the oracle's march (trace_ray) against hlsl_ref.march, the float64 restatement of traceRay
(tracing.hlsl:47-105), step by step.  The GPU tests hold every kernel to oracle/rt_oracle.c bit for bit, and
rt_shader.h's march_begin / march_step_with were written from the same reading of the loop as the oracle's
trace_ray; a misreading the two share (a constant, `dist -= lastStep`, the order of `step *= F` and
`lastStep = step * stepmult`, the fog refund of a hit, `dir /= dirLength`, which state rr.pd reports) fails here,
and in tests/test_gpu_march_kat.py for the device.

A float64 march left to itself cannot be compared with a float32 one: one density whose sign differs in the last
bits sends the ray onto another step count (profiles/r03/parity_sensitivity.md).  So the restatement is
TEACHER-FORCED: it decides no branch and computes no density that steers one.  A run capped at max_steps = k returns
the state after exactly k iterations (rr.pd.xyz the k-th sample, rr.pd.w the distance after the k-th update,
rr.density the k-th density), so the runs k = 1..STEPS are the trajectory; the restatement reads each step's density
from it, takes its sign for the branch and its value for stepmult, and restates the loop's own arithmetic.  The
density of every sample is checked on its own against hlsl_ref.density at the observed position.

Sets (256 rays a landscape: every 16th of the F0-F3 fixture rays, eye F0, the second half's dir scaled by 2.5 so
that dirLength in the first step is told from the normalised position):
    near   t_min = max(0.01, 0.97 * the full march's hit distance), 4000 for a miss, t_max 5000: refinement, the
           end by `step <= RAY_MIN_LIMIT`, the end by enddist
    far    0.01 .. 5000, the first STEPS steps: stepmult on d < -5
Shapes: primary (stepmod 1, refining; fog on greenrocks, and greenrocks without it once more), prepass (far set,
stepmod 2, skiprefine: camerarays.hlsl:18), shadow (from the near set's final hits towards shade_ref.SUN, 0.4 .. 100,
fog, skiprefine, stepmod = hlsl_ref.shadow_ray's precision; every landscape's color.hlsl casts one), and nomadplains
primary once more with RECORDING.

MEASURED holds the oracle's worst difference from the restatement over these sets and shapes; every bound is twice
that, rounded up to one significant digit (test_hlsl_kat.bound's rule).  Position is relative to max(1, |p|inf),
dist to max(1, |dist|), density by test_hlsl_kat.density_error, fcolord absolute per component over every step,
precision (the shadow ray's stepmod, color.hlsl:47-50) relative.  nomadplains' dist figure is one ray whose first
step of 15.5 (dirLength 154) lands inside the terrain: `dist -= lastStep` cancels to 0.01.  The density at the march's
samples of testing differs by more than test_hlsl_kat's own point set shows, hence a figure of its own here.

    quantity   nomadplains       testing           simple            greenrocks
    position   4.37e-07 / 9e-07  4.81e-07 / 1e-06  4.73e-07 / 1e-06  4.28e-07 / 9e-07
    dist       2.65e-06 / 6e-06  2.49e-07 / 5e-07  2.95e-07 / 6e-07  2.54e-07 / 6e-07
    density    6.66e-06 / 2e-05  4.67e-05 / 1e-04  1.47e-05 / 3e-05  5.63e-05 / 2e-04
    fcolord    0 / 0             0 / 0             0 / 0             1.30e-07 / 3e-07
    precision  2.96e-07 / 6e-07  2.95e-07 / 6e-07  2.98e-07 / 6e-07  2.58e-07 / 6e-07
(measured worst / bound.)  Termination is exact: the restated loop condition holds before every step that ran and
fails after the last step of every ray that ended before STEPS, rows within hlsl_ref.TIE_BAND of a tie left out
(at most 0.5 % of them).

The mutation check runs every hlsl_ref.mutants("march") entry -- each literal with its last printed digit changed by
one, and the structural misreadings of hlsl_ref.MARCH_STRUCTURES -- and requires it to leave a bound or to break
the termination check on the shapes that read it; ESCAPES lists those that stay inside, with the reason.
"""
import numpy as np
import pytest

import hlsl_ref as H
import ray_fixture as RF
import shade_ref as SH
import stage_ref as ST
import surface_ref as SR
import test_hlsl_kat as K

LANDS = K.LANDS
F_EYE = K.F_EYE
STEPS = 64
NEAR_FACTOR, MISS_START = 0.97, 4000.0
QUANTITIES = ("position", "dist", "density", "fcolord", "precision")

# The oracle's worst difference from the restatement, measured with this module's own sets (columns as LANDS).
MEASURED = {
    "position": (4.37e-07, 4.81e-07, 4.73e-07, 4.28e-07),
    "dist": (2.65e-06, 2.49e-07, 2.95e-07, 2.54e-07),
    "density": (6.66e-06, 4.67e-05, 1.47e-05, 5.63e-05),
    "fcolord": (0.00e+00, 0.00e+00, 0.00e+00, 1.30e-07),
    "precision": (2.96e-07, 2.95e-07, 2.98e-07, 2.58e-07),
}


def bound(quantity, land):
    """Twice the measured worst, rounded up to one significant digit."""
    return K.twice_rounded_up(MEASURED[quantity][LANDS.index(land)])


# --- the sets ------------------------------------------------------------------------------------------
def rays():
    """(origins, dirs) (256, 3) float32: every 16th F0-F3 ray, the second half's dir scaled by 2.5."""
    def make():
        o, d = RF.query(RF.F_SET)
        o, d = o[::16].copy(), d[::16].copy()
        d[len(d) // 2:] *= np.float32(2.5)
        return o, d
    return K.cached(("march rays",), make)


def full_march(land):
    """(pd (n, 4), density (n,)) of the whole refined march of rays() over 0.01 .. 5000."""
    def make():
        o, d = rays()
        res, _ = SR.trace(o, d, F_EYE, land)
        return res[:, :4].copy(), res[:, 7].copy()
    return K.cached(("march full", land), make)


def ranges(land, which):
    o, _ = rays()
    rg = np.empty((len(o), 2), np.float32)
    rg[:, 0], rg[:, 1] = SR.T_MIN, SR.T_MAX
    if which == "near":
        pd, dens = full_march(land)
        rg[:, 0] = np.where(dens > 0, np.maximum(np.float32(0.01), np.float32(NEAR_FACTOR) * pd[:, 3]),
                            np.float32(MISS_START))
    return rg


class Case:
    """One call of traceRay for n rays: its arguments, and the frame's."""

    def __init__(self, land, name, p, dir, dist0, enddist, stepmod, calcfog, skiprefine, recording=0):
        n = len(p)
        self.land, self.name, self.p, self.dir = land, name, p, dir
        self.dist0, self.enddist, self.stepmod = (np.broadcast_to(np.asarray(v, np.float32).reshape(-1), (n,)).copy()
                                                  for v in (dist0, enddist, stepmod))
        self.calcfog, self.skiprefine, self.recording = bool(calcfog), bool(skiprefine), int(recording)

    def oracle(self, max_steps):
        return ST.trace_ray(self.land, self.p, self.dist0, self.enddist, self.stepmod, self.dir, F_EYE, self.calcfog,
                            self.skiprefine, max_steps, self.recording)


def primary(land, which, calcfog=None, recording=0):
    o, d = rays()
    rg = ranges(land, which)
    fog = (land == "greenrocks") if calcfog is None else calcfog
    return Case(land, "primary %s%s%s" % (which, " fog" if fog else "", " recording" if recording else ""), o, d,
                rg[:, 0], rg[:, 1], 1.0, fog, False, recording)


def prepass(land):
    o, d = rays()
    return Case(land, "prepass", o, d, SR.T_MIN, SR.T_MAX, 2.0, False, True)  # camerarays.hlsl:18


def near_hits(land):
    """(rows, pd (m, 4)) of the near set's rays that end on the surface: where getColor casts its shadow ray."""
    def make():
        pd, _, dens, _ = primary(land, "near").oracle(0)
        rows = np.flatnonzero(dens > 0)
        return rows, pd[rows]
    return K.cached(("march near hits", land), make)


def shadow(land, tweak=None):
    """getColor's shadow ray from the near set's hits.  Start and length are the restatement's; the stepmod is the
    oracle's own `precision`, which test_shadow_precision holds to the restated one (a float64 precision rounded
    to float32 is not the oracle's to the last bit, and another last bit of stepmod is another march)."""
    _, pd = near_hits(land)
    dist0, enddist, _ = H.shadow_ray(land, pd[:, 3], tweak)
    return Case(land, "shadow", pd[:, :3].copy(), np.tile(SH.SUN, (len(pd), 1)), dist0, enddist,
                ST.shadow_precision(pd[:, 3]), True, True)


def worst_precision(land, tweak=None):
    _, pd = near_hits(land)
    ref = H.shadow_ray(land, pd[:, 3], tweak)[2]
    return float(np.abs(ST.shadow_precision(pd[:, 3]).astype(np.float64) / ref - 1.0).max())


def shapes(land):
    """The cases a landscape is checked on, by name."""
    def make():
        cs = [primary(land, "near"), primary(land, "far"), prepass(land), shadow(land)]
        if land == "greenrocks":
            cs += [primary(land, "near", calcfog=False), primary(land, "far", calcfog=False)]
        if land == "nomadplains":
            cs += [primary(land, "near", recording=1), primary(land, "far", recording=1)]
        return {c.name: c for c in cs}
    return K.cached(("march shapes", land), make)


# --- the trajectory and its checks (shared with the GPU tests) ----------------------------------------------
class Trajectory:
    """The runs capped at k = 1..STEPS side by side: index k - 1 is the state after min(k, the ray's own count)
    steps.  pd (K, n, 4), density (K, n), steps (K, n), fcolord (K, n, 4) or None; ran (K, n): the ray ran a k-th
    step."""

    def __init__(self, runs):
        self.pd = np.stack([r[0] for r in runs])
        self.density = np.stack([r[1] for r in runs])
        self.steps = np.stack([r[2] for r in runs]).astype(np.int64)
        self.fcolord = None if runs[0][3] is None else np.stack([r[3] for r in runs])
        self.ran = self.steps == np.arange(1, len(runs) + 1)[:, None]
        self.count = self.steps[-1]  # of the longest run: the ray's own count where it is below STEPS


def observe(run, steps=STEPS):
    """run(k) -> (pd, density, steps, fcolord or None) of the march capped at k."""
    return Trajectory([run(k) for k in range(1, steps + 1)])


def oracle_trajectory(case):
    def run(k):
        pd, fc, dens, st = case.oracle(k)
        return pd, dens, st, fc
    return K.cached(("march trajectory", case.land, case.name), lambda: observe(run))


def check_prefix(t):
    """The capped runs are one trajectory: a ray that ran a k-th step ran every step before it; one that did not
    reports at k what it reported at k - 1, bit for bit.  (That the (k+1)-th sample continues from the k-th
    distance is check()'s position.)"""
    assert np.all(t.steps <= np.arange(1, len(t.steps) + 1)[:, None])
    assert np.all(t.ran[:-1] | ~t.ran[1:])
    still = ~t.ran[1:]
    assert np.array_equal(t.steps[1:][still], t.steps[:-1][still])
    for a in (t.pd, t.density) + (() if t.fcolord is None else (t.fcolord,)):
        assert np.array_equal(a[1:][still].view(np.uint32), a[:-1][still].view(np.uint32))


def restate(case, t, tweak=None):
    return H.march(case.land, case.p, case.dir, case.dist0, case.enddist, case.stepmod, case.recording, case.calcfog,
                   case.skiprefine, t.density, t.pd[:, :, :3], t.pd[:, :, 3], t.ran, tweak)


def check(case, t, tweak=None, fcolord=True):
    """The worst differences of a trajectory from the restatement: {"position", "dist", "fcolord" (where the
    trajectory has it), "termination": the count of rows where the loop condition disagrees, "unsafe": the share of
    the condition's rows left out as near ties}."""
    m = restate(case, t, tweak)
    ran = t.ran
    rayp, dist = t.pd[:, :, :3].astype(np.float64), t.pd[:, :, 3].astype(np.float64)
    out = {}
    err = np.abs(m.pos - rayp).max(axis=2) / np.maximum(1.0, np.abs(rayp).max(axis=2))
    out["position"] = float(err[ran].max()) if ran.any() else 0.0
    err = np.abs(m.dist - dist) / np.maximum(1.0, np.abs(dist))
    out["dist"] = float(err[ran].max()) if ran.any() else 0.0
    if t.fcolord is not None and fcolord:
        err = np.abs(m.f[1:] - t.fcolord.astype(np.float64)).max(axis=2)
        out["fcolord"] = float(err[ran].max()) if ran.any() else 0.0
    # before every step that ran the condition holds ...
    before = ran & ~m.unsafe[:-1]
    wrong = int((before & ~m.cond[:-1]).sum())
    # ... and after the last step of a ray that ended by itself it fails, unless skiprefine's break ended it
    n = ran.shape[1]
    own = np.flatnonzero(t.count < len(ran))
    last = t.count[own]
    looped = ~m.ended[last, own]
    safe = ~m.unsafe[last, own]
    wrong += int((looped & safe & m.cond[last, own]).sum())
    if case.skiprefine:  # a hit ends the ray there, with the distance it was sampled at
        hit = ran & (t.density > 0)
        wrong += int((hit[:-1] & ran[1:]).sum())
        wrong += int((hit & (m.dist != np.concatenate([np.broadcast_to(case.dist0.astype(np.float64), (1, n)),
                                                         dist[:-1]]))).sum())
        wrong += int((m.ended[last, own] != (t.density[np.maximum(last, 1) - 1, own] > 0) & (last > 0)).sum())
    out["termination"] = wrong
    rows = int(ran.sum()) + len(own)
    out["unsafe"] = float(((ran & m.unsafe[:-1]).sum() + (~safe).sum()) / max(rows, 1))
    return out


def density_check(case, t):
    """(the worst density_error of the samples against hlsl_ref.density at the observed positions, the share left
    out as unsafe)."""
    ran = t.ran
    p = t.pd[:, :, :3][ran]
    ref, unsafe = H.density(case.land, p, F_EYE)
    err = K.density_error(t.density[ran], ref, p)
    return float(err[~unsafe].max()), float(unsafe.mean())


def assert_within(case, t, figures=None):
    """A trajectory's assertions: every figure within its bound, termination exact, near ties rare."""
    land = case.land
    got = check(case, t) if figures is None else figures
    print(land, case.name, " ".join("%s %.3g" % kv for kv in got.items()))
    for q in ("position", "dist", "fcolord"):
        if q in got:
            assert got[q] <= bound(q, land), (land, case.name, q, got[q])
    assert got["termination"] == 0, (land, case.name)
    assert got["unsafe"] <= K.MAX_UNSAFE, (land, case.name)


def assert_density(case, t):
    worst, unsafe = density_check(case, t)
    print(case.land, case.name, "density %.3g unsafe %.3g" % (worst, unsafe))
    assert unsafe <= K.MAX_UNSAFE
    assert worst <= bound("density", case.land), (case.land, case.name, worst)


def census(land, near, far, fog=None):
    """What a green run must have exercised, from the trajectories of primary near and far (and, for greenrocks,
    near's fcolord): every branch of the loop."""
    _, dens = full_march(land)
    hits = dens > 0
    ended = near.count < STEPS
    final_density = near.density[-1]
    final_dist = near.pd[-1, :, 3]
    enddist = ranges(land, "near")[:, 1]
    assert (ended & (final_density > 0))[hits].mean() >= 0.95, land
    assert (ended & (final_dist >= enddist)).sum() >= 64, land
    assert (near.ran & (near.density > 0)).sum() >= 1000, land
    d = np.concatenate([near.density[near.ran], far.density[far.ran]])
    assert (d < -5).sum() >= 1000, land
    assert ((d >= -5) & (d <= 0)).sum() >= 1000, land
    if fog is not None:
        assert (fog[:, :, 3] != 0).any(axis=0).sum() >= 64
        assert (fog < 0).any()


# --- the tests -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("land", LANDS)
def test_census(land):
    cs = shapes(land)
    near, far = (oracle_trajectory(cs[primary(land, w).name]) for w in ("near", "far"))
    census(land, near, far, near.fcolord if land == "greenrocks" else None)


@pytest.mark.parametrize("land", LANDS)
def test_the_capped_runs_are_one_trajectory(land):
    for case in shapes(land).values():
        check_prefix(oracle_trajectory(case))


@pytest.mark.parametrize("land", LANDS)
def test_march(land):
    for case in shapes(land).values():
        assert_within(case, oracle_trajectory(case))


@pytest.mark.parametrize("land", LANDS)
def test_density_at_the_samples(land):
    for case in shapes(land).values():
        if case.name.endswith(" fog") or case.recording:
            continue  # the same samples as the shape without (test_the_trajectory_does_not_depend_on_...)
        assert_density(case, oracle_trajectory(case))


def _same_steps(a, b):
    return (np.array_equal(a.pd.view(np.uint32), b.pd.view(np.uint32)) and np.array_equal(a.steps, b.steps)
            and np.array_equal(a.density.view(np.uint32), b.density.view(np.uint32)))


def test_the_trajectory_does_not_depend_on_calcfog():
    cs = shapes("greenrocks")
    for which in ("near", "far"):
        fog, plain = (oracle_trajectory(cs[primary("greenrocks", which, calcfog=f).name]) for f in (True, False))
        assert _same_steps(fog, plain)
        assert fog.fcolord.any() and not plain.fcolord.any()


def test_recording_walks_other_steps():
    cs = shapes("nomadplains")
    a, b = (oracle_trajectory(cs[primary("nomadplains", "near", recording=r).name]) for r in (0, 1))
    assert not np.array_equal(a.pd, b.pd)


@pytest.mark.parametrize("land", LANDS)
def test_fog_is_live_on_greenrocks_alone(land):
    for case in shapes(land).values():
        fc = oracle_trajectory(case).fcolord
        assert fc.any() == (land == "greenrocks" and case.calcfog), case.name


@pytest.mark.parametrize("land", LANDS)
def test_shadow_ray_is_get_colors(land):
    """The shadow shape's arguments are what get_color passes: its class and fcolord.w, bit for bit."""
    rows, pd = near_hits(land)
    case = shapes(land)["shadow"]
    _, fc, dens, _ = case.oracle(0)
    up = np.tile(np.array([0, 1, 0], np.float32), (len(pd), 1))
    _, cls, w = ST.color(land, pd[:, :3], up, K.unit(rays()[1][rows]).astype(np.float32), pd[:, 3], F_EYE)
    assert np.array_equal(np.where(dens > 0, SH.SHADOWED, SH.LIT), cls)
    assert np.array_equal(fc[:, 3].view(np.uint32), w.view(np.uint32))
    assert min((cls == SH.LIT).sum(), (cls == SH.SHADOWED).sum()) >= 8


@pytest.mark.parametrize("land", LANDS)
def test_shadow_precision(land):
    """`precision` of color.hlsl:47-50, relative; both sides of its floor of 8."""
    stepmod = shapes(land)["shadow"].stepmod
    assert (stepmod > 8).sum() >= 16 and (stepmod == 8).sum() >= 16
    assert worst_precision(land) <= bound("precision", land)


def fog_colour_check(t, shaded):
    """The fog the march accumulates, seen through the shaded query, whose capped state is a miss wherever the
    k-th density is <= 0: colour = lerp(lerp(sky, f.rgb, f.w), sky, skyAmount) (tracescreen.hlsl:37-38) with the
    RESTATED f, teacher-forced on the trajectory t of the surface query for the same rays (greenrocks, far set).
    shaded: the shaded query's results capped at k = 1..STEPS, (n, 8) each.  (worst colour difference over the
    compared rows, the count of compared rows with f.w > 1e-3)."""
    case = shapes("greenrocks")["primary far fog"]
    shaded = np.stack(shaded)
    pd, dens = shaded[:, :, [4, 5, 6, 3]], shaded[:, :, 7]
    assert np.array_equal(pd.view(np.uint32), t.pd.view(np.uint32))  # the two queries walk the same steps
    assert np.array_equal(dens.view(np.uint32), t.density.view(np.uint32))
    f = restate(case, t).f[1:]
    k, i = np.nonzero(t.ran & ~(dens > 0))
    ref, _ = H.sample_color("greenrocks", pd[k, i], dens[k, i], f[k, i], K.unit(case.dir)[i], F_EYE, SH.SUN, None, None,
                            None)
    err = np.abs(shaded[k, i, :3].astype(np.float64) - ref).max()
    return float(err), int((f[k, i, 3] > 1e-3).sum())


def fog_colour_bound():
    return K.bound("miss", "greenrocks") + bound("fcolord", "greenrocks")


def test_fog_reaches_the_miss_colour():
    """fog_colour_check on the checkers of the surface and shaded queries (tests/test_gpu_march_kat.py runs it on
    the device): the oracle's trace_ray once more, through tests/tools/surface_ref.c and shade_ref.c."""
    case = shapes("greenrocks")["primary far fog"]
    rg = np.stack([case.dist0, case.enddist], axis=1)

    def run(k):
        res, st = SR.trace(case.p, case.dir, F_EYE, "greenrocks", ranges=rg, max_steps=k)
        return res[:, :4], res[:, 7], st, None
    t = observe(run)
    assert _same_steps(t, oracle_trajectory(case))
    shaded = [SH.shade(case.p, case.dir, F_EYE, "greenrocks", ranges=rg, max_steps=k)[0] for k in range(1, STEPS + 1)]
    worst, live = fog_colour_check(t, shaded)
    print("fog colour %.3g, %d rows with f.w > 1e-3" % (worst, live))
    assert live >= 1000
    assert worst <= fog_colour_bound()


# antialiasing.hlsl:9-49, AA_SAMPLE_OFFSETS per AA_SAMPLES
AA_SAMPLE_OFFSETS = {
    1: [(0.0, 0.0)],
    2: [(4.0, 4.0), (-4.0, -4.0)],
    4: [(-2.0, -6.0), (6.0, -2.0), (-6.0, 2.0), (2.0, 6.0)],
    8: [(1.0, -3.0), (-1.0, 3.0), (5.0, 1.0), (-3.0, -5.0), (-5.0, 5.0), (-7.0, -1.0), (3.0, 7.0), (7.0, -7.0)],
    16: [(1.0, 1.0), (-1.0, 3.0), (-3.0, 2.0), (4.0, -1.0), (-5.0, -2.0), (2.0, 5.0), (5.0, 3.0), (3.0, -5.0),
         (-2.0, 6.0), (0.0, -7.0), (-4.0, -6.0), (-6.0, 4.0), (-8.0, 0.0), (7.0, -4.0), (6.0, 7.0), (-7.0, -8.0)],
}


@pytest.mark.parametrize("samples", sorted(AA_SAMPLE_OFFSETS))
def test_aa_offsets(samples):
    """getSampleOffset (antialiasing.hlsl:56-59): the table over 16, exact in float32."""
    want = np.array(AA_SAMPLE_OFFSETS[samples], np.float64) / 16.0
    got = ST.aa_offsets(samples)
    assert got.shape == want.shape and np.array_equal(got.astype(np.float64), want)


# --- the mutation check --------------------------------------------------------------------------------
# Mutants that stay inside every bound and keep the termination check: name -> (measured worst deviation: of the
# march's as a multiple of its bound, of `precision` itself; reason).
ESCAPES = {
    "nomadplains.shadow.length": (0.07, "enddist enters the loop condition alone, and no shadow ray of the set ends "
                                  "with its distance in [100, 100.1)"),
}
for _land, _m in zip(LANDS, MEASURED["precision"]):
    ESCAPES[_land + ".shadow.mip_floor"] = (_m, "saturated: max(0.5 log2 dist, 1) is another value for dist < 4 alone, "
                                            "where precision stays at its floor of 8")


def mutant_shapes(name):
    """(land, shape name) of the trajectories that read a mutant's literal."""
    if name in H.MARCH_FOG:
        return [("greenrocks", "primary near fog"), ("greenrocks", "primary far fog"), ("greenrocks", "shadow")]
    if name in H.MARCH_RECORDING:
        return [("nomadplains", "primary near recording"), ("nomadplains", "primary far recording")]
    return [("nomadplains", "primary near"), ("nomadplains", "primary far")]


def mutant_worst(name, tweak):
    """(leaves: a bound is exceeded or termination disagrees, the largest figure over its bound)."""
    ratio = 0.0
    for land, shape in mutant_shapes(name):
        case = shapes(land)[shape]
        got = check(case, oracle_trajectory(case), tweak)
        if got["termination"]:
            return True, float("inf")
        for q in ("position", "dist", "fcolord"):
            if q in got:
                b = bound(q, land)
                ratio = max(ratio, got[q] / b if b else (float("inf") if got[q] else 0.0))
        if ratio > 1.0:
            return True, ratio
    return False, ratio


def test_mutants():
    """Every mutant leaves a bound or breaks the termination check on the shapes that read it, or is listed in
    ESCAPES with the reason (and then does stay inside)."""
    wrong = []
    for name, tweak in H.mutants("march"):
        leaves, ratio = mutant_worst(name, tweak)
        if leaves == (name in ESCAPES):
            wrong.append((name, ratio))
    assert not wrong, wrong


def shadow_mutant_leaves(land, name, tweak):
    """A literal of the shadow ray's arguments: `precision` against the oracle's, start and length through the
    shadow shape's trajectory (the oracle marched from 0.4 to 100)."""
    if worst_precision(land, tweak) > bound("precision", land):
        return True
    case = shapes(land)["shadow"]
    got = check(shadow(land, tweak), oracle_trajectory(case))
    return bool(got["termination"]) or any(got[q] > bound(q, land) for q in ("position", "dist", "fcolord"))


@pytest.mark.parametrize("land", LANDS)
def test_shadow_mutants(land):
    wrong = []
    for name, tweak in H.mutants(land + ".shadow"):
        if shadow_mutant_leaves(land, name, tweak) == (name in ESCAPES):
            wrong.append(name)
    assert not wrong, wrong


def all_mutants():
    yield from H.mutants("march")
    for land in LANDS:
        yield from H.mutants(land + ".shadow")


def test_every_escape_names_a_mutant():
    names = {n for n, _ in all_mutants()}
    for k in ESCAPES:
        assert k in names, k


def test_the_mutants_cover_the_issue():
    names = {n for n, _ in H.mutants("march")}
    for lit in ("ray_step", "final_precision", "density_factor", "recording_density_factor", "step_factor",
                "recording_step_factor", "refine", "density_bias", "stepmult_one", "mid_half"):
        assert "march." + lit in names
    assert {"march.structure=" + s for s in H.MARCH_STRUCTURES} <= names
    for n in H.MARCH_RECORDING + H.MARCH_NOT_RECORDING + H.MARCH_FOG:
        assert n in names, n


if __name__ == "__main__":  # the figures of MEASURED and ESCAPES, from this module's own sets
    worst = {q: [0.0] * len(LANDS) for q in QUANTITIES}
    for i, land in enumerate(LANDS):
        for case in shapes(land).values():
            t = oracle_trajectory(case)
            got = check(case, t)
            if not (case.name.endswith(" fog") or case.recording):
                got["density"], got["density unsafe"] = density_check(case, t)
            print(land, case.name, " ".join("%s %.3g" % kv for kv in got.items()))
            for q in QUANTITIES:
                worst[q][i] = max(worst[q][i], got.get(q, 0.0))
        worst["precision"][i] = worst_precision(land)
    for q in QUANTITIES:
        print('    "%s": (%s),' % (q, ", ".join("%.2e" % v for v in worst[q])))
    if all(v is not None for v in MEASURED.values()):
        for q in QUANTITIES:
            print("    %-10s %s" % (q, "  ".join("%.2e / %.0e" % (MEASURED[q][i], bound(q, land))
                                                 for i, land in enumerate(LANDS))))
        for name, tweak in H.mutants("march"):
            leaves, ratio = mutant_worst(name, tweak)
            print("mutant", name, "leaves" if leaves else "ESCAPES", "%.3g x bound" % ratio)
        for land in LANDS:
            for name, tweak in H.mutants(land + ".shadow"):
                print("mutant", name, "leaves" if shadow_mutant_leaves(land, name, tweak) else "ESCAPES")
