"""Known-answer tests of the AO extension and the AA resolve against tests/hlsl_ref.py's float64 reading of DESIGN.md
section 9 and of tracescreen.hlsl:63-75.  AO has no reference shader: its definition is a paragraph of DESIGN.md
that was typed twice, into the oracle (rt_oracle.c ao_dir / ambient_occlusion) and into the device (rt_shader.h),
and every other AO test compares those two copies.  A misreading they share (u1 and u2 swapped, a uniform
hemisphere, the other handedness, k * 16 + a, AO inside the saturate or on the sky) fails here, and in
tests/test_gpu_ao_kat.py for the device.

What is compared, and with which bound:
    pcg_hash      the oracle's against Python integers mod 2^32: equal, with three known answers
    ao_uv         the restatement against a literal transcription of the paragraph written here: equal
    ao_dir        the oracle's direction against the restatement on dir_inputs() (20,418 normals and keys): the largest
                  component difference over max(|n|, 1) within DIR_BOUND = 2 * DIR_MEASURED; for unit normals
                  ||d| - 1| (measured 2.3e-7) and |d.n - sqrt(1 - u1)| (1.5e-7) within the same bound and d.n >= 0
                  (the least is 2.4e-4, the grazing ray's 2^-12)
    distribution  of the restated (u1, u2) over three frame tiles: no duplicates, the mean of sqrt(1 - u1) within 5
                  standard errors of 2/3 (a cosine-weighted hemisphere; a uniform one has 1/2), chi^2 of an 8 x 8
                  histogram below 103 (99.9 % for 63 degrees of freedom)
    composition   ambient_occlusion = ao_factor(the count of occluded stage_ref.trace_ray runs with ao_ray()'s
                  arguments along st_ao_dir) at camera F0's hits (768, 736, 767 and 762 points): the count and the step
                  sum equal, the float within 2 * 2^-24 (measured 3.0e-8), for K = 1, 4 and 16.  At K = 4 the four
                  sets together hold 1998 points with occ = 0, 1005 with 0 < occ < 4 and 30 with occ = 4 (10, 1, 0
                  and 19 a landscape: the smooth hills of testing and simple close in on hardly any hit)
    resolve       every pixel of ro_tracescreen's 64 x 64 frames of camera F0 (greenrocks and simple, the (A, K) of
                  RESOLVE_CASES) rebuilt through hlsl_ref.resolve from st_trace_samples within (A + 4) * 2^-24: A
                  products and A additions of partial sums <= A, the multiply by rcp(A) exact for a power of two
                  (asserted), two roundings in ao_factor; measured 1.7e-7 at A = 16 (bound 1.2e-6).  RGBA8 equal to
                  unorm8 of the restated value away from rounding ties, within one code at them; ties at most 0.1 %
                  of the channels (cap 1 %)

The march is not restated here: occlusion is stage_ref.trace_ray's, which tests/test_march_kat.py pins step by step;
the stepmod it is given is the oracle's own shadow_precision, held to the restated one as test_march_kat does (a
float64 precision rounded to float32 need not be the oracle's last bit, and another last bit is another march).

The mutation check runs every hlsl_ref.mutants("ao") and mutants("resolve") entry through mutant_leaves(); ESCAPES
lists those that no check can see, with the reason.
"""
import numpy as np
import pytest

import hlsl_ref as H
import oracle_lib as O
import point_ref as PR
import ray_fixture as RF
import shade_ref as SH
import stage_ref as ST
import test_hlsl_kat as K
import test_march_kat as M

F_EYE = K.F_EYE
LANDS = K.LANDS
# The oracle's largest difference from the restated direction over dir_inputs(), a component over max(|n|, 1)
# (python tests/test_ao_kat.py prints it); the bound is twice that.
DIR_MEASURED = 3.98e-07
DIR_BOUND = 2.0 * DIR_MEASURED
FACTOR_BOUND = 2.0 * 2.0 ** -24  # the two roundings of fma(-0.6, occ * rcp(K), 1) at values <= 1
AO_COUNTS = (1, 4, 16)
SEED = 3
FRAME = 64
RESOLVE_CASES = ((1, 0), (1, 4), (2, 1), (4, 0), (8, 2), (16, 4))  # (AA_SAMPLES, RT_AO_SAMPLES)
RESOLVE_LANDS = ("greenrocks", "simple")  # nomadplains' F0 view holds 2 hit samples with a channel above 1
MAX_TIES = 0.01


# --- pcg_hash and (u1, u2) -----------------------------------------------------------------------------
def test_pcg_hash():
    assert H.pcg_hash(0) == 0x07BB2FE2 and H.pcg_hash(1) == 0xA8BEEA3C and H.pcg_hash(0xFFFFFFFF) == 0xE62A4902
    rng = np.random.default_rng(90)
    x = np.concatenate([rng.integers(0, 2 ** 32, 2 ** 16, dtype=np.uint64).astype(np.uint32),
                        np.array([0, 1, 0x80000000, 0xFFFFFFFF], np.uint32)])
    got = ST.pcg_hash(x)
    assert np.array_equal(got.astype(np.uint64), H.pcg_hash(x))
    assert [int(v) for v in got[-4:]] == [H.pcg_hash(int(v)) for v in x[-4:]]  # the integer and the array form


def _uv_by_the_letter(px, py, a, k):
    """DESIGN.md section 9, first item, as it is printed, for one key."""
    m = 0xFFFFFFFF

    def pcg(x):
        st = (x * 747796405 + 2891336453) & m
        w = (((st >> ((st >> 28) + 4)) ^ st) * 277803737) & m
        return (w >> 22) ^ w

    h = pcg(((px * 0x9E3779B1) & m) ^ ((py * 0x85EBCA77) & m) ^ (((a * 16 + k) * 0xC2B2AE3D) & m))
    return (h >> 8) * 2.0 ** -24, (pcg(h) >> 8) * 2.0 ** -24


def test_ao_uv():
    rng = np.random.default_rng(91)
    keys = np.concatenate([frame_keys(rng, 1500), query_keys(rng, 500)])
    u1, u2 = H.ao_uv(*keys.T)
    want = np.array([_uv_by_the_letter(*(int(v) for v in row)) for row in keys])
    assert np.array_equal(u1, want[:, 0]) and np.array_equal(u2, want[:, 1])
    assert H.ao_uv(5, 7, 2, 3) == _uv_by_the_letter(5, 7, 2, 3)


# --- the directions ------------------------------------------------------------------------------------
def frame_keys(rng, n):
    """(px, py, a, k) over a frame's ranges: px < 3840, py < 2160, a < 16, k < 16."""
    return np.stack([rng.integers(0, hi, n) for hi in (3840, 2160, 16, 16)], axis=1).astype(np.uint32)


def query_keys(rng, n):
    """shade_points' keys (point index, seed, 0, k): px < 2^26, py any uint32, a = 0."""
    return np.stack([rng.integers(0, 2 ** 26, n), rng.integers(0, 2 ** 32, n), np.zeros(n, np.int64),
                     rng.integers(0, 16, n)], axis=1).astype(np.uint32)


def _unit32(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _with_nx(nx, rng):
    """Unit normals (float32) whose x is the float32 nx exactly."""
    nx = np.asarray(nx, np.float32)
    phi = rng.uniform(0, 2 * np.pi, len(nx))
    r = np.sqrt(1.0 - nx.astype(np.float64) ** 2)
    n = np.stack([nx.astype(np.float64), r * np.cos(phi), r * np.sin(phi)], axis=1).astype(np.float32)
    n[:, 0] = nx
    return n


def extreme_keys():
    """The keys with the smallest and the largest u1 among the 2^24 consecutive pixels px = 0 .. 2^24 - 1 (py = a =
    k = 0): the ray along the normal and the grazing ray."""
    def make():
        px = np.arange(2 ** 24, dtype=np.uint64)
        h = H.pcg_hash(H.ao_key(px, np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint64))) >> np.uint64(8)
        lo, hi = int(h.argmin()), int(h.argmax())
        return np.array([[lo, 0, 0, 0], [hi, 0, 0, 0]], np.uint32), (int(h[lo]), int(h[hi]))
    return K.cached(("ao extreme keys",), make)


def dir_inputs():
    """(normals (n, 3) float32, keys (n, 4) uint32, the rows with unit normals, {group: rows})."""
    def make():
        rng = np.random.default_rng(92)
        f32 = np.float32
        edge = f32(0.9)
        around = np.array([np.nextafter(edge, f32(0)), edge, np.nextafter(edge, f32(1))], f32)
        axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(f32)
        band = rng.uniform(0.8, 0.9, 1000).astype(f32) * np.where(rng.random(1000) < 0.5, -1, 1).astype(f32)
        scaled = _unit32(rng.normal(size=(1000, 3)))
        ext, _ = extreme_keys()
        groups = [
            ("frame", _unit32(rng.normal(size=(12000, 3))), frame_keys(rng, 12000)),
            ("query", _unit32(rng.normal(size=(6000, 3))), query_keys(rng, 6000)),
            ("axes", np.tile(axes, (4, 1)), frame_keys(rng, 24)),
            ("switch", _with_nx(np.linspace(0.899, 0.901, 200).astype(f32), rng), frame_keys(rng, 200)),
            ("around", _with_nx(np.concatenate([around, -around]), rng), frame_keys(rng, 6)),
            ("band", _with_nx(band, rng), frame_keys(rng, 1000)),
            ("half", scaled[:500] * f32(0.5), query_keys(rng, 500)),
            ("double", scaled[500:] * f32(2), frame_keys(rng, 500)),
            ("along", _unit32(rng.normal(size=(94, 3))), np.tile(ext[0], (94, 1))),
            ("grazing", _unit32(rng.normal(size=(94, 3))), np.tile(ext[1], (94, 1))),
        ]
        rows, at = {}, 0
        for name, nr, _ in groups:
            rows[name] = np.arange(at, at + len(nr))
            at += len(nr)
        normals = np.ascontiguousarray(np.concatenate([g[1] for g in groups]), f32)
        keys = np.ascontiguousarray(np.concatenate([g[2] for g in groups]), np.uint32)
        unit = np.ones(len(normals), bool)
        unit[rows["half"]] = unit[rows["double"]] = False
        for a in (normals, keys, unit):
            a.setflags(write=False)
        return normals, keys, unit, rows
    return K.cached(("ao dir inputs",), make)


def oracle_dirs():
    return K.cached(("ao oracle dirs",), lambda: ST.ao_dir(*dir_inputs()[:2]))


def worst_dir(got, tweak=None):
    """The largest component difference of directions from the restatement over dir_inputs(), over max(|n|, 1)."""
    normals, keys, _, _ = dir_inputs()
    ref = H.ao_dir(normals, *keys.T, tweak=tweak)
    scale = np.maximum(np.linalg.norm(normals.astype(np.float64), axis=1), 1.0)
    return float((np.abs(np.asarray(got, np.float64) - ref).max(axis=1) / scale).max())


def worst_properties(got):
    """For the unit normals: (the largest ||d| - 1|, the largest |d.n - sqrt(1 - u1)|, the smallest d.n)."""
    normals, keys, unit, _ = dir_inputs()
    d, n = np.asarray(got, np.float64)[unit], normals.astype(np.float64)[unit]
    u1, _ = H.ao_uv(*keys[unit].T)
    dn = (d * n).sum(axis=1)
    return (float(np.abs(np.linalg.norm(d, axis=1) - 1.0).max()), float(np.abs(dn - np.sqrt(1.0 - u1)).max()),
            float(dn.min()))


def test_dir_inputs():
    normals, keys, unit, rows = dir_inputs()
    assert len(normals) >= 20000
    nx = np.abs(normals[:, 0])
    edge = np.float32(0.9)
    sw = nx[rows["switch"]]
    assert (sw > edge).sum() >= 50 and (sw < edge).sum() >= 50
    for sign in (1, -1):
        got = set((sign * normals[rows["around"], 0]).tolist())
        assert {float(np.nextafter(edge, np.float32(0))), float(edge), float(np.nextafter(edge, np.float32(1)))} <= got
    assert ((nx[rows["band"]] > 0.8) & (nx[rows["band"]] < edge)).all()
    length = np.linalg.norm(normals.astype(np.float64), axis=1)
    assert np.allclose(length[rows["half"]], 0.5, atol=1e-6) and np.allclose(length[rows["double"]], 2, atol=1e-6)
    assert np.allclose(length[unit], 1, atol=1e-6)
    assert keys[rows["query"], 0].max() >= 2 ** 25 and keys[rows["query"], 1].max() >= 2 ** 31
    _, (lo, hi) = extreme_keys()
    assert lo <= 2 and hi >= 2 ** 24 - 3, (lo, hi)  # u1 within 2e-7 of 0 and of 1


def assert_directions(got):
    """What the oracle's and the device's directions must meet."""
    worst = worst_dir(got)
    length, cosine, least = worst_properties(got)
    print("ao_dir %.3g, |d| - 1 %.3g, d.n - sqrt(1 - u1) %.3g, least d.n %.3g" % (worst, length, cosine, least))
    assert worst <= DIR_BOUND
    assert length <= DIR_BOUND and cosine <= DIR_BOUND
    assert least >= 0.0


def test_ao_dir():
    assert_directions(oracle_dirs())


# --- the distribution the definition promises -----------------------------------------------------------
def tile_keys(size, aa, ao):
    y, x, a, k = np.meshgrid(np.arange(size), np.arange(size), np.arange(aa), np.arange(ao), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), a.ravel(), k.ravel()], axis=1).astype(np.uint32)


TILES = ((64, 1, 4), (32, 4, 4), (16, 16, 16))


def distribution(keys, tweak=None):
    """(duplicate (u1, u2) pairs, the mean of sqrt(1 - u1) in standard errors from 2/3, chi^2 of the 8 x 8 histogram)."""
    u1, u2 = H.ao_uv(*keys.T, tweak=tweak)
    n = len(u1)
    pairs = (u1 * 2.0 ** 24).astype(np.int64) << 24 | (u2 * 2.0 ** 24).astype(np.int64)
    dup = n - len(np.unique(pairs))
    z = (np.sqrt(1.0 - u1).mean() - 2.0 / 3.0) / (np.sqrt(1.0 / 18.0) / np.sqrt(n))
    hist = np.histogram2d(u1, u2, bins=8, range=((0, 1), (0, 1)))[0]
    chi2 = ((hist - n / 64.0) ** 2 / (n / 64.0)).sum()
    return int(dup), float(z), float(chi2)


def distribution_fails(tweak=None):
    for tile in TILES:
        dup, z, chi2 = distribution(tile_keys(*tile), tweak)
        if dup or abs(z) > 5.0 or chi2 >= 103.0:
            return True
    return False


@pytest.mark.parametrize("tile", TILES)
def test_distribution(tile):
    dup, z, chi2 = distribution(tile_keys(*tile))
    print("tile %s: %d duplicates, mean %.2f standard errors from 2/3, chi2 %.1f" % (tile, dup, z, chi2))
    assert dup == 0
    assert abs(z) <= 5.0
    assert chi2 < 103.0


# --- ambient_occlusion as a composition ---------------------------------------------------------------
def hits(land):
    """(points, normals, dist) of camera F0's rays that hit: the oracle's rr.pd and get_normal."""
    def make():
        o, d = RF.rays("F0")
        pd, nd, _, _, _ = PR.primary(o, d, F_EYE, land)
        h = np.flatnonzero(nd[:, 3] > 0)
        return tuple(np.ascontiguousarray(a) for a in (pd[h, :3], nd[h, :3], pd[h, 3]))
    return K.cached(("ao hits", land), make)


def point_keys(n, seed, k):
    return np.stack([np.arange(n), np.full(n, seed), np.zeros(n, np.int64), np.full(n, k)], axis=1).astype(np.uint32)


def compose(land, p, normals, dist, keys_of, samples, dirs=ST.ao_dir, tweak=None):
    """(occ (n,), steps (n,)) of `samples` AO rays from each point: stage_ref.trace_ray with hlsl_ref.ao_ray's
    arguments along dirs(normals, keys_of(k)).  The stepmod is the oracle's shadow_precision(dist), which must lie
    within test_march_kat's bound of the restated one."""
    n = len(p)
    dist0, enddist, precision, calcfog, skiprefine, cap = H.ao_ray(dist, tweak, land)
    stepmod = ST.shadow_precision(dist)
    assert np.abs(stepmod / precision - 1.0).max() <= M.bound("precision", land)
    occ, steps = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for k in range(samples):
        _, _, dens, st = ST.trace_ray(land, p, dist0, enddist, stepmod, dirs(normals, keys_of(k)), F_EYE, calcfog,
                                      skiprefine, cap)
        occ += dens > 0
        steps += st
    return occ, steps


def decode_occ(ao, samples):
    """The count of occluded rays an AO factor stands for."""
    return np.rint((1.0 - np.asarray(ao, np.float64)) * samples / 0.6).astype(np.int64)


def composition_check(land, samples, tweak=None):
    """(rows whose decoded count differs, rows whose step sum differs, the largest difference of the factor, occ)."""
    p, nr, dist = hits(land)
    want, want_steps = K.cached(("ao oracle", land, samples),
                                lambda: PR.ambient_occlusion(p, nr, dist, F_EYE, land, samples, SEED))
    occ, steps = compose(land, p, nr, dist, lambda k: point_keys(len(p), SEED, k), samples, tweak=tweak)
    err = np.abs(H.ao_factor(occ, samples, tweak) - want.astype(np.float64)).max()
    return (int((decode_occ(want, samples) != occ).sum()), int((steps != want_steps.astype(np.int64)).sum()), float(err),
            occ)


@pytest.mark.parametrize("samples", AO_COUNTS)
@pytest.mark.parametrize("land", LANDS)
def test_ambient_occlusion_is_the_composition(land, samples):
    assert len(hits(land)[0]) >= 512
    wrong, wrong_steps, err, occ = composition_check(land, samples)
    print(land, samples, "factor %.3g" % err, np.bincount(occ, minlength=samples + 1))
    assert wrong == 0 and wrong_steps == 0
    assert err <= FACTOR_BOUND
    if samples == 4:
        assert min((occ == 0).sum(), ((occ > 0) & (occ < 4)).sum()) >= 16


def test_composition_census():
    """At K = 4 the sets hold every class of the count: none, some and all of the rays occluded, 16 times at least
    (all four occluded is rare at a camera's hits: the four landscapes' sets are counted together)."""
    occ = np.concatenate([composition_check(land, 4)[3] for land in LANDS])
    assert min((occ == 0).sum(), ((occ > 0) & (occ < 4)).sum(), (occ == 4).sum()) >= 16


def test_ao_factor():
    for samples in (1, 2, 4, 16):
        for occ in range(samples + 1):
            assert abs(float(ST.ao_factor(occ, samples)) - H.ao_factor(occ, samples)) <= FACTOR_BOUND


# --- the resolve -----------------------------------------------------------------------------------------
def frame_consts():
    c = dict(RF.consts("F0"))
    c["width"] = c["height"] = FRAME
    c["sun"] = SH.SUN
    return c


def oracle_frame(land, aa, ao):
    return K.cached(("ao frame", land, aa, ao), lambda: O.render(
        O.noise_tables(), O.make_frame(frame_consts(), landscape=O.LANDSCAPES[land], aa=aa, ao=ao)))


def sample_rays(aa, cell_distance):
    """The samples of the frame's pixels, pixel after pixel: (p, dir, ranges, keys (px, py, a))."""
    f32 = np.float32
    off = ST.aa_offsets(aa)
    assert len(off) == aa
    y, x, a = (v.ravel() for v in np.meshgrid(np.arange(FRAME), np.arange(FRAME), np.arange(aa), indexing="ij"))
    p, d = ST.pixel_ray(frame_consts(), x.astype(f32) + off[a, 0], y.astype(f32) + off[a, 1])
    # tracescreen.hlsl:57-61: the pixel's cell of the 32 x 32 prepass, exact for a 64 x 64 frame
    cell = (y * 32 // FRAME) * 32 + x * 32 // FRAME
    cd = np.asarray(cell_distance, f32).reshape(1024, 2)
    ranges = np.stack([cd[cell, 0], np.full(len(cell), RF.FAR, f32)], axis=1).astype(f32)
    return p, d, ranges, np.stack([x, y, a], axis=1).astype(np.uint32)


def oracle_samples(land, aa, ao):
    def make():
        p, d, rg, keys = sample_rays(aa, oracle_frame(land, aa, ao)["cell_distance"])
        return ST.trace_samples(frame_consts(), land, p, d, rg, keys, aa, ao)
    return K.cached(("ao samples", land, aa, ao), make)


def restate_pixels(aa, ao, colours, factors, hit, tweak=None):
    """hlsl_ref.resolve for a frame's samples (pixel after pixel).  A miss has no AO factor: it is handed the
    darkest one, ao_factor(K, K), which the definition must not read."""
    n = len(colours) // aa
    dark = H.ao_factor(ao, ao) if ao else 1.0
    f = np.where(hit, factors, dark) if ao else np.ones(len(colours))
    return H.resolve(np.asarray(colours).reshape(n, aa, 3), f.reshape(n, aa), np.asarray(hit).reshape(n, aa), tweak)


def resolve_bound(aa):
    return (aa + 4) * 2.0 ** -24


def resolve_check(aa, ref, img32, img8=None):
    """(the largest difference of the float pixels, RGBA8 codes that break the tie rule, the share of channels at a
    tie).  img32 may be None (an RGBA8-only device)."""
    ref = ref.reshape(-1, 4)
    err = 0.0 if img32 is None else float(np.abs(np.asarray(img32, np.float64).reshape(-1, 4) - ref).max())
    if img8 is None:
        return err, 0, 0.0
    t = 255.0 * np.clip(ref, 0.0, 1.0)
    tie = np.abs(t - np.floor(t) - 0.5) <= 255.0 * resolve_bound(aa)
    diff = np.abs(np.asarray(img8, np.int64).reshape(-1, 4) - H.unorm8(ref))
    return err, int(((diff > 0) & ~tie).sum() + (diff > 1).sum()), float(tie.mean())


def assert_resolved(aa, ref, img32, img8):
    err, wrong8, ties = resolve_check(aa, ref, img32, img8)
    print("A %d: float %.3g (bound %.3g), %d wrong codes, ties %.4f" % (aa, err, resolve_bound(aa), wrong8, ties))
    assert err <= resolve_bound(aa)
    assert wrong8 == 0
    assert ties < MAX_TIES


def resolve_census(colours, hit):
    """(hit samples, miss samples) with a channel above 1: what the resolve's misreadings differ on."""
    over = (np.asarray(colours) > 1).any(axis=1)
    return int((over & hit).sum()), int((over & ~hit).sum())


def oracle_resolve(land, aa, ao, tweak=None):
    col, f, _, dens = oracle_samples(land, aa, ao)
    return restate_pixels(aa, ao, col, f, dens > 0, tweak)


def test_rcp_of_a_power_of_two_is_exact():
    x = np.array([1, 2, 4, 8, 16], np.float32)
    assert np.array_equal(O.unary(6, x), np.float32(1) / x)


@pytest.mark.parametrize("aa,ao", RESOLVE_CASES)
@pytest.mark.parametrize("land", RESOLVE_LANDS)
def test_resolve(land, aa, ao):
    fr = oracle_frame(land, aa, ao)
    assert_resolved(aa, oracle_resolve(land, aa, ao), fr["rgba32f"], fr["rgba8"])
    col, f, _, dens = oracle_samples(land, aa, ao)
    assert (f[~(dens > 0)] == 1).all()
    if ao:
        assert (f[dens > 0] < 1).sum() >= 64


@pytest.mark.parametrize("land", RESOLVE_LANDS)
def test_resolve_census(land):
    for aa, ao in RESOLVE_CASES:
        col, _, _, dens = oracle_samples(land, aa, ao)
        over_hit, over_miss = resolve_census(col, dens > 0)
        print(land, aa, ao, over_hit, over_miss)
        assert over_hit >= 8 and over_miss >= 8


# --- the mutation check --------------------------------------------------------------------------------
# Mutants that no check here can see: name -> the reason.
ESCAPES = {
    "ao.up_steep_y": "the basis normalises up x n: (0, 1.1, 0) spans the same tx as (0, 1, 0)",
    "ao.up_x": "the basis normalises up x n: (1.1, 0, 0) spans the same tx as (1, 0, 0)",
    "ao.structure=fog_on": "the fog accumulation steers no branch of the march (test_march_kat's "
                           "test_the_trajectory_does_not_depend_on_calcfog) and ambient_occlusion reads the sign of "
                           "rr.density alone: an AO ray marched with fog on is occluded on the same rays after the same "
                           "steps, so the flag costs time and cannot change a pixel",
}
MUTANT_LAND, MUTANT_SAMPLES = "greenrocks", 4


def mutant_leaves(name, tweak):
    """Whether a mutant puts one of the checks above outside its bound."""
    if name.startswith("resolve."):
        for land in RESOLVE_LANDS:
            for aa, ao in RESOLVE_CASES:
                fr = oracle_frame(land, aa, ao)
                err, wrong8, _ = resolve_check(aa, oracle_resolve(land, aa, ao, tweak), fr["rgba32f"], fr["rgba8"])
                if err > resolve_bound(aa) or wrong8:
                    return True
        return False
    x = (np.arange(4096, dtype=np.uint64) * np.uint64(1048583)).astype(np.uint32)
    if not np.array_equal(ST.pcg_hash(x).astype(np.uint64), H.pcg_hash(x, tweak)):  # test_pcg_hash's comparison
        return True
    if worst_dir(oracle_dirs(), tweak) > DIR_BOUND:
        return True
    def reads(t):  # what the composition takes from the restatement besides the directions
        ray = H.ao_ray(1.0, t, MUTANT_LAND)
        return ray[:2] + ray[3:] + (H.ao_factor(1, MUTANT_SAMPLES, t),)

    if reads(tweak) != reads(None):  # (the composition with these as they are is the test above)
        wrong, wrong_steps, err, _ = composition_check(MUTANT_LAND, MUTANT_SAMPLES, tweak)
        if wrong or wrong_steps or err > FACTOR_BOUND:
            return True
    return False


def all_mutants():
    yield from H.mutants("ao")
    yield from H.mutants("resolve")


def test_mutants():
    """Every literal with its last digit changed by one and every named misreading leaves a bound, or is listed in
    ESCAPES with the reason (and then does stay inside)."""
    wrong = [name for name, tweak in all_mutants() if mutant_leaves(name, tweak) == (name in ESCAPES)]
    assert not wrong, wrong


def test_the_distribution_conditions_are_live():
    """They fail where the pairs are not uniform on the square or the height is not a cosine hemisphere's."""
    assert not distribution_fails()
    assert distribution_fails({"ao.shift_u": 9})  # (h >> 9) * 2^-24 fills a quarter of the square
    assert distribution_fails({"ao.key_px": 0})  # a key that forgets px: the pixels of a row share their pairs
    u1, _ = H.ao_uv(*tile_keys(*TILES[0]).T)
    z = ((1.0 - u1).mean() - 2.0 / 3.0) / (np.sqrt(1.0 / 18.0) / np.sqrt(len(u1)))
    assert abs(z) > 5.0  # sz = 1 - u1, the uniform hemisphere's height, has the mean 1/2


def test_the_mutants_cover_the_issue():
    names = {n for n, _ in all_mutants()}
    for lit in ("key_px", "key_py", "key_k", "pcg_mul", "pcg_add", "pcg_out", "shift_top", "shift_base", "shift_out",
                "shift_u", "pack", "up_switch", "up_steep_x", "up_steep_y", "up_steep_z", "up_x", "up_y", "up_z", "start",
                "end", "strength"):
        assert "ao." + lit in names, lit
    assert {"ao.structure=" + s for s in H.AO_STRUCTURES} | {"resolve.structure=" + s for s in H.RESOLVE_STRUCTURES} <= names
    for s in ("swap_u", "uniform_hemisphere", "rehash_key", "left_handed", "k_major", "swap_pixel", "fog_on", "refine"):
        assert s in H.AO_STRUCTURES
    for s in ("ao_inside_saturate", "ao_on_misses", "saturate_after_mean"):
        assert s in H.RESOLVE_STRUCTURES
    for k in ESCAPES:
        assert k in names, k


if __name__ == "__main__":  # the figures of DIR_MEASURED and ESCAPES, from this module's own sets
    print("ao_dir: worst %.3e over %d inputs" % (worst_dir(oracle_dirs()), len(dir_inputs()[0])))
    print("properties: |d| - 1 %.3e, d.n - sqrt(1 - u1) %.3e, least d.n %.3e" % worst_properties(oracle_dirs()))
    normals, keys, unit, rows = dir_inputs()
    ref = H.ao_dir(normals, *keys.T)
    scale = np.maximum(np.linalg.norm(normals.astype(np.float64), axis=1), 1.0)
    err = np.abs(oracle_dirs().astype(np.float64) - ref).max(axis=1) / scale
    for g, r in rows.items():
        print("    %-8s %.3e" % (g, err[r].max()))
    for tile in TILES:
        print("tile", tile, "duplicates %d, z %.2f, chi2 %.1f" % distribution(tile_keys(*tile)))
    for land in LANDS:
        for samples in AO_COUNTS:
            wrong, wrong_steps, e, occ = composition_check(land, samples)
            print(land, samples, len(occ), "hits; wrong", wrong, wrong_steps, "factor %.3e" % e,
                  np.bincount(occ, minlength=samples + 1))
    for land in RESOLVE_LANDS:
        for aa, ao in RESOLVE_CASES:
            fr = oracle_frame(land, aa, ao)
            col, _, _, dens = oracle_samples(land, aa, ao)
            print(land, aa, ao, "float %.3e (bound %.3e), wrong codes %d, ties %.4f" % (
                (resolve_check(aa, oracle_resolve(land, aa, ao), fr["rgba32f"], fr["rgba8"])[0], resolve_bound(aa))
                + resolve_check(aa, oracle_resolve(land, aa, ao), fr["rgba32f"], fr["rgba8"])[1:]),
                "census", resolve_census(col, dens > 0))
    for name, tweak in all_mutants():
        print("mutant", name, "leaves" if mutant_leaves(name, tweak) else "ESCAPES")
