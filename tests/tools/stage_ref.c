/*
 * stage_ref.c -- TEST INFRASTRUCTURE: the oracle's shading stages at inputs of the caller's own, for the
 * known-answer tests against the float64 restatement of the HLSL (tests/hlsl_ref.py, tests/test_hlsl_kat.py).
 * The oracle keeps get_normal (tracing.hlsl:107-116), get_fog (terrain.hlsl), get_pixel_ray (tracing.hlsl:124-134)
 * and get_color (color.hlsl) static, so this includes its source and calls them per element; likewise trace_ray
 * (tracing.hlsl:47-105) and the AA offset tables (antialiasing.hlsl:9-59) for tests/test_march_kat.py, and pcg_hash,
 * ao_dir, the AO factor and trace_sample for tests/test_ao_kat.py.  Built by tests/stage_ref.py with the oracle's
 * own flags.
 *
 * fr->eye is Eye, fr->sun SunDirection, fr->landscape, fr->recording, fr->width, fr->height, fr->projection and
 * fr->view_inverse the constants.  All arrays are interleaved per element.
 */
#include "../../oracle/rt_oracle.c"

/* pd: 4 floats an element (pos.xyz, density at pos); normals: 3 */
void st_normal(const ro_noise* nz, const ro_frame* fr, const float* pd, int64_t n, float* normals)
{
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n; ++i) {
        ctx c;
        ctx_init(&c, nz, fr);
        f4 q = {pd[4 * i], pd[4 * i + 1], pd[4 * i + 2], pd[4 * i + 3]};
        f3 r = get_normal(&c, q);
        normals[3 * i] = r.x; normals[3 * i + 1] = r.y; normals[3 * i + 2] = r.z;
    }
}

/* p: 3 floats, dist: 1, out: 4 (fog colour rgb, fog density) */
void st_fog(const ro_noise* nz, const ro_frame* fr, const float* p, const float* dist, int64_t n, float* out)
{
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) {
        ctx c;
        ctx_init(&c, nz, fr);
        f4 r = get_fog(&c, v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]), dist[i]);
        out[4 * i] = r.x; out[4 * i + 1] = r.y; out[4 * i + 2] = r.z; out[4 * i + 3] = r.w;
    }
}

/* pixel: 2 floats (x, y); outp, outdir: 3 each */
void st_pixel_ray(const ro_noise* nz, const ro_frame* fr, const float* pixel, int64_t n, float* outp, float* outdir)
{
    ctx c;
    ctx_init(&c, nz, fr);
    for (int64_t i = 0; i < n; ++i) {
        f3 p, d;
        get_pixel_ray(&c, pixel[2 * i], pixel[2 * i + 1], &p, &d);
        outp[3 * i] = p.x; outp[3 * i + 1] = p.y; outp[3 * i + 2] = p.z;
        outdir[3 * i] = d.x; outdir[3 * i + 1] = d.y; outdir[3 * i + 2] = d.z;
    }
}

/* traceRay (tracing.hlsl:47-105) with every argument the caller's own, for the march's known-answer tests
 * (tests/test_march_kat.py): p, dir 3 floats a ray; dist, enddist, stepmod 1 each; calcfog, skiprefine and the
 * build's max_steps (0: none) per call; fr->recording picks the constants.  pd, fcolord: 4 floats a ray. */
void st_trace_ray(const ro_noise* nz, const ro_frame* fr, const float* p, const float* dist, const float* enddist,
                  const float* stepmod, const float* dir, int64_t n, int calcfog, int skiprefine, int max_steps,
                  float* pd, float* fcolord, float* density, uint32_t* steps)
{
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n; ++i) {
        ctx c;
        ctx_init(&c, nz, fr);
        ray_result rr = trace_ray(&c, v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]), dist[i], enddist[i], stepmod[i],
                                  v3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]), calcfog, skiprefine, max_steps);
        pd[4 * i] = rr.pd.x; pd[4 * i + 1] = rr.pd.y; pd[4 * i + 2] = rr.pd.z; pd[4 * i + 3] = rr.pd.w;
        fcolord[4 * i] = rr.fcolord.x; fcolord[4 * i + 1] = rr.fcolord.y;
        fcolord[4 * i + 2] = rr.fcolord.z; fcolord[4 * i + 3] = rr.fcolord.w;
        density[i] = rr.density;
        steps[i] = (uint32_t)rr.steps;
    }
}

/* the stepmod of getColor's shadow ray (color.hlsl:47-50) for hits at dist */
void st_shadow_precision(const float* dist, int64_t n, float* out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = shadow_precision(dist[i]);
}

/* getSampleOffset(num) for AA_SAMPLES = samples (antialiasing.hlsl:9-59): the table ro_tracescreen selects, by its
 * own selector and its own division by 16.  out: 2 floats a sample; returns the sample count. */
int st_aa_offsets(int samples, float* out)
{
    int aa = samples;
    if (aa != 2 && aa != 4 && aa != 8 && aa != 16) aa = 1;
    const float (*offs)[2] = aa_table(aa);
    for (int a = 0; a < aa; ++a) {
        out[2 * a] = offs[a][0] * (1.0f / 16.0f);
        out[2 * a + 1] = offs[a][1] * (1.0f / 16.0f);
    }
    return aa;
}

/* The AO extension's pieces for tests/test_ao_kat.py: the hash ... */
void st_pcg_hash(const uint32_t* x, int64_t n, uint32_t* out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = pcg_hash(x[i]);
}

/* ... ao_dir for normals of 3 floats and keys of 4 uint32 (px, py, a, k) each; out: 3 floats ... */
void st_ao_dir(const float* nrm, const uint32_t* key, int64_t n, float* out)
{
    for (int64_t i = 0; i < n; ++i) {
        f3 d = ao_dir(v3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]), key[4 * i], key[4 * i + 1], key[4 * i + 2],
                      key[4 * i + 3]);
        out[3 * i] = d.x; out[3 * i + 1] = d.y; out[3 * i + 2] = d.z;
    }
}

/* ... and the factor of occ occluded rays of ao, by ambient_occlusion's own expression. */
float st_ao_factor(int occ, int ao)
{
    return fmaf(-RO_AO_STRENGTH, (float)occ * rcp((float)ao), 1.0f);
}

/* trace_sample (tracescreen.hlsl:16-48 and the AO extension) for n rays of the caller's own, as ro_tracescreen
 * calls it for the samples of a pixel: p, dir 3 floats a ray, range 2 (plane.x, plane.y), key 3 uint32 (px, py, a);
 * fr->ao_samples and fr->max_steps are the frame's.  color: 3 floats, NOT saturated; ao: trace_sample's factor (1
 * for a miss); pd: 4 floats, the primary march's rr.pd, and density its rr.density (the primary march once more,
 * as st_color repeats the shadow ray). */
void st_trace_samples(const ro_noise* nz, const ro_frame* fr, const float* p, const float* dir, const float* range,
                      const uint32_t* key, int64_t n, float* color, float* ao, float* pd, float* density)
{
    sky_consts k;
    sky_init(&k);
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n; ++i) {
        ctx c;
        ctx_init(&c, nz, fr);
        c.pixel_secondary_steps = 0.0f;
        const f3 pp = v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
        const f3 pdir = v3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
        float steps = 0.0f;
        uint64_t pst = 0, hits = 0, sst = 0, aost = 0, aor = 0;
        f3 s = trace_sample(&c, &k, pp, pdir, norm3(pdir), range[2 * i], range[2 * i + 1], &steps, &pst, &hits, &sst,
                            key[3 * i], key[3 * i + 1], key[3 * i + 2], &ao[i], &aost, &aor);
        color[3 * i] = s.x; color[3 * i + 1] = s.y; color[3 * i + 2] = s.z;
        ray_result rr = trace_ray(&c, pp, range[2 * i], range[2 * i + 1], 1.0f, pdir, 1, 0, fr->max_steps);
        pd[4 * i] = rr.pd.x; pd[4 * i + 1] = rr.pd.y; pd[4 * i + 2] = rr.pd.z; pd[4 * i + 3] = rr.pd.w;
        density[i] = rr.density;
    }
}

/* getColor(p, nrm, d, dist): p, nrm, d 3 floats each, dist 1; rgb: 3.  classes: 1 where the shadow ray ended in
 * the air (lit), 2 where it hit (shadowed); shadow_w: that ray's fcolord.w -- get_color's own shadow ray
 * (color.hlsl:47-51) once more, as tests/tools/shade_ref.c classifies. */
void st_color(const ro_noise* nz, const ro_frame* fr, const float* p, const float* nrm, const float* d,
              const float* dist, int64_t n, float* rgb, uint8_t* classes, float* shadow_w)
{
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n; ++i) {
        ctx c;
        ctx_init(&c, nz, fr);
        uint64_t shadow = 0;
        const f3 pos = v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
        f3 col = get_color(&c, pos, v3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]),
                           v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), dist[i], &shadow);
        rgb[3 * i] = col.x; rgb[3 * i + 1] = col.y; rgb[3 * i + 2] = col.z;
        ray_result sh = trace_ray(&c, pos, 0.4f, 100.0f, shadow_precision(dist[i]), c.sun, 1, 1, 0);
        classes[i] = sh.density > 0.0f ? 2 : 1;
        shadow_w[i] = sh.fcolord.w;
    }
}
