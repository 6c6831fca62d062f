/*
 * stage_ref.c -- TEST INFRASTRUCTURE: the oracle's shading stages at inputs of the caller's own, for the
 * known-answer tests against the float64 restatement of the HLSL (tests/hlsl_ref.py, tests/test_hlsl_kat.py).
 * The oracle keeps get_normal (tracing.hlsl:107-116), get_fog (terrain.hlsl), get_pixel_ray (tracing.hlsl:124-134)
 * and get_color (color.hlsl) static, so this includes its source and calls them per element.  Built by
 * tests/stage_ref.py with the oracle's own flags.
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
