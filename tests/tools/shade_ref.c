/*
 * shade_ref.c -- TEST INFRASTRUCTURE: the checker of the shaded queries (rt_terrain_shade_rays,
 * include/frosttrace.h).  The oracle shades the pixel rays of a camera only, so this includes the oracle's source
 * and evaluates the header's definition for rays of the caller's own from the oracle's static functions:
 * trace_ray (tracing.hlsl:47-105), get_normal (:107-116), get_color (color.hlsl, with its shadow ray),
 * get_rayleigh_mie and get_space_color (sky.hlsl).  Built by tests/shade_ref.py with the oracle's own flags.
 *
 * Ray i: origins / dirs xyz interleaved; ranges (2n: t_min_i, t_max_i) or NULL for t_min / t_max.  fr->eye is E
 * (the density's, the normal's and the sky's Eye), fr->sun, fr->landscape and fr->recording the constants;
 * fr->aa_samples, fr->max_steps and fr->ao_samples are not read.
 * results: 8 floats a ray (colour rgb NOT saturated, pd.w | pd.xyz, density); rgba8: unorm8(saturate(colour)),
 * R in the low byte, alpha 255; steps: 2 a ray (primary, shadow iterations).  For the tests' own census, each
 * optional: classes (0 a miss, 1 a lit hit, 2 a shadowed hit), fog_w (the primary march's fcolord.w) and fog_rgb
 * (3 a ray: its fcolord.rgb).
 *
 * sr_trace_sample is the oracle's own trace_sample (tracescreen.hlsl:16-48) for the same rays, stepmod 1 as it
 * has it, with fr->ao_samples = 0 and fr->max_steps as the cap: what pins sr_shade_rays.
 */
#include "../../oracle/rt_oracle.c"

void sr_shade_rays(const ro_noise* nz, const ro_frame* fr, const float* origins, const float* dirs,
                   const float* ranges, int64_t n, float t_min, float t_max, float stepmod, int max_steps,
                   float* results, uint32_t* rgba8, uint32_t* steps, uint8_t* classes, float* fog_w, float* fog_rgb)
{
    sky_consts k;
    sky_init(&k);
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n; ++i) {
        ctx c;
        ctx_init(&c, nz, fr);
        const float t0 = ranges ? ranges[2 * i] : t_min, t1 = ranges ? ranges[2 * i + 1] : t_max;
        const f3 dir = v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
        const f3 pdn = norm3(dir);
        ray_result rr = trace_ray(&c, v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]), t0, t1, stepmod, dir,
                                  1, 0, max_steps);
        float skyAmount = rr.pd.w * 0.0005f;
        skyAmount = sat(skyAmount * skyAmount);
        sky_color scat = get_rayleigh_mie(&c, &k, pdn);
        uint64_t shadow = 0;
        f3 color;
        if (rr.density > 0.0f) {
            f4 npd = {rr.pd.x, rr.pd.y, rr.pd.z, rr.density};
            f3 nrm = get_normal(&c, npd);
            color = get_color(&c, v3(rr.pd.x, rr.pd.y, rr.pd.z), nrm, pdn, rr.pd.w, &shadow);
            color = v3(lerp(color.x, rr.fcolord.x, rr.fcolord.w), lerp(color.y, rr.fcolord.y, rr.fcolord.w),
                       lerp(color.z, rr.fcolord.z, rr.fcolord.w));
            color = v3(lerp(color.x, scat.rayleigh.x, skyAmount), lerp(color.y, scat.rayleigh.y, skyAmount),
                       lerp(color.z, scat.rayleigh.z, skyAmount));
        } else {
            float space = get_space_color(&c, pdn);
            f3 sky = v3((scat.mie.x + scat.rayleigh.x) + space, (scat.mie.y + scat.rayleigh.y) + space,
                        (scat.mie.z + scat.rayleigh.z) + space);
            color = v3(lerp(sky.x, rr.fcolord.x, rr.fcolord.w), lerp(sky.y, rr.fcolord.y, rr.fcolord.w),
                       lerp(sky.z, rr.fcolord.z, rr.fcolord.w));
            color = v3(lerp(color.x, sky.x, skyAmount), lerp(color.y, sky.y, skyAmount), lerp(color.z, sky.z, skyAmount));
        }
        float* r = results + 8 * i;
        r[0] = color.x; r[1] = color.y; r[2] = color.z; r[3] = rr.pd.w;
        r[4] = rr.pd.x; r[5] = rr.pd.y; r[6] = rr.pd.z; r[7] = rr.density;
        rgba8[i] = (uint32_t)unorm8(color.x) | (uint32_t)unorm8(color.y) << 8 | (uint32_t)unorm8(color.z) << 16 | 0xff000000u;
        steps[2 * i] = (uint32_t)rr.steps;
        steps[2 * i + 1] = (uint32_t)shadow;
        if (fog_w) fog_w[i] = rr.fcolord.w; /* the primary's */
        if (fog_rgb) { fog_rgb[3 * i] = rr.fcolord.x; fog_rgb[3 * i + 1] = rr.fcolord.y; fog_rgb[3 * i + 2] = rr.fcolord.z; }
        if (classes) { /* 0 a miss, 1 a lit hit, 2 a shadowed hit: get_color's shadow ray once more */
            classes[i] = 0;
            if (rr.density > 0.0f) {
                ray_result sh = trace_ray(&c, v3(rr.pd.x, rr.pd.y, rr.pd.z), 0.4f, 100.0f, shadow_precision(rr.pd.w),
                                          c.sun, 1, 1, 0);
                classes[i] = sh.density > 0.0f ? 2 : 1;
            }
        }
    }
}

void sr_trace_sample(const ro_noise* nz, const ro_frame* fr, const float* origins, const float* dirs,
                     const float* ranges, int64_t n, float t_min, float t_max, float* colors, uint32_t* steps)
{
    sky_consts k;
    sky_init(&k);
    ro_frame f0 = *fr;
    f0.ao_samples = 0;
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n; ++i) {
        ctx c;
        ctx_init(&c, nz, &f0);
        const float t0 = ranges ? ranges[2 * i] : t_min, t1 = ranges ? ranges[2 * i + 1] : t_max;
        const f3 dir = v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
        float psteps = 0.0f, ao = 1.0f;
        uint64_t prim = 0, hits = 0, shadow = 0, aost = 0, aor = 0;
        f3 s = trace_sample(&c, &k, v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]), dir, norm3(dir), t0, t1,
                            &psteps, &prim, &hits, &shadow, 0u, 0u, 0u, &ao, &aost, &aor);
        colors[3 * i] = s.x; colors[3 * i + 1] = s.y; colors[3 * i + 2] = s.z;
        steps[2 * i] = (uint32_t)prim;
        steps[2 * i + 1] = (uint32_t)shadow;
    }
}
