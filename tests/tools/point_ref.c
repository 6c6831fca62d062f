/*
 * point_ref.c -- TEST INFRASTRUCTURE: the checker of point shading (rt_terrain_shade_points,
 * include/frosttrace.h).  The oracle shades the pixel rays of a camera only, so this includes the oracle's source
 * and evaluates the header's definition for points and normals of the caller's own from the oracle's static
 * functions: get_color (color.hlsl, with its shadow ray) and ambient_occlusion (the AO extension), with
 * ao_samples set on a copy of the frame.  Built by tests/point_ref.py with the oracle's own flags.
 *
 * Point i: points / normals xyz interleaved (3n floats each).  fr->eye is E (the density's Eye and the
 * viewpoint), fr->sun, fr->landscape and fr->recording the constants; fr->aa_samples, fr->max_steps and
 * fr->ao_samples are not read.
 * results: 4 floats a point (colour rgb NOT saturated, ao); rgba8: unorm8(saturate(colour) * ao), R in the low
 * byte, alpha 255; steps: 2 a point (shadow iterations, the AO rays' sum).  For the tests' own census, each
 * optional: classes (1 lit, 2 shadowed), occ (the occluded AO rays), view (4 a point: pdn, dist as the
 * definition recomputes them from p - E).
 *
 * What pins pr_shade_points (tests/test_point_query_host.py): pr_primary is the oracle's own primary march and
 * get_normal for rays (trace_sample's first lines), pr_trace_sample the oracle's own trace_sample with
 * ao_samples = K and (px, py, a) = (i, seed, 0), pr_get_color and pr_ambient_occlusion its get_color and
 * ambient_occlusion at a given (pdn, dist), pr_blend trace_sample's two lerps, pr_norm_len its norm3 / len3 and
 * pr_precision its shadow_precision.
 */
#include "../../oracle/rt_oracle.c"

void pr_shade_points(const ro_noise* nz, const ro_frame* fr, const float* points, const float* normals, int64_t n,
                     int ao_samples, uint32_t seed, float* results, uint32_t* rgba8, uint32_t* steps, uint8_t* classes,
                     uint32_t* occ, float* view)
{
    ro_frame f0 = *fr;
    f0.ao_samples = ao_samples;
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n; ++i) {
        ctx c;
        ctx_init(&c, nz, &f0);
        const f3 p = v3(points[3 * i], points[3 * i + 1], points[3 * i + 2]);
        const f3 nrm = v3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]);
        const f3 v = sub3(p, c.eye);
        const float dist = len3(v);
        const f3 pdn = norm3(v);
        uint64_t shadow = 0, aost = 0, aor = 0;
        const f3 color = get_color(&c, p, nrm, pdn, dist, &shadow);
        float ao = 1.0f;
        if (ao_samples > 0) ao = ambient_occlusion(&c, p, nrm, dist, (uint32_t)i, seed, 0u, &aost, &aor);
        float* r = results + 4 * i;
        r[0] = color.x; r[1] = color.y; r[2] = color.z; r[3] = ao;
        rgba8[i] = (uint32_t)unorm8(sat(color.x) * ao) | (uint32_t)unorm8(sat(color.y) * ao) << 8 |
                   (uint32_t)unorm8(sat(color.z) * ao) << 16 | 0xff000000u;
        steps[2 * i] = (uint32_t)shadow;
        steps[2 * i + 1] = (uint32_t)aost;
        if (view) { view[4 * i] = pdn.x; view[4 * i + 1] = pdn.y; view[4 * i + 2] = pdn.z; view[4 * i + 3] = dist; }
        if (classes) { /* 1 lit, 2 shadowed: get_color's shadow ray once more */
            ray_result sh = trace_ray(&c, p, 0.4f, 100.0f, shadow_precision(dist), c.sun, 1, 1, 0);
            classes[i] = sh.density > 0.0f ? 2 : 1;
        }
        if (occ) { /* ambient_occlusion's rays once more */
            uint32_t o = 0;
            for (int k = 0; k < ao_samples; ++k) {
                ray_result rr = trace_ray(&c, p, 0.4f, RO_AO_END, shadow_precision(dist),
                                          ao_dir(nrm, (uint32_t)i, seed, 0u, (uint32_t)k), 0, 1, 0);
                if (rr.density > 0.0f) o += 1;
            }
            occ[i] = o;
        }
    }
}

/* trace_sample's first lines for ray i: pd (4), normal and density (4; the normal 0 for a miss), fcolord (4),
 * scat.rayleigh (3) and pdn (3) */
void pr_primary(const ro_noise* nz, const ro_frame* fr, const float* origins, const float* dirs, int64_t n, float t_min,
                float t_max, float* pd, float* nd, float* fc, float* ray, float* pdn_out)
{
    sky_consts k;
    sky_init(&k);
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n; ++i) {
        ctx c;
        ctx_init(&c, nz, fr);
        const f3 dir = v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
        const f3 pdn = norm3(dir);
        ray_result rr = trace_ray(&c, v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]), t_min, t_max, 1.0f, dir,
                                  1, 0, fr->max_steps);
        sky_color scat = get_rayleigh_mie(&c, &k, pdn);
        f3 nrm = v3(0.0f, 0.0f, 0.0f);
        if (rr.density > 0.0f) {
            f4 npd = {rr.pd.x, rr.pd.y, rr.pd.z, rr.density};
            nrm = get_normal(&c, npd);
        }
        pd[4 * i] = rr.pd.x; pd[4 * i + 1] = rr.pd.y; pd[4 * i + 2] = rr.pd.z; pd[4 * i + 3] = rr.pd.w;
        nd[4 * i] = nrm.x; nd[4 * i + 1] = nrm.y; nd[4 * i + 2] = nrm.z; nd[4 * i + 3] = rr.density;
        fc[4 * i] = rr.fcolord.x; fc[4 * i + 1] = rr.fcolord.y; fc[4 * i + 2] = rr.fcolord.z; fc[4 * i + 3] = rr.fcolord.w;
        ray[3 * i] = scat.rayleigh.x; ray[3 * i + 1] = scat.rayleigh.y; ray[3 * i + 2] = scat.rayleigh.z;
        pdn_out[3 * i] = pdn.x; pdn_out[3 * i + 1] = pdn.y; pdn_out[3 * i + 2] = pdn.z;
    }
}

/* the oracle's own trace_sample for ray i with fr->ao_samples = ao_samples and (px, py, a) = (i, seed, 0):
 * colours (3), ao, steps (3: primary, shadow, AO) */
void pr_trace_sample(const ro_noise* nz, const ro_frame* fr, const float* origins, const float* dirs, int64_t n,
                     float t_min, float t_max, int ao_samples, uint32_t seed, float* colors, float* ao_out,
                     uint32_t* steps)
{
    sky_consts k;
    sky_init(&k);
    ro_frame f0 = *fr;
    f0.ao_samples = ao_samples;
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n; ++i) {
        ctx c;
        ctx_init(&c, nz, &f0);
        const f3 dir = v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
        float psteps = 0.0f, ao = 1.0f;
        uint64_t prim = 0, hits = 0, shadow = 0, aost = 0, aor = 0;
        f3 s = trace_sample(&c, &k, v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]), dir, norm3(dir), t_min,
                            t_max, &psteps, &prim, &hits, &shadow, (uint32_t)i, seed, 0u, &ao, &aost, &aor);
        colors[3 * i] = s.x; colors[3 * i + 1] = s.y; colors[3 * i + 2] = s.z;
        ao_out[i] = ao;
        steps[3 * i] = (uint32_t)prim;
        steps[3 * i + 1] = (uint32_t)shadow;
        steps[3 * i + 2] = (uint32_t)aost;
    }
}

/* the oracle's get_color at a given viewpoint term: colours (3), shadow iterations */
void pr_get_color(const ro_noise* nz, const ro_frame* fr, const float* points, const float* normals, const float* pdn,
                  const float* dist, int64_t n, float* colors, uint32_t* shadow_steps)
{
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n; ++i) {
        ctx c;
        ctx_init(&c, nz, fr);
        uint64_t shadow = 0;
        f3 s = get_color(&c, v3(points[3 * i], points[3 * i + 1], points[3 * i + 2]),
                         v3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]),
                         v3(pdn[3 * i], pdn[3 * i + 1], pdn[3 * i + 2]), dist[i], &shadow);
        colors[3 * i] = s.x; colors[3 * i + 1] = s.y; colors[3 * i + 2] = s.z;
        shadow_steps[i] = (uint32_t)shadow;
    }
}

/* the oracle's ambient_occlusion with fr->ao_samples = ao_samples and (px, py, a) = (i, seed, 0) at a given dist:
 * ao, the AO rays' iterations */
void pr_ambient_occlusion(const ro_noise* nz, const ro_frame* fr, const float* points, const float* normals,
                          const float* dist, int64_t n, int ao_samples, uint32_t seed, float* ao_out, uint32_t* ao_steps)
{
    ro_frame f0 = *fr;
    f0.ao_samples = ao_samples;
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n; ++i) {
        ctx c;
        ctx_init(&c, nz, &f0);
        uint64_t aost = 0, aor = 0;
        ao_out[i] = ambient_occlusion(&c, v3(points[3 * i], points[3 * i + 1], points[3 * i + 2]),
                                      v3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]), dist[i], (uint32_t)i,
                                      seed, 0u, &aost, &aor);
        ao_steps[i] = (uint32_t)aost;
    }
}

/* trace_sample's two lerps for a hit (tracescreen.hlsl:33-35): colours (3), the primary's pd.w, fcolord (4) and
 * scat.rayleigh (3) */
void pr_blend(const float* colors, const float* pdw, const float* fc, const float* ray, int64_t n, float* out)
{
    for (int64_t i = 0; i < n; ++i) {
        float skyAmount = pdw[i] * 0.0005f;
        skyAmount = sat(skyAmount * skyAmount);
        f3 color = v3(colors[3 * i], colors[3 * i + 1], colors[3 * i + 2]);
        color = v3(lerp(color.x, fc[4 * i], fc[4 * i + 3]), lerp(color.y, fc[4 * i + 1], fc[4 * i + 3]),
                   lerp(color.z, fc[4 * i + 2], fc[4 * i + 3]));
        color = v3(lerp(color.x, ray[3 * i], skyAmount), lerp(color.y, ray[3 * i + 1], skyAmount),
                   lerp(color.z, ray[3 * i + 2], skyAmount));
        out[3 * i] = color.x; out[3 * i + 1] = color.y; out[3 * i + 2] = color.z;
    }
}

/* norm3 and len3 of v (3 a vector): out 4 a vector */
void pr_norm_len(const float* v, int64_t n, float* out)
{
    for (int64_t i = 0; i < n; ++i) {
        const f3 a = v3(v[3 * i], v[3 * i + 1], v[3 * i + 2]);
        const f3 u = norm3(a);
        out[4 * i] = u.x; out[4 * i + 1] = u.y; out[4 * i + 2] = u.z; out[4 * i + 3] = len3(a);
    }
}

void pr_precision(const float* dist, int64_t n, float* out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = shadow_precision(dist[i]);
}
