/*
 * surface_ref.c -- TEST INFRASTRUCTURE: the checker of the surface queries (rt_terrain_trace_surface,
 * include/frosttrace.h).  The oracle exports no refined march for rays of the caller's own, so this includes
 * the oracle's source and calls its static trace_ray (tracing.hlsl:47-105, calcfog 0, skiprefine 0) and
 * get_normal (tracing.hlsl:107-116) per ray.  Built by tests/surface_ref.py with the oracle's own flags.
 *
 * Ray i: origins / dirs xyz interleaved; ranges (2n: t_min_i, t_max_i) or NULL for t_min / t_max.  fr->eye is
 * the LOD eye (getDensity's Eye and getNormal's), fr->landscape and fr->recording the constants.
 * results: 8 floats a ray (pd.xyz, pd.w | n.xyz, density), n = 0 where density <= 0; steps: loop iterations.
 */
#include "../../oracle/rt_oracle.c"

void sr_trace_surface(const ro_noise* nz, const ro_frame* fr, const float* origins, const float* dirs,
                      const float* ranges, int64_t n, float t_min, float t_max, float stepmod, int max_steps,
                      float* results, uint32_t* steps)
{
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n; ++i) {
        ctx c;
        ctx_init(&c, nz, fr);
        const float t0 = ranges ? ranges[2 * i] : t_min, t1 = ranges ? ranges[2 * i + 1] : t_max;
        ray_result rr = trace_ray(&c, v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]), t0, t1, stepmod,
                                  v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]), 0, 0, max_steps);
        f3 nrm = v3(0.0f, 0.0f, 0.0f);
        if (rr.density > 0.0f) {
            f4 pd = {rr.pd.x, rr.pd.y, rr.pd.z, rr.density};
            nrm = get_normal(&c, pd);
        }
        float* r = results + 8 * i;
        r[0] = rr.pd.x; r[1] = rr.pd.y; r[2] = rr.pd.z; r[3] = rr.pd.w;
        r[4] = nrm.x; r[5] = nrm.y; r[6] = nrm.z; r[7] = rr.density;
        steps[i] = (uint32_t)rr.steps;
    }
}
