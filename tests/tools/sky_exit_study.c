/*
 * sky_exit_study.c -- DIAGNOSTIC (not product, not the checker): the primary march samples of the oracle,
 * per pixel, for counting what k_trace's sky exit (rt_shader.h sky_exit) leaves out.  Each sample of a
 * primary ray (the refining march: skiprefine off) is recorded as three floats: its height p.y, its density d
 * and the noise3d calls it cost (octaves + the steep noise).  tests/tools/sky_exit_study.py builds this with
 * the oracle's own source included and does the counting.
 */
#define RO_STUDY 1
#include "../../oracle/rt_oracle.c"

typedef struct { float* v; int64_t n, cap; } buff;
static buff* g_pix = NULL;
static int64_t g_npix = 0;

void st_config(int64_t npix)
{
    for (int64_t i = 0; i < g_npix; ++i) free(g_pix[i].v);
    free(g_pix);
    g_npix = npix;
    g_pix = (buff*)calloc((size_t)npix, sizeof(buff));
}

int64_t st_pixel_len(int64_t i) { return g_pix[i].n; }
const float* st_pixel_data(int64_t i) { return g_pix[i].v; }

static void ro_study_sample(ctx* c, f3 p, float d, int calcfog, int skiprefine, int max_steps, int iters,
                            float dist, float enddist, float step, float lastStep)
{
    (void)calcfog; (void)max_steps; (void)iters; (void)dist; (void)enddist; (void)step; (void)lastStep;
    if (c->fr->landscape != RO_NOMADPLAINS || skiprefine) return;
    if (c->study_pixel < 0 || c->study_pixel >= g_npix) return;
    float dd = ro_max(len3(sub3(p, c->eye)), 0.01f);
    float detail = ro_max(18.0f - ro_pow(dd, 0.33f), 2.0f);
    int n = 0;
    for (int N = 1; (float)N <= detail; ++N) n = N;
    buff* b = &g_pix[c->study_pixel]; /* one thread per row: no two threads share a pixel */
    if (b->n + 3 > b->cap) {
        b->cap = b->cap ? b->cap * 2 : 96;
        b->v = (float*)realloc(b->v, (size_t)b->cap * sizeof(float));
    }
    b->v[b->n++] = p.y;
    b->v[b->n++] = d;
    b->v[b->n++] = (float)(n + 1);
}
