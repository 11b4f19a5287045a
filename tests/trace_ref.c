/*
 * trace_ref.c -- the reference for the ray-query tests (rt_trace_rays_async / rt_trace_inw): per
 * query, the CPU oracle's own closest-hit walk (traverse(), rt_oracle.c: 01_BVH...glsl:431-473 /
 * 04...glsl:524-563 with IntersectRay) on an empty 40-float stack, with t_limiting = tmax, the
 * query's time ratio and the child order of the invert flag.
 *
 * Test infrastructure only: it builds on the oracle by including its source, so the walk is the
 * very function the render parity tests check.  tests/golden/make_trace_golden.py compiles it to
 * write the trace_*.npz fixtures, tests/test_trace_ref.py compiles it again to recompute them.
 */
#include "../oracle/rt_oracle.c"

typedef struct { float o[3]; float tmax; float d[3]; float ratio; } ref_ray;                 /* rt_ray */
typedef struct { float t; int32_t id; float n[3]; float extra; uint32_t pad[2]; } ref_hit;   /* rt_hit */

/* hits[q] as rt_trace_rays_async defines them; counters = {node visits, primitive tests, dropped
 * pushes} summed over the queries with tmax > 0 (the others are misses by the walk's own tests, and
 * the product may skip their walk). */
int trace_ref(const float *geom, uint32_t n, int layout, const float *nodes, const ref_ray *rays, uint32_t n_rays,
              int invert, ref_hit *hits, uint64_t counters[3]) {
    if (!geom || !nodes || n == 0 || (n_rays && (!rays || !hits)) || !counters) return -1;
    inw_scene S;
    memset(&S, 0, sizeof(S));
    S.geom = geom; S.nodes = nodes; S.n = n; S.layout = layout; S.spp = 1;
    S.camdir = invert ? V3(1, 1, 1) : V3(-1, -1, -1);  /* traverse: invert = dot(camdir, (1,1,1)) > 0 */
    counters[0] = counters[1] = counters[2] = 0;
    for (uint32_t q = 0; q < n_rays; q++) {
        const ref_ray *r = rays + q;
        fstack K;
        memset(&K, 0, sizeof(K));
        ray_t ray = {V3(r->o[0], r->o[1], r->o[2]), V3(r->d[0], r->d[1], r->d[2])};
        float tlim = r->tmax, extra = 0.0f;
        v3 normal = V3(0, 0, 0);
        ctr c = {0, 0, 0, 0, 0, 0};
        const float g = traverse(&S, &K, ray, r->ratio, &tlim, &normal, &extra, -1.0f, 0, &c);
        ref_hit *h = hits + q;
        memset(h, 0, sizeof(*h));
        if (tlim < r->tmax) {
            h->t = tlim; h->id = (int32_t)g;
            h->n[0] = normal.x; h->n[1] = normal.y; h->n[2] = normal.z;
            h->extra = extra;
        } else {
            h->t = r->tmax; h->id = -1;
        }
        if (r->tmax > 0.0f) { counters[0] += c.nodes; counters[1] += c.prims; counters[2] += c.drops; }
    }
    return 0;
}
