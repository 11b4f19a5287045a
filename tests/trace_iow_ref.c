/*
 * trace_iow_ref.c -- the reference for the IOW-03 ray-query tests (rt_trace_iow_rays_async /
 * rt_trace_iow03): per query, the CPU oracle's own launch_ray() (rt_oracle.c: LaunchRay,
 * 03_Shadows_and_Materials/computeShaderSrc.glsl:196-256) with max_t = tmax for the payload (normal,
 * material), and a restated loop over the oracle's t_ray_obj with the shader's rule
 * (min_t > t && t > 0) for (t, id), which launch_ray does not return.
 *
 * The restated loop cannot drift from the oracle's: a query is refused (non-zero return) unless
 * launch_ray().point has the bits of o + d * t, its material.z those of the winner's record float 20,
 * or both report a miss.
 *
 * Test infrastructure only: it builds on the oracle by including its source.
 * tests/golden/make_trace_iow_golden.py compiles it to write the trace_iow_*.npz fixtures,
 * tests/test_trace_iow_ref.py compiles it again to recompute them.
 */
#include "../oracle/rt_oracle.c"

typedef struct { float o[3]; float tmax; float d[3]; float ratio; } ref_ray;                 /* rt_ray */
typedef struct { float t; int32_t id; float n[3]; float extra; uint32_t pad[2]; } ref_hit;   /* rt_hit */

static int same_v3(v3 a, v3 b) { return memcmp(&a.x, &b.x, 4) == 0 && memcmp(&a.y, &b.y, 4) == 0 && memcmp(&a.z, &b.z, 4) == 0; }

/* hits[q] as rt_trace_iow_rays_async defines them.  Returns 0, -1 for bad arguments, or 1 + the index
 * of the first query on which the restated loop and launch_ray() disagree. */
int trace_iow_ref(const float *types, const float *rec, uint32_t n, const ref_ray *rays, uint32_t n_rays,
                  ref_hit *hits) {
    if (!types || !rec || n == 0 || (n_rays && (!rays || !hits))) return -1;
    iow_scene S;
    memset(&S, 0, sizeof(S));
    S.types = types; S.rec = rec; S.n = n; S.spp = 1;
    for (uint32_t q = 0; q < n_rays; q++) {
        const ref_ray *r = rays + q;
        const v3 go = V3(r->o[0], r->o[1], r->o[2]), gd = V3(r->d[0], r->d[1], r->d[2]);
        ctr c = {0, 0, 0, 0, 0, 0};
        const rrd_t data = launch_ray(&S, go, gd, r->tmax, 1.0f, &c);
        /* the same loop for (t, id): 03...glsl:200-226 */
        float min_t = r->tmax;
        int32_t best = -1;
        for (uint32_t j = 0; j < n; j++) {
            const int type = (int)types[j];
            const float *R = rec + (size_t)j * 24;
            const m3 M = rec_m3(R + 3);
            const ray_t tr = {m3mul(M, sub(go, V3(R[0], R[1], R[2]))), normalize(m3mul(M, gd))};
            const int t3 = type == IOW_ELLIPSOID ? 2 : (type == IOW_CUBOID ? 1 : 0);
            const float t = t_ray_obj(tr, t3, V3(R[12], R[13], R[14]));
            if (min_t > t && t > 0) { min_t = t; best = (int32_t)j; }
        }
        ref_hit *h = hits + q;
        memset(h, 0, sizeof(*h));
        if (min_t < r->tmax) {
            const float ri = rec[(size_t)best * 24 + 20];
            if (!same_v3(data.point, add(go, mul(gd, min_t))) || memcmp(&data.material.z, &ri, 4) != 0)
                return 1 + (int)q;
            h->t = min_t; h->id = best;
            h->n[0] = data.normal.x; h->n[1] = data.normal.y; h->n[2] = data.normal.z;
            h->extra = data.material.z;
        } else {
            if (!same_v3(data.point, V3(0, 0, 0)) || !same_v3(data.normal, V3(0, 0, 0))) return 1 + (int)q;
            h->t = r->tmax; h->id = -1;
        }
    }
    return 0;
}
