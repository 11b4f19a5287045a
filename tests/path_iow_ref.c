/*
 * path_iow_ref.c -- the reference for the IOW-03 path-query tests (rt_path_iow_rays_async /
 * rt_path_iow03): per query, the CPU oracle's own launch_rays() (rt_oracle.c: LaunchRays,
 * 03_Shadows_and_Materials/computeShaderSrc.glsl:285-358) on an iow_stack whose ri[] holds the
 * incoming state, for rgb, ri_out and the counts; and a restatement of that loop that also tracks
 * which slots the path wrote and which incoming RI values it read as a parent RI, for `stale`.
 *
 * The restatement cannot drift from the oracle's loop: a query is refused (non-zero return naming it)
 * unless its rgb, ri[], segments, drops and nans have the bits of launch_rays()'s.
 *
 * path_iow_camera() restates out_Pixel's camera ray (orc_render_iow03's inner loop) and writes the
 * queries of a w x h x spp frame in (y, x, s) order; tests/test_path_iow_ref.py folds their chained
 * answers and compares the frame with orc_render_iow03's, which checks it.
 *
 * Test infrastructure only: it builds on the oracle by including its source.
 * tests/golden/make_path_iow_golden.py compiles it to write the path_iow_*.npz fixtures,
 * tests/test_path_iow_ref.py compiles it again to recompute them.
 */
#include "../oracle/rt_oracle.c"

typedef struct { float o[3]; uint32_t sample; float d[3]; uint32_t pad; float ri_in[4]; } ref_ray;   /* rt_path_iow_ray */
typedef struct { float rgb[3]; uint32_t stale; uint32_t segments, drops, nans, status; float ri_out[4]; } ref_out; /* rt_path_iow_out */

/* launch_rays() (03.glsl:285-358) restated with the written / stale-read slot masks */
static v3 launch_rays_tracked(const iow_scene *S, iow_stack *K, v3 ro, v3 rd, int sidx, ctr *c, uint32_t *stale) {
    uint32_t wmask = 0, rmask = 0;
#define PUSH_T(r, cc, ri_, b) do { if (K->size < IOW_STACK) wmask |= 1u << K->size; iow_push(K, r, cc, ri_, b, c); } while (0)
    ray_t r0 = {ro, rd};
    PUSH_T(r0, 1.0f, 1.0f, 0);
    v3 sample = V3(0, 0, 0);
    int skip = 0;
    while (K->size > 0) {
        K->size--;
        float contribution = K->contrib[K->size], ri = K->ri[K->size];
        int bounced = K->bounce[K->size];
        ray_t cur = K->ray[K->size];
        rrd_t data = launch_ray(S, cur.o, cur.d, 32000.0f, contribution, c);
        int hit = dot(data.normal, data.normal) > 0.9f;
        sample = add(sample, mul(hit ? data.color : background(cur.d, 0), contribution));
        if (bounced < S->max_bounces && hit) {
            bounced++;
            int spawnRefl = 0, spawnRefr = 0;
            v3 refr_dir = V3(0, 0, 0), refl_dir = V3(0, 0, 0);
            float cos_t = dot(data.normal, cur.d);
            float sin_t = sqrtf(1.0f - cos_t * cos_t);
            float target_ri;
            {
                int pi = K->size - 1 - skip;
                float parent = (pi < 0) ? 1.0f : (pi < IOW_STACK ? K->ri[pi] : 0.0f);
                target_ri = cos_t > 0 ? parent : data.material.z;
                /* the incoming value of slot pi is used: the slot is read and this path has not written it */
                if (cos_t > 0 && pi >= 0 && pi < IOW_STACK && !((wmask >> pi) & 1u)) rmask |= 1u << pi;
            }
            float rr = (ri * rcp(target_ri)) * sin_t;
            float refr_c = data.material.x, refl_c = data.material.y;
            v3 n_ = cos_t > 0 ? data.normal : neg(data.normal);
            if (cos_t < 0) {
                refl_dir = fib_dir(S, sidx, data.scat[1], data.reflected); spawnRefl = 1;
                float inc = refr_c * schlick(-cos_t, ri * rcp(target_ri));
                refr_c -= inc; refl_c += inc;
            } else if (rr > 1.0f) {
                refr_dir = data.reflected; spawnRefl = 1; refl_c = 1.0f;
            }
            if (rr <= 1.0f) {
                v3 yc = mul(n_, cos_t), xc = sub(cur.d, yc);
                spawnRefr = 1;
                refr_dir = add(mul(n_, rr), mul(xc, sqrtf(1.0f - rr * rr)));
                refr_dir = fib_dir(S, sidx, data.scat[0], refr_dir);
            }
            skip = (spawnRefl && spawnRefr) ? skip - 1 : (spawnRefl ? skip : (spawnRefr ? skip + 1 : 0));
            if (spawnRefl) {
                ray_t nr = {sub(data.point, mul(n_, 0.000015f)), refl_dir};
                if (isnan(dot(refl_dir, refl_dir))) c->nans++;
                PUSH_T(nr, contribution * refl_c, ri, bounced);
            }
            if (spawnRefr) {
                ray_t nr = {add(data.point, mul(n_, 0.000015f)), refr_dir};
                if (isnan(dot(refr_dir, refr_dir))) c->nans++;
                PUSH_T(nr, contribution * refr_c, target_ri, bounced);
            }
        } else skip = 0;
    }
#undef PUSH_T
    *stale = rmask;
    return sample;
}

/* out[q] as rt_path_iow_rays_async defines them; ctr3 (may be NULL) += segments, drops, nans.
 * Returns 0, -1 for bad arguments, or 1 + the index of the first query on which the restated loop and
 * launch_rays() disagree. */
int path_iow_ref(const float *types, const float *rec, uint32_t n, int spp, int max_bounces, const ref_ray *rays,
                 uint32_t n_rays, uint32_t chain, ref_out *out, uint64_t *ctr3) {
    if (!types || !rec || n == 0 || spp < 1 || max_bounces < 0 || chain == 0 || (n_rays && (!rays || !out)))
        return -1;
    float *fb = (float *)malloc(sizeof(float) * 3 * (size_t)spp);
    orc_sample_tables(spp, NULL, fb, NULL);
    iow_scene S = {types, rec, n, NULL, fb, NULL, spp, max_bounces};
    int rc = 0;
    float state[IOW_STACK] = {0, 0, 0, 0};
    for (uint32_t q = 0; q < n_rays && rc == 0; q++) {
        const ref_ray *r = rays + q;
        ref_out *o = out + q;
        memset(o, 0, sizeof(*o));
        if (q % chain == 0) memcpy(state, r->ri_in, sizeof(state));  /* else the predecessor's outgoing state */
        if (r->sample >= (uint32_t)spp) {
            o->status = 1;
            memcpy(o->ri_out, state, sizeof(state));
            continue;
        }
        const v3 ro = V3(r->o[0], r->o[1], r->o[2]), rd = V3(r->d[0], r->d[1], r->d[2]);
        iow_stack K, K2;
        memset(&K, 0, sizeof(K));
        memcpy(K.ri, state, sizeof(state));
        K2 = K;
        ctr c = {0, 0, 0, 0, 0, 0}, c2 = {0, 0, 0, 0, 0, 0};
        const v3 rgb = launch_rays(&S, &K, ro, rd, (int)r->sample, &c);
        uint32_t stale = 0;
        const v3 rgb2 = launch_rays_tracked(&S, &K2, ro, rd, (int)r->sample, &c2, &stale);
        if (memcmp(&rgb.x, &rgb2.x, 4) || memcmp(&rgb.y, &rgb2.y, 4) || memcmp(&rgb.z, &rgb2.z, 4) ||
            memcmp(K.ri, K2.ri, sizeof(K.ri)) || c.seg != c2.seg || c.drops != c2.drops || c.nans != c2.nans ||
            K.size != 0 || K2.size != 0) {
            rc = 1 + (int)q;
            break;
        }
        o->rgb[0] = rgb.x; o->rgb[1] = rgb.y; o->rgb[2] = rgb.z;
        o->stale = stale;
        o->segments = (uint32_t)c.seg; o->drops = (uint32_t)c.drops; o->nans = (uint32_t)c.nans;
        memcpy(o->ri_out, K.ri, sizeof(state));
        memcpy(state, K.ri, sizeof(state));
        if (ctr3) { ctr3[0] += c.seg; ctr3[1] += c.drops; ctr3[2] += c.nans; }
    }
    free(fb);
    return rc;
}

/* The camera rays of out_Pixel (03.glsl:362-418, as orc_render_iow03 restates it) for a W x H frame of
 * spp samples, as queries in (y, x, s) order with ri_in = 0.  A sample whose ring entry is the
 * early-return marker (03.glsl:396) gets sample = 0xffffffff and a zero ray: the shader stops the
 * pixel there, and so does the fold of the answers. */
int path_iow_camera(const orc_camera *cam, int W, int H, int spp, ref_ray *rays) {
    if (!cam || !rays || W <= 0 || H <= 0 || spp < 1) return -1;
    float *sf = (float *)malloc(sizeof(float) * 2 * (size_t)spp);
    int *ring = (int *)malloc(sizeof(int) * 2 * (size_t)spp);
    orc_sample_tables(spp, sf, NULL, ring);
    const v3 D = V3(cam->dir[0], cam->dir[1], cam->dir[2]);
    const v3 P = V3(cam->pos[0], cam->pos[1], cam->pos[2]);
    const float sd = 1.0f / (2.0f * (float)tan((double)(cam->fov_y_rad * 0.5f)));
    int grid = 1;
    while (grid * grid < spp) grid++;
    for (int yy = 0; yy < H; yy++) {
        for (int xx = 0; xx < W; xx++) {
            float aspect = (float)W * rcp((float)H);
            float sx = (aspect * ((float)xx * 2.0f - (float)W)) * rcp(2.0f * (float)W);
            float sy = ((float)yy * 2.0f - (float)H) * rcp(2.0f * (float)H);
            float dsx = aspect * rcp((float)(W * grid));
            float dsy = 1.0f * rcp((float)(H * grid));
            v3 look_at = add(P, mul(D, cam->focus_dist));
            v3 up = V3(0, 1, 0);
            v3 cr = cross(D, up), cu = cross(cr, D);
            for (int s = 0; s < spp; s++) {
                ref_ray *r = rays + ((size_t)yy * W + xx) * spp + s;
                memset(r, 0, sizeof(*r));
                int ix = ring[2 * s], iy = ring[2 * s + 1];
                if (ix < 0) { r->sample = 0xffffffffu; continue; }
                float rx = (sf[2 * s] * cam->aperture) * 0.5f, ry = (sf[2 * s + 1] * cam->aperture) * 0.5f;
                v3 ro = add(add(P, mul(cr, rx)), mul(cu, ry));
                v3 ld = normalize(sub(look_at, ro));
                v3 r_ = cross(ld, up), u_ = cross(cr, ld);
                v3 rd = normalize(add(add(mul(ld, sd), mul(r_, sx + dsx * (float)ix)),
                                      mul(u_, sy + dsy * (float)iy)));
                r->o[0] = ro.x; r->o[1] = ro.y; r->o[2] = ro.z;
                r->d[0] = rd.x; r->d[1] = rd.y; r->d[2] = rd.z;
                r->sample = (uint32_t)s;
            }
        }
    }
    free(sf); free(ring);
    return 0;
}
