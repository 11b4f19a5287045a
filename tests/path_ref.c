/*
 * path_ref.c -- the reference for the path-query tests (rt_path_rays_async / rt_path_inw): per
 * query, the CPU oracle's sample loop (inw_sample's `while (K.size > 0)`, rt_oracle.c: out_Pixel's
 * ray loop, 01_BVH...glsl:414-597 / 04...glsl:510-713) restated to start from a given ray on an
 * empty 40-float stack, the MULTIFOCUS lines dropped; and the camera ray of (px, py, s) formed as
 * inw_sample forms it for the single-focus camera, so that the restated loop can be checked
 * against inw_sample itself.
 *
 * Test infrastructure only: it builds on the oracle by including its source, so the walks, the
 * stack, the materials and the textures are the very functions the render parity tests check.
 * tests/golden/make_path_golden.py compiles it to write the paths_*.npz fixtures,
 * tests/test_path_ref.py compiles it again to recompute them.
 */
#include "../oracle/rt_oracle.c"

typedef struct { float o[3]; uint32_t sample; float d[3]; uint32_t pad; } ref_path_ray;                     /* rt_path_ray */
typedef struct { float rgb[3]; float depth; uint32_t segments, drops, nans, status; } ref_path_out;         /* rt_path_out */

/* the ray loop of inw_sample from the ray `start`, sample index s */
static void path_loop(const inw_scene *S, ray_t start, int s, v3 *out_color, float *out_depth, ctr *c) {
    fstack K;
    K.size = 0;
    K.data[0] = 0;
    v3 color = V3(0, 0, 0);
    float depth = 0.0f;
    const float ratio = (float)s * rcp((float)S->spp);
    stk_push_ray(&K, start, 1.0f, 0.0f, c);
    const int L4 = S->layout == 4;
    while (K.size > 0) {
        v3 normal = V3(0, 0, 0), hitpoint;
        float contribution, bounced, surr = 0.0f;
        float m_ri = 0, m_refr = 0, m_refl = 0, m_srfr = 0, m_srfl = 0;
        v3 m_color = V3(0, 0, 0);
        v3 incoming;
        ray_t cur;
        {
            K.size -= 8;
            float *d = K.data + K.size;
            cur.o = V3(d[0], d[1], d[2]); cur.d = V3(d[3], d[4], d[5]);
            contribution = d[6]; bounced = (float)(int)d[7];
        }
        c->seg++;
        const float tlim0 = MAX_T_DEPTH;
        float tlim = tlim0;
        float extra = 0.0f;
        float fg = traverse(S, &K, cur, ratio, &tlim, &normal, &extra, L4 ? -1.0f : 0.0f, 0, c);
        incoming = cur.d;
        hitpoint = add(cur.o, mul(cur.d, tlim));
        if (tlim < tlim0) {
            const float *f = S->geom + (size_t)fg * 28;
            if (!L4) {
                m_ri = f[20]; m_refr = f[21]; m_refl = f[22]; m_srfr = f[23]; m_srfl = f[24];
                m_color = V3(f[25], f[26], f[27]);
            } else {
                m_ri = extra; m_refr = f[20]; m_refl = f[21]; m_srfr = f[22]; m_srfl = f[23];
                m_color = V3(f[24], f[25], f[26]);
                const uint32_t ti = f2u(f[27] + 0.1f);
                if (ti > 0 && ti <= S->n_tex) {
                    const xform_t x = fetch_xform(S, (int)fg);
                    m_color = mulv(m_color, tex_color(S->tex + (ti - 1), m3tmul(x.R, sub(hitpoint, x.pos))));
                }
            }
            surr = surrounding_ri(S, &K, add(hitpoint, mul(normal, 0.001f)), ratio, c);
        } else {
            color = add(color, mul(background(cur.d, L4 && S->n_lights > 0), contribution));
            depth = tlim;
            continue;
        }
        if (L4) {
            uint32_t is_lit = S->n_lights > 0 ? 0u : (uint32_t)is_lit_geom(S, f2u(fg + 0.1f));
            if (is_lit == 0) {
                for (uint32_t i = 0; i < S->n_lights; i++) {
                    const float *lt = S->lights + (size_t)i * 7;
                    v3 bmin = V3(lt[0], lt[1], lt[2]), bmax = V3(lt[3], lt[4], lt[5]);
                    ray_t sr;
                    sr.o = add(hitpoint, mul(normal, 0.0001f));
                    float sl = length(sub(mul(add(bmax, bmin), 0.5f), sr.o)) + length(sub(bmax, bmin));
                    sr.d = normalize(sub(add(bmin, mul(sub(bmax, bmin), ratio)), sr.o));
                    c->shadow++;
                    float sg = traverse(S, &K, sr, ratio, &sl, NULL, NULL, -1.0f, 1, c);
                    is_lit += (uint32_t)is_lit_geom(S, f2u(sg + 0.1f));
                }
                uint32_t nl = S->n_lights > 1 ? S->n_lights : 1u;
                contribution *= (float)is_lit * rcp((float)nl);
            } else {
                color = V3(1, 1, 1);
                K.size = 0;
                break;
            }
        }
        int bounce_ok;
        if (!L4) { bounced += 1.0f; bounce_ok = bounced < (float)S->max_bounces; }
        else bounce_ok = bounced < (float)S->max_bounces;
        if ((m_refl > 0.002f || m_refr > 0.002f) && contribution > 0.01f && bounce_ok) {
            if (L4) bounced += 1.0f;
            v3 refl = V3(0, 0, 0), refr = V3(0, 0, 0);
            int inner = dot(normal, incoming) > 0;
            if (!inner) {
                if (m_refl > 0.002f) {
                    refl = normalize(reflect3(incoming, normal));
                    if (m_srfl > 0.001f) refl = deviate(S, refl, m_srfl, s);
                }
                if (m_refr > 0.002f) {
                    refr = normalize(refract3(incoming, normal, surr * rcp(m_ri)));
                    if (m_srfr > 0.001f) refr = deviate(S, refr, m_srfr, s);
                }
            } else {
                normal = mul(normal, -1.0f);
                refr = refract3(incoming, normal, m_ri * rcp(surr));
                if (dot(refr, refr) < 0.1f) refl = reflect3(incoming, normal);
            }
            float carried = 0.0f;
            float rr2 = dot(refr, refr);
            if (isnan(rr2)) c->nans++;
            if (rr2 > 0.1f) {
                ray_t nr = {sub(hitpoint, mul(normal, 0.0001f)), refr};
                carried += m_refr;
                stk_push_ray(&K, nr, contribution * m_refr, bounced, c);
            }
            if (dot(refl, refl) > 0.1f) {
                ray_t nr = {add(hitpoint, mul(normal, 0.0001f)), refl};
                carried += m_refl;
                stk_push_ray(&K, nr, contribution * m_refl, bounced, c);
            }
            contribution *= (1.0f - 0.5f * carried);
        }
        color = add(color, mul(m_color, contribution));
    }
    *out_color = color;
    *out_depth = depth;
}

static void path_scene(inw_scene *S, const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                       uint32_t n_lights, const orc_texture *tex, uint32_t n_tex, int spp, int max_bounces,
                       const float *sf, v3 camdir) {
    memset(S, 0, sizeof(*S));
    S->geom = geom; S->nodes = nodes; S->lights = lights; S->n = n; S->n_lights = layout == 4 ? n_lights : 0;
    S->layout = layout; S->spp = spp; S->max_bounces = max_bounces; S->sf = sf;
    S->camdir = camdir;
    S->tex = layout == 4 ? tex : NULL;
    S->n_tex = layout == 4 ? n_tex : 0;
    S->n_focus = 0;
}

/* out[q] as rt_path_rays_async defines them; counters = the six rt_stats counts summed over the
 * queries with sample < spp */
int path_ref(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights, uint32_t n_lights,
             const orc_texture *tex, uint32_t n_tex, int spp, int max_bounces, const ref_path_ray *rays,
             uint32_t n_rays, int invert, ref_path_out *out, uint64_t counters[6]) {
    if (!geom || !nodes || n == 0 || spp < 1 || (n_rays && (!rays || !out)) || !counters) return -1;
    float *sf = (float *)malloc(sizeof(float) * 2 * (size_t)spp);
    orc_sample_tables(spp, sf, NULL, NULL);
    inw_scene S;
    path_scene(&S, geom, n, layout, nodes, lights, n_lights, tex, n_tex, spp, max_bounces, sf,
               invert ? V3(1, 1, 1) : V3(-1, -1, -1));  /* traverse: invert = dot(camdir, (1,1,1)) > 0 */
    ctr total = {0, 0, 0, 0, 0, 0};
    for (uint32_t q = 0; q < n_rays; q++) {
        const ref_path_ray *r = rays + q;
        ref_path_out *o = out + q;
        memset(o, 0, sizeof(*o));
        if (r->sample >= (uint32_t)spp) { o->status = 1; continue; }
        ray_t ray = {V3(r->o[0], r->o[1], r->o[2]), V3(r->d[0], r->d[1], r->d[2])};
        ctr c = {0, 0, 0, 0, 0, 0};
        v3 col; float dep;
        path_loop(&S, ray, (int)r->sample, &col, &dep, &c);
        o->rgb[0] = col.x; o->rgb[1] = col.y; o->rgb[2] = col.z; o->depth = dep;
        o->segments = (uint32_t)c.seg; o->drops = (uint32_t)c.drops; o->nans = (uint32_t)c.nans;
        total.seg += c.seg; total.nodes += c.nodes; total.prims += c.prims;
        total.shadow += c.shadow; total.drops += c.drops; total.nans += c.nans;
    }
    free(sf);
    counters[0] = total.seg; counters[1] = total.nodes; counters[2] = total.prims;
    counters[3] = total.shadow; counters[4] = total.drops; counters[5] = total.nans;
    return 0;
}

/* The camera rays of pixels [0, W) x [0, H), samples [0, spp), as inw_sample forms them for the
 * single-focus camera (BVH.glsl:366-410), in the order (y, x, s): rays[(y * W + x) * spp + s]. */
int path_camera_rays(const orc_camera *cam, int W, int H, int spp, ref_path_ray *rays) {
    if (!cam || !rays || W <= 0 || H <= 0 || spp < 1) return -1;
    float *sf = (float *)malloc(sizeof(float) * 2 * (size_t)spp);
    orc_sample_tables(spp, sf, NULL, NULL);
    const float sd = 1.0f / (2.0f * (float)tan((double)(cam->fov_y_rad * 0.5f)));
    const v3 D = V3(cam->dir[0], cam->dir[1], cam->dir[2]);
    const v3 campos = V3(cam->pos[0], cam->pos[1], cam->pos[2]);
    for (int py = 0; py < H; py++)
        for (int px = 0; px < W; px++)
            for (int s = 0; s < spp; s++) {
                float aspect = (float)W * rcp((float)H);
                float srx = (float)px * rcp((float)W) - 0.5f;
                float sry = (float)py * rcp((float)H) - 0.5f;
                srx *= aspect;
                v3 up = V3(0, 1, 0);
                v3 cr = cross(D, up), cu = cross(cr, D);
                ray_t c;
                c.o = campos;
                c.d = normalize(add(add(mul(D, sd), mul(cr, srx)), mul(cu, sry)));
                float ox = sf[2 * s] * (cam->aperture * 0.5f), oy = sf[2 * s + 1] * (cam->aperture * 0.5f);
                v3 rr = cross(c.d, up), ru = cross(rr, c.d);
                v3 tip = add(add(add(c.o, c.d), mul(rr, ox)), mul(ru, oy));
                v3 la = normalize(sub(add(c.o, mul(c.d, cam->focus_dist)), tip));
                c.o = sub(tip, la);
                c.d = la;
                ref_path_ray *r = rays + ((size_t)py * W + px) * spp + s;
                r->o[0] = c.o.x; r->o[1] = c.o.y; r->o[2] = c.o.z; r->sample = (uint32_t)s;
                r->d[0] = c.d.x; r->d[1] = c.d.y; r->d[2] = c.d.z; r->pad = 0;
            }
    free(sf);
    return 0;
}

/* inw_sample itself for every (y, x, s) of a W x H frame, in path_camera_rays' order: the sample's
 * colour, depth and per-sample counts as path_ref reports them; counters = the six totals. */
int path_inw_samples(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                     uint32_t n_lights, const orc_texture *tex, uint32_t n_tex, const orc_camera *cam, int W, int H,
                     int spp, int max_bounces, ref_path_out *out, uint64_t counters[6]) {
    if (!geom || !nodes || n == 0 || !cam || !out || !counters || W <= 0 || H <= 0 || spp < 1) return -1;
    float *sf = (float *)malloc(sizeof(float) * 2 * (size_t)spp);
    orc_sample_tables(spp, sf, NULL, NULL);
    inw_scene S;
    path_scene(&S, geom, n, layout, nodes, lights, n_lights, tex, n_tex, spp, max_bounces, sf,
               V3(cam->dir[0], cam->dir[1], cam->dir[2]));
    const float sd = 1.0f / (2.0f * (float)tan((double)(cam->fov_y_rad * 0.5f)));
    const v3 P = V3(cam->pos[0], cam->pos[1], cam->pos[2]);
    ctr total = {0, 0, 0, 0, 0, 0};
    for (int py = 0; py < H; py++)
        for (int px = 0; px < W; px++)
            for (int s = 0; s < spp; s++) {
                ctr c = {0, 0, 0, 0, 0, 0};
                v3 col; float dep;
                inw_sample(&S, px, py, W, H, sd, P, cam->fov_y_rad, cam->aperture, cam->focus_dist, s, &col, &dep, &c);
                ref_path_out *o = out + ((size_t)py * W + px) * spp + s;
                memset(o, 0, sizeof(*o));
                o->rgb[0] = col.x; o->rgb[1] = col.y; o->rgb[2] = col.z; o->depth = dep;
                o->segments = (uint32_t)c.seg; o->drops = (uint32_t)c.drops; o->nans = (uint32_t)c.nans;
                total.seg += c.seg; total.nodes += c.nodes; total.prims += c.prims;
                total.shadow += c.shadow; total.drops += c.drops; total.nans += c.nans;
            }
    free(sf);
    counters[0] = total.seg; counters[1] = total.nodes; counters[2] = total.prims;
    counters[3] = total.shadow; counters[4] = total.drops; counters[5] = total.nans;
    return 0;
}
