// rt_beam_prune.hpp -- which culling-BVH leaves a pixel's beam list keeps (DESIGN.md §5.2 "Pixel
// beams", rt_options.inw_beam_prune): the beam's geometry as the host derives it from the camera
// (beam_geom, what set_beam gives k_inw_beam) and the keep / drop predicate, one function for the
// device (k_inw_beam) and the host (rt_beam_keep_host, the CPU tests).  Plain floats and doubles,
// no device types, so a host compiler takes it as it is.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_BEAM_HD __host__ __device__
#else
#define RT_BEAM_HD
#endif

namespace rtk {

// The extra argument of k_inw_beam.  A pixel's primary rays leave a tip within d0 of C0 = co + cd
// and pass through F = C0 + L * cd, L in [1 / inv_ll, 1 / inv_lh] (rounding of the focus and of cd),
// so at central parameter t they lie within d0 * |1 - t / L| + slack of the central ray; R is
// that bound over the scene's whole range [tmin, tfar] (InwScene::beam_R, beam_tmin, beam_tfar).
struct BeamPrune {
    uint32_t mode = 0;  // 0: the R-inflated lists; 1: + the boxes re-tested with their own radius; 2: + swept spheres
    uint32_t bins = 1;  // time bins of the lists (1: one list over the whole shutter interval)
    float d0 = 0.0f, inv_ll = 0.0f, inv_lh = 0.0f, slack = 0.0f;
    float R = 0.0f, tmin = 0.0f, tfar = 0.0f;
};

// set_beam's geometry.  false: no beam lists for this camera (the focal point too close to the lens).
struct BeamGeom {
    double d0, Ll, Lh, tmin, tfar, slack, R, kappa;
};
inline bool beam_geom(const float pos[3], float aperture, float focus, float sf_max, float wbound, BeamGeom &g) {
    const double ap = fabs(double(aperture)), L = double(focus) - 1.0;
    g.d0 = 0.5 * ap * double(sf_max) * (1.0 + 1e-4) + 1e-6;
    if (!(L > 8.0 * g.d0 + 1e-3)) return false;
    const double cam = sqrt(double(pos[0]) * pos[0] + double(pos[1]) * pos[1] + double(pos[2]) * pos[2]);
    g.Lh = L + 1e-3 * (1.0 + cam);
    g.Ll = L - 1e-3 * (1.0 + cam);
    if (!(g.Ll > 4.0 * g.d0)) return false;
    // every point of a culling box lies within sqrt(3) * wbound of the origin
    g.tfar = (cam + 1.0 + sqrt(3.0) * double(wbound) + 2.0) / (1.0 - g.d0 / g.Ll) * 1.001;
    g.tmin = -g.Lh / (g.Ll - g.d0) - 0.01;
    const double r = g.d0 * fmax(1.0 - g.tmin / g.Ll, fabs(1.0 - g.tfar / g.Ll));
    g.slack = 2e-3 + 1e-5 * (cam + g.tfar);
    g.R = r + 2e-3 + 1e-5 * (cam + g.tfar);
    g.kappa = g.Lh / (g.Ll - g.d0) * (1.0 + 1e-5);
    return true;
}
inline BeamPrune beam_prune_of(const BeamGeom &g, int mode, uint32_t bins) {
    BeamPrune p;
    p.mode = mode < 0 ? 0u : uint32_t(mode);
    p.bins = bins > 1u ? bins : 1u;
    // rounded to float away from the exact value on the conservative side
    p.d0 = nextafterf(float(g.d0), INFINITY);
    p.inv_ll = nextafterf(float(1.0 / g.Ll), INFINITY);
    p.inv_lh = nextafterf(float(1.0 / g.Lh), 0.0f);
    p.slack = nextafterf(float(g.slack), INFINITY);
    p.R = float(g.R);
    p.tmin = float(g.tmin);
    p.tfar = float(g.tfar);
    return p;
}

// Entry and exit of the central ray o + t * cd (id = 1 / cd, neg[a] = cd[a] < 0) for the box with
// near / far planes nr / fr inflated outward by r: k_inw_beam's slab test, the same float operations.
RT_BEAM_HD inline void beam_slab(const float nr[3], const float fr[3], const float o[3], const float id[3],
                                 const bool neg[3], float r, float &te, float &tx) {
    const float rx = neg[0] ? r : -r, ry = neg[1] ? r : -r, rz = neg[2] ? r : -r;
    te = fmaxf(fmaxf(((nr[0] + rx) - o[0]) * id[0], ((nr[1] + ry) - o[1]) * id[1]), ((nr[2] + rz) - o[2]) * id[2]);
    tx = fminf(fminf(((fr[0] - rx) - o[0]) * id[0], ((fr[1] - ry) - o[1]) * id[1]), ((fr[2] - rz) - o[2]) * id[2]);
}

// Step 1, the box's own radius.  [te, tx] is the central ray's interval in the box inflated by R;
// every point where a primary ray of the pixel touches the box has its central parameter in
// [ta, tb] = [max(te, tmin), min(tx, tfar)], and |1 - t / L| is convex in t, so the beam is no
// wider there than at the interval's ends: the radius returned (rounded up, at most R).
RT_BEAM_HD inline float beam_box_radius(const BeamPrune &P, float te, float tx) {
    const float ta = fmaxf(te, P.tmin), tb = fminf(tx, P.tfar);
    const float m = fmaxf(fmaxf(fabsf(1.0f - ta * P.inv_ll), fabsf(1.0f - ta * P.inv_lh)),
                          fmaxf(fabsf(1.0f - tb * P.inv_ll), fabsf(1.0f - tb * P.inv_lh)));
    const float r = (P.d0 * m) * 1.00001f + P.slack;
    return r < P.R ? r : P.R;  // (a NaN keeps R)
}
// ... and the box re-tested with it: false when the central ray misses the box inflated by that
// radius, so no primary ray of the pixel touches the box.  A NaN keeps the box.
RT_BEAM_HD inline bool beam_box_keep(const BeamPrune &P, const float nr[3], const float fr[3], const float o[3],
                                     const float id[3], const bool neg[3], float te, float tx) {
    const float r = beam_box_radius(P, te, tx);
    if (!(r < P.R)) return true;
    float te2, tx2;
    beam_slab(nr, fr, o, id, neg, r, te2, tx2);
    return !(fmaxf(te2, P.tmin) > fminf(tx2, P.tfar));
}

// Step 2, the swept sphere (sphere records: p = (position, RN(1 / scale)), q = position -
// last_position).  A ray with time ratio r in bin b of K meets the sphere of radius rho = 1 / p[3]
// around c(r) = p - q * (1 - r), r in [b / K, (b + 1) / K] (widened by 1e-4 for the rounding of
// r * K; r itself lies in [0, 1]).  A hit point H of a primary ray lies within rho of c(r) and
// within the beam's radius of the central line, so the line passes the segment of centres within
// rho + radius.  The radius is the beam's over the central parameters such an H can have: within
// (rho + R) of the projections of the segment's ends, cut to [tmin, tfar].  In double; two terms
// cover the float test that decides a hit (t_ellipsoid on the object-space ray):
//  - its determinant hb^2 - a * c carries an absolute error below 24 * 2^-24 * a * A^2, A the scaled
//    distance from the ray's origin to the centre, so it can report a hit up to
//    sqrt(rho^2 + 24 * 2^-24 * D^2) from the centre (D that distance; 32 taken);
//  - the object-space origin (o - p) + q * (1 - r) is rounded three times: 1e-6 * D.
// Anything not finite keeps the sphere.
RT_BEAM_HD inline bool beam_sphere_keep(const BeamPrune &P, const float o[3], const float cd[3], const float p[4],
                                        const float q[3], uint32_t bin) {
    const double K = double(P.bins), r0 = double(bin) / K - 1e-4, r1 = double(bin + 1u) / K + 1e-4;
    const double cc = double(cd[0]) * cd[0] + double(cd[1]) * cd[1] + double(cd[2]) * cd[2];
    const double rho = fabs(1.0 / double(p[3])) * (1.0 + 1e-6);
    if (!(cc > 0.0) || !(rho < 1e30)) return true;
    double w0[3], w1[3], t0 = 0.0, t1 = 0.0, D2 = 0.0;
    for (int e = 0; e < 2; e++) {
        const double k = 1.0 - (e ? r1 : r0);
        const double v[3] = {(double(p[0]) - double(q[0]) * k) - o[0], (double(p[1]) - double(q[1]) * k) - o[1],
                             (double(p[2]) - double(q[2]) * k) - o[2]};
        const double t = (v[0] * cd[0] + v[1] * cd[1] + v[2] * cd[2]) / cc;
        double *w = e ? w1 : w0;
        for (int a = 0; a < 3; a++) w[a] = v[a] - t * double(cd[a]);  // the part across the central line
        (e ? t1 : t0) = t;
        D2 = fmax(D2, v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    }
    const double b[3] = {w1[0] - w0[0], w1[1] - w0[1], w1[2] - w0[2]};
    const double bb = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
    double s = bb > 0.0 ? -(w0[0] * b[0] + w0[1] * b[1] + w0[2] * b[2]) / bb : 0.0;  // a stationary sphere: bb = 0
    s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
    const double x[3] = {w0[0] + s * b[0], w0[1] + s * b[1], w0[2] + s * b[2]};
    const double dist2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
    const double D = sqrt(D2) + 1.0 + double(P.d0) + 1e-3;  // the ray starts one unit behind its tip
    const double rho_e = sqrt(rho * rho + (32.0 / 16777216.0) * D * D);
    // the beam's radius where such a hit can lie
    const double nc = sqrt(cc), reach = (rho_e + double(P.R)) / nc * (1.0 + 1e-6) + 1e-6;
    const double ta = fmax(fmin(t0, t1) - reach, double(P.tmin)), tb = fmin(fmax(t0, t1) + reach, double(P.tfar));
    if (!(ta <= tb)) return true;
    const double m = fmax(fmax(fabs(1.0 - ta * double(P.inv_ll)), fabs(1.0 - ta * double(P.inv_lh))),
                          fmax(fabs(1.0 - tb * double(P.inv_ll)), fabs(1.0 - tb * double(P.inv_lh))));
    const double rad = fmin(double(P.d0) * m * (1.0 + 1e-6) + double(P.slack), double(P.R));
    const double thr = rho_e + rad + 1e-6 * D;
    return !(dist2 > thr * thr);
}

}  // namespace rtk
