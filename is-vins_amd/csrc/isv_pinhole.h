// isv_pinhole.h -- PinholeCamera::liftProjective (PinholeCamera.cc:461-521, :657-673) for the kernels that lift pixel coordinates:
// k_kf_brief (isv_keyframe.hip), k_trk_track (isv_tracker.hip) and k_rej_f (isv_reject.hip).  Doubles, in the reference's operation
// order, contraction off: the CPU restatements (tests/native/isv_kf_oracle.c, isv_trk_oracle.c) give the same bits.  The last
// section is plain C that compiles as HIP device code or as host C: tests/native/isv_rej_oracle.c includes this file.
#pragma once
#ifdef __clang__
#pragma clang fp contract(off)
#endif
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PINHOLE_HD static __device__ __forceinline__
#else
#define PINHOLE_HD static inline
#endif

typedef struct PinholeCam {       // PinholeCamera's members, formed once at creation
    double inv_K11, inv_K13, inv_K22, inv_K23, k1, k2, p1, p2;
    int32_t no_distortion, pad;
} PinholeCam;

// PinholeCamera::PinholeCamera / setParameters: m_inv_K11 = 1.0 / fx, m_inv_K13 = -cx / fx, m_inv_K22, m_inv_K23, m_noDistortion
static inline PinholeCam pinhole_make(double fx, double fy, double cx, double cy, double k1, double k2, double p1, double p2) {
    PinholeCam c;
    c.inv_K11 = 1.0 / fx; c.inv_K13 = -cx / fx; c.inv_K22 = 1.0 / fy; c.inv_K23 = -cy / fy;
    c.k1 = k1; c.k2 = k2; c.p1 = p1; c.p2 = p2;
    c.no_distortion = (k1 == 0.0 && k2 == 0.0 && p1 == 0.0 && p2 == 0.0) ? 1 : 0;
    c.pad = 0;
    return c;
}

#if defined(__HIPCC__)
__device__ __forceinline__ void pinhole_distortion(const PinholeCam &c, double x, double y, double *dx, double *dy) {
    const double mx2_u = x * x, my2_u = y * y, mxy_u = x * y, rho2_u = mx2_u + my2_u;
    const double rad_dist_u = c.k1 * rho2_u + c.k2 * rho2_u * rho2_u;
    *dx = x * rad_dist_u + 2.0 * c.p1 * mxy_u + c.p2 * (rho2_u + 2.0 * mx2_u);
    *dy = y * rad_dist_u + 2.0 * c.p2 * mxy_u + c.p1 * (rho2_u + 2.0 * my2_u);
}

// liftProjective of the pixel (px, py): out = ((float)(mx_u / 1.0), (float)(my_u / 1.0))
__device__ __forceinline__ void pinhole_lift(const PinholeCam &cam, float px, float py, float *ox, float *oy) {
    const double mx_d = cam.inv_K11 * (double)px + cam.inv_K13, my_d = cam.inv_K22 * (double)py + cam.inv_K23;
    double mx_u = mx_d, my_u = my_d;
    if (!cam.no_distortion) {
        double dx, dy;
        pinhole_distortion(cam, mx_d, my_d, &dx, &dy);
        mx_u = mx_d - dx; my_u = my_d - dy;
        for (int it = 1; it < 8; it++) {
            pinhole_distortion(cam, mx_u, my_u, &dx, &dy);
            mx_u = mx_d - dx; my_u = my_d - dy;
        }
    }
    *ox = (float)(mx_u / 1.0); *oy = (float)(my_u / 1.0);
}
#endif

// ---- plain C, device or host: the same operations with the lifted point left in doubles (P = (mx_u, my_u, 1.0)) ----
PINHOLE_HD void pinhole_distortion_c(const PinholeCam *c, double x, double y, double *dx, double *dy) {
    const double mx2_u = x * x, my2_u = y * y, mxy_u = x * y, rho2_u = mx2_u + my2_u;
    const double rad_dist_u = c->k1 * rho2_u + c->k2 * rho2_u * rho2_u;
    *dx = x * rad_dist_u + 2.0 * c->p1 * mxy_u + c->p2 * (rho2_u + 2.0 * mx2_u);
    *dy = y * rad_dist_u + 2.0 * c->p2 * mxy_u + c->p1 * (rho2_u + 2.0 * my2_u);
}

PINHOLE_HD void pinhole_lift_d(const PinholeCam *cam, double px, double py, double *bx, double *by) {
    const double mx_d = cam->inv_K11 * px + cam->inv_K13, my_d = cam->inv_K22 * py + cam->inv_K23;
    double mx_u = mx_d, my_u = my_d;
    if (!cam->no_distortion) {
        double dx, dy;
        pinhole_distortion_c(cam, mx_d, my_d, &dx, &dy);
        mx_u = mx_d - dx; my_u = my_d - dy;
        for (int it = 1; it < 8; it++) {
            pinhole_distortion_c(cam, mx_u, my_u, &dx, &dy);
            mx_u = mx_d - dx; my_u = my_d - dy;
        }
    }
    *bx = mx_u; *by = my_u;
}
