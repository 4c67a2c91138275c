/* isv_det_oracle.c -- the serial CPU restatement of include/isvins_detect.h: FeatureTracker::setMask and cv::goodFeaturesToTrack
 * (blockSize 3, Sobel 3, minimum eigenvalue) as that header states them, one item at a time on one image, written for clarity.
 * The kernels of is-vins_amd/csrc/isv_detect.hip are pinned to it bit for bit; tests/test_det_oracle.py pins it independently
 * against numpy statements of the definitions.  Built by tests/det_oracle.py with -ffp-contract=off.
 *
 *   setMask (feature_tracker_simple.cpp:37-69)          det_set_mask
 *   cv::circle, thickness -1 (drawing.cpp, Circle)      isvo_det_disc: the midpoint recurrence itself, row by row
 *   cornerMinEigenVal(3, 3) (corner.cpp)                isvo_det_sums, isvo_det_response
 *   minMaxLoc, threshold, dilate, the candidate loop,   isvo_det_detect: a sort of all candidates, then every accepted corner is
 *   the sort and the minimum distance (featureselect)   tested, no cell grid
 *   liftProjective (PinholeCamera.cc:461-521)           isvo_det_lift
 * isvo_det_detect also counts what happened (C_* below), so that the tests can assert that a scenario reaches its condition.
 * There are no slots here: the image comes with the call.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "isvins_detect.h"

enum { C_DROPPED, C_CLIPPED, C_CANDIDATES, C_REJECTED, C_CAP_REACHED, C_TIE_PAIRS, C_PLATEAU, C_MASKED, C_COUNT };

int isvo_det_sizeof(int i) {
    switch (i) {
    case 0: return (int)sizeof(isv_det_config_t);
    case 1: return (int)sizeof(isv_det_item_t);
    case 2: return (int)sizeof(isv_det_result_t);
    default: return -1;
    }
}

/* BORDER_REFLECT_101 (cv::borderInterpolate), the general loop */
static int reflect101(int p, int len) {
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}

static void fill_row(uint8_t *mask, int W, int H, int y, int xa, int xb, int *clipped) {
    if (y < 0 || y >= H) { *clipped = 1; return; }
    if (xa < 0) { xa = 0; *clipped = 1; }
    if (xb > W - 1) { xb = W - 1; *clipped = 1; }
    for (int x = xa; x <= xb; x++) mask[(size_t)y * W + x] = 0;
}

/* cv::circle(mask, (cx, cy), r, 0, -1): the midpoint raster.  Returns 1 if the image clipped it. */
int isvo_det_disc(uint8_t *mask, int W, int H, int cx, int cy, int r) {
    int err = 0, dx = r, dy = 0, plus = 1, minus = 2 * r - 1, clipped = 0;
    while (dx >= dy) {
        fill_row(mask, W, H, cy - dy, cx - dx, cx + dx, &clipped);
        fill_row(mask, W, H, cy + dy, cx - dx, cx + dx, &clipped);
        fill_row(mask, W, H, cy - dx, cx - dy, cx + dy, &clipped);
        fill_row(mask, W, H, cy + dx, cx - dy, cx + dy, &clipped);
        dy++; err += plus; plus += 2;
        if (err > 0) { err -= minus; dx--; minus -= 2; }
    }
    return clipped;
}

static int pixel(const uint8_t *img, int W, int H, int stride, int x, int y) {
    return img[(size_t)reflect101(y, H) * stride + reflect101(x, W)];
}

/* The 3 x 3 Sobel pair at every pixel and the unnormalised 3 x 3 box sums of their products; each [H][W] (any may be NULL). */
void isvo_det_sums(const uint8_t *img, int W, int H, int stride, int32_t *Dx, int32_t *Dy, int32_t *Sxx, int32_t *Sxy, int32_t *Syy) {
    const size_t n = (size_t)W * H;
    int32_t *dx = malloc(n * sizeof(int32_t)), *dy = malloc(n * sizeof(int32_t));
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            int gx = 0, gy = 0;
            for (int j = -1; j <= 1; j++) {
                const int w = j == 0 ? 2 : 1;
                gx += w * (pixel(img, W, H, stride, x + 1, y + j) - pixel(img, W, H, stride, x - 1, y + j));
                gy += w * (pixel(img, W, H, stride, x + j, y + 1) - pixel(img, W, H, stride, x + j, y - 1));
            }
            dx[(size_t)y * W + x] = gx; dy[(size_t)y * W + x] = gy;
        }
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            int32_t sxx = 0, sxy = 0, syy = 0;
            for (int j = -1; j <= 1; j++)
                for (int i = -1; i <= 1; i++) {
                    const size_t q = (size_t)reflect101(y + j, H) * W + reflect101(x + i, W);      /* the covariance images' border */
                    sxx += dx[q] * dx[q]; sxy += dx[q] * dy[q]; syy += dy[q] * dy[q];
                }
            const size_t p = (size_t)y * W + x;
            if (Sxx) Sxx[p] = sxx;
            if (Sxy) Sxy[p] = sxy;
            if (Syy) Syy[p] = syy;
        }
    if (Dx) memcpy(Dx, dx, n * sizeof(int32_t));
    if (Dy) memcpy(Dy, dy, n * sizeof(int32_t));
    free(dx); free(dy);
}

/* cornerMinEigenVal(image, eig, 3, 3): eig [H][W] */
void isvo_det_response(const uint8_t *img, int W, int H, int stride, float *eig) {
    const size_t n = (size_t)W * H;
    int32_t *sxx = malloc(n * sizeof(int32_t)), *sxy = malloc(n * sizeof(int32_t)), *syy = malloc(n * sizeof(int32_t));
    isvo_det_sums(img, W, H, stride, NULL, NULL, sxx, sxy, syy);
    const float k = (float)(1.0 / (3060.0 * 3060.0));
    for (size_t p = 0; p < n; p++) {
        const float a = (float)sxx[p] * k * 0.5f, b = (float)sxy[p] * k, c = (float)syy[p] * k * 0.5f;
        const float d = (a - c) * (a - c) + b * b;
        eig[p] = (a + c) - (float)sqrt((double)d);
    }
    free(sxx); free(sxy); free(syy);
}

static void distortion(const isv_trk_config_t *c, double x, double y, double *dx, double *dy) {
    const double k1 = c->k1, k2 = c->k2, p1 = c->p1, p2 = c->p2;
    const double mx2_u = x * x, my2_u = y * y, mxy_u = x * y, rho2_u = mx2_u + my2_u;
    const double rad_dist_u = k1 * rho2_u + k2 * rho2_u * rho2_u;
    *dx = x * rad_dist_u + 2.0 * p1 * mxy_u + p2 * (rho2_u + 2.0 * mx2_u);
    *dy = y * rad_dist_u + 2.0 * p2 * mxy_u + p1 * (rho2_u + 2.0 * my2_u);
}

/* liftProjective of (u, v) and feature_tracker_simple.cpp:207: out = (float)(x / z), (float)(y / z) with z = 1.0 */
void isvo_det_lift(const isv_trk_config_t *c, float u, float v, float out[2]) {
    const double m_inv_K11 = 1.0 / c->fx, m_inv_K13 = -c->cx / c->fx, m_inv_K22 = 1.0 / c->fy, m_inv_K23 = -c->cy / c->fy;
    const int m_noDistortion = c->k1 == 0.0 && c->k2 == 0.0 && c->p1 == 0.0 && c->p2 == 0.0;
    const double mx_d = m_inv_K11 * (double)u + m_inv_K13, my_d = m_inv_K22 * (double)v + m_inv_K23;
    double mx_u, my_u;
    if (m_noDistortion) {
        mx_u = mx_d; my_u = my_d;
    } else {
        const int n = 8;
        double dx, dy;
        distortion(c, mx_d, my_d, &dx, &dy);
        mx_u = mx_d - dx; my_u = my_d - dy;
        for (int i = 1; i < n; ++i) {
            distortion(c, mx_u, my_u, &dx, &dy);
            mx_u = mx_d - dx; my_u = my_d - dy;
        }
    }
    out[0] = (float)(mx_u / 1.0); out[1] = (float)(my_u / 1.0);
}

/* cvRound of a float32, half to even; outside int's range it does not exist */
static int round_coord(float f, int *out) {
    if (!(f >= -2147483648.0f && f < 2147483648.0f)) return 0;
    *out = (int)lrintf(f);
    return 1;
}

/* G4: the float32 encodings in their total order */
static uint32_t order_key(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

static int check_item(const isv_det_config_t *c, const uint8_t *img, int W, int H, int stride, const isv_det_item_t *it, const int32_t *kept_index,
                      const float *new_pts, const float *new_un_pts) {
    if (!img || W < 1 || H < 1 || stride < W || it->n_points < 0 || it->max_new < 0) return ISV_DET_INPUT;
    if (it->n_points > 0 && (!it->cur_pts || !it->track_cnt || !kept_index)) return ISV_DET_INPUT;
    if (it->max_new > 0 && (!new_pts || !new_un_pts)) return ISV_DET_INPUT;
    if (it->n_points > c->max_points || it->max_new > c->max_corners) return ISV_DET_CAPACITY;
    for (int p = 0; p < it->n_points; p++) {
        const float x = it->cur_pts[2 * p], y = it->cur_pts[2 * p + 1];
        int rx, ry;
        if (!isfinite(x) || !isfinite(y) || !round_coord(x, &rx) || !round_coord(y, &ry) || rx < 0 || rx >= W || ry < 0 || ry >= H) return ISV_DET_INPUT;
    }
    return ISV_DET_OK;
}

/* setMask: returns the number of kept points */
static int det_set_mask(const isv_det_item_t *it, int r, uint8_t *mask, int W, int H, int32_t *kept_index, int64_t *cnt) {
    const int n = it->n_points;
    int32_t *order = malloc((size_t)(n > 0 ? n : 1) * sizeof(int32_t));
    /* G1: descending track_cnt, the input order among equals (an insertion sort is stable) */
    for (int i = 0; i < n; i++) {
        int j = i;
        while (j > 0 && it->track_cnt[order[j - 1]] < it->track_cnt[i]) { order[j] = order[j - 1]; j--; }
        order[j] = i;
    }
    int kept = 0;
    for (int s = 0; s < n; s++) {
        const int i = order[s];
        int x = 0, y = 0;             /* check_item has seen that both exist */
        round_coord(it->cur_pts[2 * i], &x); round_coord(it->cur_pts[2 * i + 1], &y);
        if (mask[(size_t)y * W + x] == 255) {
            kept_index[kept++] = i;
            cnt[C_CLIPPED] += isvo_det_disc(mask, W, H, x, y, r);
        } else cnt[C_DROPPED]++;
    }
    free(order);
    return kept;
}

typedef struct { float v; int32_t idx; } cand_t;

/* descending v; G2: among equals the higher raster index first */
static int cand_cmp(const void *pa, const void *pb) {
    const cand_t *a = pa, *b = pb;
    if (a->v > b->v) return -1;
    if (a->v < b->v) return 1;
    return a->idx > b->idx ? -1 : (a->idx < b->idx ? 1 : 0);
}

/* One item on one image ([H][stride], 8-bit).  cam supplies the camera (its other fields are not read).  eig_out: NULL or [H][W],
 * written when max_new > 0; mask_out: NULL or [H][W]; counters: NULL or [8] (the C_* above).  The other arrays as in
 * isv_det_detect_batch; a refused item leaves them untouched. */
void isvo_det_detect(const isv_det_config_t *c, const isv_trk_config_t *cam, const uint8_t *img, int W, int H, int stride, const isv_det_item_t *it,
                     isv_det_result_t *r, int32_t *kept_index, float *new_pts, float *new_un_pts, float *eig_out, uint8_t *mask_out, int64_t *counters) {
    int64_t cnt[C_COUNT];
    memset(cnt, 0, sizeof(cnt));
    r->status = check_item(c, img, W, H, stride, it, kept_index, new_pts, new_un_pts);
    r->n_points = it->n_points; r->n_kept = 0; r->n_new = 0; r->n_candidates = 0; r->max_val = 0.f;
    if (counters) memcpy(counters, cnt, sizeof(cnt));
    if (r->status != ISV_DET_OK) return;
    const size_t n = (size_t)W * H;
    uint8_t *mask = malloc(n);
    memset(mask, 255, n);
    r->n_kept = det_set_mask(it, c->min_dist, mask, W, H, kept_index, cnt);
    for (size_t p = 0; p < n; p++) cnt[C_MASKED] += mask[p] == 0;
    if (mask_out) memcpy(mask_out, mask, n);
    if (it->max_new > 0) {
        float *eig = malloc(n * sizeof(float)), *v = malloc(n * sizeof(float));
        isvo_det_response(img, W, H, stride, eig);
        if (eig_out) memcpy(eig_out, eig, n * sizeof(float));
        /* minMaxLoc under the mask */
        float maxVal = 0.f;
        int any = 0;
        for (size_t p = 0; p < n; p++)
            if (mask[p] && (!any || order_key(eig[p]) > order_key(maxVal))) { maxVal = eig[p]; any = 1; }
        r->max_val = maxVal;
        const float t = (float)((double)maxVal * c->quality_level);
        for (size_t p = 0; p < n; p++) v[p] = eig[p] > t ? eig[p] : 0.f;        /* THRESH_TOZERO */
        cand_t *cand = malloc((n > 0 ? n : 1) * sizeof(cand_t));
        size_t nc = 0;
        for (int y = 1; y < H - 1; y++)
            for (int x = 1; x < W - 1; x++) {
                const size_t p = (size_t)y * W + x;
                float dil = v[p];                  /* dilate: the 3 x 3 maximum */
                int equal = 0;
                for (int j = -1; j <= 1; j++)
                    for (int i = -1; i <= 1; i++) {
                        const float q = v[(size_t)(y + j) * W + (x + i)];
                        if (q > dil) dil = q;
                        if ((i || j) && q == v[p]) equal = 1;
                    }
                if (v[p] != 0.f && v[p] == dil && mask[p]) {
                    cand[nc].v = v[p]; cand[nc].idx = (int32_t)p; nc++;
                    cnt[C_PLATEAU] += equal;
                }
            }
        r->n_candidates = (int32_t)nc;
        cnt[C_CANDIDATES] = (int64_t)nc;
        qsort(cand, nc, sizeof(cand_t), cand_cmp);
        for (size_t k = 1; k < nc; k++) cnt[C_TIE_PAIRS] += cand[k].v == cand[k - 1].v;
        const int md2 = c->min_dist * c->min_dist;
        int nn = 0;
        for (size_t k = 0; k < nc && nn < it->max_new; k++) {
            const int x = cand[k].idx % W, y = cand[k].idx / W;
            int good = 1;
            for (int a = 0; a < nn && good; a++) {
                const int dx = x - (int)new_pts[2 * a], dy = y - (int)new_pts[2 * a + 1];
                if (dx * dx + dy * dy < md2) good = 0;
            }
            if (!good) { cnt[C_REJECTED]++; continue; }
            new_pts[2 * nn] = (float)x; new_pts[2 * nn + 1] = (float)y;
            isvo_det_lift(cam, (float)x, (float)y, new_un_pts + 2 * (size_t)nn);
            nn++;
        }
        r->n_new = nn;
        cnt[C_CAP_REACHED] = nn == it->max_new;
        free(cand); free(eig); free(v);
    }
    free(mask);
    if (counters) memcpy(counters, cnt, sizeof(cnt));
}
