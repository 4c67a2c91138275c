/* isv_kf_oracle.c -- the serial restatement of include/isvins_keyframe.h in plain C: one item in, its arrays out.
 * The kernels of is-vins_amd/csrc/isv_keyframe.hip are pinned to it bit for bit; tests/test_kf_oracle.py pins it independently
 * (numpy statements of FAST, the blur, BRIEF and the lift written from their definitions, shift invariance, the quirks).
 * Built with gcc -O2 -ffp-contract=off by tests/kf_oracle.py.
 *
 * Restated (own text) from OpenCV 3.2.0 as published and from the reference:
 *   FAST_t<16> / makeOffsets     features2d/src/fast.cpp            fast_image: threshold table, the 25-entry wrapped circle, count > 8
 *   cornerScore<16>              features2d/src/fast_score.cpp      corner_score
 *   getGaussianKernel            imgproc/src/smooth.cpp             isvo_kf_kernel
 *   createSeparableLinearFilter  imgproc/src/filter.cpp             blur_image: 8-bit fixed point, both kernels * 256, (v + 32768) >> 16
 *   cv::borderInterpolate        core/src/copy.cpp                  reflect101
 *   BRIEF::compute               thirdparty/DVision/BRIEF.cpp:39-106                       brief_at
 *   liftProjective, distortion   PinholeCamera.cc:461-521, :657-673                        isvo_kf_lift
 *   KeyFrame::computeWindowBRIEFPoint / computeBRIEFPoint   src/pose_graph/keyframe.cpp:43-69   isvo_kf_extract
 *
 * isvo_kf_set_quirks_off(bits) switches kept reference quirks off one at a time, for the tests that show each one matters:
 *   1  K1  a test coordinate is rounded down (floor) instead of toward zero
 *   2  K2  a corner survives a neighbour of EQUAL score (>= instead of >)
 *   4  K4  BRIEF reads the raw image as FAST does
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "isvins_keyframe.h"

enum { QK1 = 1, QK2 = 2, QK4 = 4 };
static int g_quirks_off = 0;
void isvo_kf_set_quirks_off(int bits) { g_quirks_off = bits; }

int isvo_kf_sizeof(int i) {
    switch (i) {
    case 0: return (int)sizeof(isv_kf_config_t);
    case 1: return (int)sizeof(isv_kf_item_t);
    case 2: return (int)sizeof(isv_kf_result_t);
    }
    return -1;
}

/* getGaussianKernel(9, 2, CV_32F), then convertTo(CV_32S, 256): out[9].  Returns 1 iff they are the integers the header states. */
int isvo_kf_kernel(int32_t out[9]) {
    static const int32_t want[9] = {7, 17, 32, 46, 52, 46, 32, 17, 7};
    const int n = 9;
    const double sigmaX = 2.0, scale2X = -0.5 / (sigmaX * sigmaX);
    float cf[9];
    double sum = 0;
    for (int i = 0; i < n; i++) {
        const double x = i - (n - 1) * 0.5;
        const double t = exp(scale2X * x * x);
        cf[i] = (float)t;
        sum += cf[i];
    }
    sum = 1. / sum;
    int same = 1;
    for (int i = 0; i < n; i++) {
        cf[i] = (float)(cf[i] * sum);
        out[i] = (int32_t)lrint((double)cf[i] * 256.0);       /* cvRound: to nearest, ties to even */
        same &= out[i] == want[i];
    }
    return same;
}

static int reflect101(int p, int len) {
    if (len == 1) return 0;
    do {
        if (p < 0) p = -p - 1 + 1;
        else if (p >= len) p = len - 1 - (p - len) - 1;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

/* src [H][stride] -> dst [H][W] */
static void blur_image(const uint8_t *src, int W, int H, int stride, uint8_t *dst) {
    int32_t K[9];
    if (!isvo_kf_kernel(K)) abort();
    if (W <= 0 || H <= 0) return;
    int32_t *rows = malloc(sizeof(int32_t) * (size_t)W * H);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            int32_t s = 0;
            for (int k = 0; k < 9; k++) s += K[k] * src[(size_t)y * stride + reflect101(x + k - 4, W)];
            rows[(size_t)y * W + x] = s;
        }
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            int32_t s = 0;
            for (int k = 0; k < 9; k++) s += K[k] * rows[(size_t)reflect101(y + k - 4, H) * W + x];
            dst[(size_t)y * W + x] = (uint8_t)((s + 32768) >> 16);
        }
    free(rows);
}

/* K3: cornerScore<16> */
static int corner_score(const uint8_t *ptr, const int pixel[25], int threshold) {
    const int K = 8, N = K * 3 + 1;
    int k, v = ptr[0];
    short d[25];
    for (k = 0; k < N; k++) d[k] = (short)(v - ptr[pixel[k]]);
    int a0 = threshold;
    for (k = 0; k < 16; k += 2) {
        int a = d[k + 1] < d[k + 2] ? d[k + 1] : d[k + 2];
        a = a < d[k + 3] ? a : d[k + 3];
        if (a <= a0) continue;
        for (int j = 4; j <= 8; j++) a = a < d[k + j] ? a : d[k + j];
        int m = a < d[k] ? a : d[k];
        a0 = a0 > m ? a0 : m;
        m = a < d[k + 9] ? a : d[k + 9];
        a0 = a0 > m ? a0 : m;
    }
    int b0 = -a0;
    for (k = 0; k < 16; k += 2) {
        int b = d[k + 1] > d[k + 2] ? d[k + 1] : d[k + 2];
        b = b > d[k + 3] ? b : d[k + 3];
        for (int j = 4; j <= 5; j++) b = b > d[k + j] ? b : d[k + j];
        if (b >= b0) continue;
        for (int j = 6; j <= 8; j++) b = b > d[k + j] ? b : d[k + j];
        int m = b > d[k] ? b : d[k];
        b0 = b0 < m ? b0 : m;
        m = b > d[k + 9] ? b : d[k + 9];
        b0 = b0 < m ? b0 : m;
    }
    return -b0 - 1;
}

/* FAST_t<16> before the suppression: smap [H][W], the score where (x, y) is a corner, else 0.  K4: img is the raw image. */
static void fast_image(const uint8_t *img, int W, int H, int stride, int threshold, uint8_t *smap) {
    static const int offsets16[16][2] = {{0, 3}, {1, 3}, {2, 2}, {3, 1}, {3, 0}, {3, -1}, {2, -2}, {1, -3},
                                         {0, -3}, {-1, -3}, {-2, -2}, {-3, -1}, {-3, 0}, {-3, 1}, {-2, 2}, {-1, 3}};
    const int K = 8, N = 25;
    int pixel[25];
    uint8_t threshold_tab[512];
    if (W > 0 && H > 0) memset(smap, 0, (size_t)W * H);
    for (int k = 0; k < 16; k++) pixel[k] = offsets16[k][0] + offsets16[k][1] * stride;
    for (int k = 16; k < N; k++) pixel[k] = pixel[k - 16];
    for (int i = -255; i <= 255; i++) threshold_tab[i + 255] = (uint8_t)(i < -threshold ? 1 : i > threshold ? 2 : 0);
    for (int i = 3; i < H - 3; i++) {
        const uint8_t *ptr = img + (size_t)i * stride + 3;
        for (int j = 3; j < W - 3; j++, ptr++) {
            const int v = ptr[0];
            const uint8_t *tab = &threshold_tab[0] - v + 255;
            int d = tab[ptr[pixel[0]]] | tab[ptr[pixel[8]]];
            if (d == 0) continue;
            d &= tab[ptr[pixel[2]]] | tab[ptr[pixel[10]]];
            d &= tab[ptr[pixel[4]]] | tab[ptr[pixel[12]]];
            d &= tab[ptr[pixel[6]]] | tab[ptr[pixel[14]]];
            if (d == 0) continue;
            d &= tab[ptr[pixel[1]]] | tab[ptr[pixel[9]]];
            d &= tab[ptr[pixel[3]]] | tab[ptr[pixel[11]]];
            d &= tab[ptr[pixel[5]]] | tab[ptr[pixel[13]]];
            d &= tab[ptr[pixel[7]]] | tab[ptr[pixel[15]]];
            int corner = 0;
            if (d & 1) {
                const int vt = v - threshold;
                int count = 0;
                for (int k = 0; k < N; k++) {
                    const int x = ptr[pixel[k]];
                    if (x < vt) { if (++count > K) { corner = 1; break; } }
                    else count = 0;
                }
            }
            if (!corner && (d & 2)) {
                const int vt = v + threshold;
                int count = 0;
                for (int k = 0; k < N; k++) {
                    const int x = ptr[pixel[k]];
                    if (x > vt) { if (++count > K) { corner = 1; break; } }
                    else count = 0;
                }
            }
            if (corner) smap[(size_t)i * W + j] = (uint8_t)corner_score(ptr, pixel, threshold);
        }
    }
}

/* the suppression of FAST_t<16>: a score against its row and the rows above and below (all zero outside the candidate area) */
static int survives(const uint8_t *smap, int W, int x, int y) {
    const uint8_t *prev = smap + (size_t)y * W, *pprev = prev - W, *curr = prev + W;
    const int score = prev[x];
    if (!score) return 0;
    if (g_quirks_off & QK2)
        return score >= prev[x + 1] && score >= prev[x - 1] && score >= pprev[x - 1] && score >= pprev[x] && score >= pprev[x + 1] &&
               score >= curr[x - 1] && score >= curr[x] && score >= curr[x + 1];
    return score > prev[x + 1] && score > prev[x - 1] && score > pprev[x - 1] && score > pprev[x] && score > pprev[x + 1] &&   /* K2 */
           score > curr[x - 1] && score > curr[x] && score > curr[x + 1];
}

/* (int) of a float32; outside int's range (undefined in C): outside every image */
static int trunc_coord(float f) {
    if (!(f > -2147483648.0f && f < 2147483648.0f)) return -1;
    if (g_quirks_off & QK1) return (int)floorf(f);
    return (int)f;                                /* K1 */
}

/* BRIEF::compute's inner loop on the image im [H][W] */
static void brief_at(const isv_kf_config_t *c, const uint8_t *im, int W, int H, float px, float py, uint64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    for (int i = 0; i < ISV_KF_PATTERN_BITS; i++) {
        const int x1 = trunc_coord(px + (float)c->x1[i]), y1 = trunc_coord(py + (float)c->y1[i]);
        const int x2 = trunc_coord(px + (float)c->x2[i]), y2 = trunc_coord(py + (float)c->y2[i]);
        if (x1 >= 0 && x1 < W && y1 >= 0 && y1 < H && x2 >= 0 && x2 < W && y2 >= 0 && y2 < H)    /* K5 */
            if (im[(size_t)y1 * W + x1] < im[(size_t)y2 * W + x2]) out[i >> 6] |= 1ull << (i & 63);
    }
}

static void distortion(const isv_kf_config_t *c, double x, double y, double *dx, double *dy) {
    const double k1 = c->k1, k2 = c->k2, p1 = c->p1, p2 = c->p2;
    const double mx2_u = x * x, my2_u = y * y, mxy_u = x * y, rho2_u = mx2_u + my2_u;
    const double rad_dist_u = k1 * rho2_u + k2 * rho2_u * rho2_u;
    *dx = x * rad_dist_u + 2.0 * p1 * mxy_u + p2 * (rho2_u + 2.0 * mx2_u);
    *dy = y * rad_dist_u + 2.0 * p2 * mxy_u + p1 * (rho2_u + 2.0 * my2_u);
}

/* liftProjective of (u, v) and keyframe.cpp:66: out = (float)(x / z), (float)(y / z) with z = 1.0 */
void isvo_kf_lift(const isv_kf_config_t *c, float u, float v, float out[2]) {
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

static int check_item(const isv_kf_config_t *c, const isv_kf_item_t *it) {
    if (it->width < 0 || it->height < 0 || it->n_points < 0 || it->stride < it->width) return ISV_KF_INPUT;
    if (it->width > 0 && it->height > 0 && !it->image) return ISV_KF_INPUT;
    if (it->n_points > 0 && !it->point_2d_uv) return ISV_KF_INPUT;
    if (it->width > c->max_width || it->height > c->max_height || it->n_points > c->max_points) return ISV_KF_CAPACITY;
    for (size_t k = 0; k < 2 * (size_t)it->n_points; k++)
        if (!isfinite(it->point_2d_uv[k])) return ISV_KF_INPUT;
    return ISV_KF_OK;
}

/* One item.  blurred / score_map: NULL or [height][width], written whenever the item passes the input checks.  The other arrays
 * as in isv_kf_extract_batch; a refused item leaves them untouched. */
void isvo_kf_extract(const isv_kf_config_t *c, const isv_kf_item_t *it, isv_kf_result_t *r, uint64_t *brief, float *keypoints_uv,
                     float *keypoints_norm, uint8_t *score, uint64_t *window_brief, uint8_t *blurred, uint8_t *score_map) {
    r->status = check_item(c, it); r->n_keypoints = 0; r->n_points = it->n_points; r->_pad = 0;
    if (r->status != ISV_KF_OK) return;
    const int W = it->width, H = it->height;
    const size_t px = (size_t)W * H;
    uint8_t *blur = malloc(px + 1), *smap = malloc(px + 1), *raw = malloc(px + 1);
    if (W > 0) for (int y = 0; y < H; y++) memcpy(raw + (size_t)y * W, it->image + (size_t)y * it->stride, W);
    blur_image(it->image, W, H, it->stride, blur);                    /* K6: once */
    fast_image(it->image, W, H, it->stride, c->fast_threshold, smap);
    if (blurred && px) memcpy(blurred, blur, px);
    if (score_map && px) memcpy(score_map, smap, px);
    int count = 0;
    for (int y = 3; y < H - 3; y++)
        for (int x = 3; x < W - 3; x++) count += survives(smap, W, x, y);
    r->n_keypoints = count;
    if (count > c->max_keypoints) r->status = ISV_KF_CAPACITY;
    else {
        const uint8_t *im = (g_quirks_off & QK4) ? raw : blur;        /* K4 */
        int k = 0;
        for (int y = 3; y < H - 3; y++)
            for (int x = 3; x < W - 3; x++) {
                if (!survives(smap, W, x, y)) continue;
                keypoints_uv[2 * k] = (float)x; keypoints_uv[2 * k + 1] = (float)y;
                score[k] = smap[(size_t)y * W + x];
                brief_at(c, im, W, H, (float)x, (float)y, brief + 4 * (size_t)k);
                isvo_kf_lift(c, (float)x, (float)y, keypoints_norm + 2 * (size_t)k);
                k++;
            }
        for (int i = 0; i < it->n_points; i++)
            brief_at(c, im, W, H, it->point_2d_uv[2 * i], it->point_2d_uv[2 * i + 1], window_brief + 4 * (size_t)i);
    }
    free(blur); free(smap); free(raw);
}
