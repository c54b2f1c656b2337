// lh_klt.h — pyramidal KLT tracking (lh_klt_track, include/lego_ba.h): the kernels' arguments,
// shared with the host side, and the per-point arithmetic of cv::calcOpticalFlowPyrLK's scalar path with an
// 11 x 11 window on 8-bit images.
//
// The arithmetic is plain C++ on one point's own data, written once for the kernels (lh_klt.hip) and for any host
// compiler (tests/klt_probe.cpp runs the very same operations).  The pyramid, the derivatives and the window sums are
// exact integers; every float step is one correctly rounded IEEE binary32 operation.  Contraction is off in this
// file, and the two operations a device may not round correctly in binary32 (division, square root) go through
// binary64, whose result rounded to binary32 is the correctly rounded one (53 >= 2 * 24 + 2).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define LH_KLT_FN __host__ __device__ inline
#else
#define LH_KLT_FN inline
#endif

#define LH_KLT_MAX_LEVELS 4    // max_level <= 3
#define LH_KLT_WIN 11          // the window; a point's window reaches 11 pixels past an edge
#define LH_KLT_HALF 5
#define LH_KLT_MIN_SIZE 12     // cols, rows of every level: one REFLECT_101 fold covers every read

struct lh_klt_levels {
    const uint8_t* data[LH_KLT_MAX_LEVELS];
    int32_t cols[LH_KLT_MAX_LEVELS], rows[LH_KLT_MAX_LEVELS];
    int64_t step[LH_KLT_MAX_LEVELS];
};

struct lh_klt_args {
    lh_klt_levels I, J;        // the two pyramids (one shape)
    int32_t n_levels;          // L + 1
    int32_t n_points;
    const float* kp1;          // [n_points][2]
    float* kp2;                // [n_points][2] in: the guess (has_initial); out: the tracked points
    uint8_t* success;          // [n_points]
    int32_t has_initial, max_iters;
    double eps2;               // epsilon * epsilon
    double min_eig;
};

// The level sizes of a cols x rows image: level l + 1 is ((cols + 1) / 2, (rows + 1) / 2), built while l < max_level
// and both its sizes are > 11 (buildOpticalFlowPyramid).  Returns the number of levels, L + 1.
LH_KLT_FN int lh_klt_level_sizes(int cols, int rows, int max_level, int32_t* lc, int32_t* lr) {
    int n = 1;
    lc[0] = cols; lr[0] = rows;
    while (n - 1 < max_level && n < LH_KLT_MAX_LEVELS) {
        const int c = (lc[n - 1] + 1) / 2, r = (lr[n - 1] + 1) / 2;
        if (c <= LH_KLT_WIN || r <= LH_KLT_WIN) break;
        lc[n] = c; lr[n] = r;
        ++n;
    }
    return n;
}

#ifdef LH_KLT_IMPL   // the arithmetic: lh_klt.hip and the CPU probe define it; the host side needs the structs alone
#pragma clang fp contract(off)

// BORDER_REFLECT_101 with one fold, which covers every index the definition reads (|offset past an edge| <= 11 < n).
// An index further out (a staged tile's corner that no tap reads) is clamped, so the read stays inside the image.
LH_KLT_FN int lh_klt_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// ---- pyrDown: dst(x, y) = (sum_ij w_i w_j src(r(2x + i), r(2y + j)) + 128) >> 8, w = (1, 4, 6, 4, 1) ----
LH_KLT_FN int lh_klt_pyr_row(const uint8_t* row, int cols, int x) {   // the horizontal pass of output column x
    return row[lh_klt_reflect(2 * x - 2, cols)] + 4 * row[lh_klt_reflect(2 * x - 1, cols)] + 6 * row[lh_klt_reflect(2 * x, cols)] +
           4 * row[lh_klt_reflect(2 * x + 1, cols)] + row[lh_klt_reflect(2 * x + 2, cols)];
}
LH_KLT_FN uint8_t lh_klt_pyr_col(int h0, int h1, int h2, int h3, int h4) {   // the vertical pass and the rounding
    return (uint8_t)((h0 + 4 * h1 + 6 * h2 + 4 * h3 + h4 + 128) >> 8);
}
LH_KLT_FN uint8_t lh_klt_pyr_pixel(const uint8_t* src, int cols, int rows, int64_t step, int x, int y) {
    int h[5];
    for (int j = 0; j < 5; ++j) h[j] = lh_klt_pyr_row(src + (int64_t)lh_klt_reflect(2 * y - 2 + j, rows) * step, cols, x);
    return lh_klt_pyr_col(h[0], h[1], h[2], h[3], h[4]);
}

// ---- Scharr derivatives of one pixel from its 3 x 3 neighbourhood nb[dy][dx] (REFLECT_101 bytes at the edge) ----
//   t0(x, y) = 3 (I(x, y-1) + I(x, y+1)) + 10 I(x, y)    Ix(x, y) = t0(x+1, y) - t0(x-1, y)
//   t1(x, y) = I(x, y+1) - I(x, y-1)                     Iy(x, y) = 3 (t1(x-1, y) + t1(x+1, y)) + 10 t1(x, y)
LH_KLT_FN void lh_klt_scharr(const int nb[3][3], int* ix, int* iy) {
    const int t0l = 3 * (nb[0][0] + nb[2][0]) + 10 * nb[1][0], t0r = 3 * (nb[0][2] + nb[2][2]) + 10 * nb[1][2];
    const int t1l = nb[2][0] - nb[0][0], t1c = nb[2][1] - nb[0][1], t1r = nb[2][2] - nb[0][2];
    *ix = t0r - t0l;
    *iy = 3 * (t1l + t1r) + 10 * t1c;
}

// ---- steps 1 and 5.1: the range test on a floored position, in float (NaN and huge values fail) ----
LH_KLT_FN bool lh_klt_in_range(float ix, float iy, int cols, int rows) {
    return ix >= -(float)LH_KLT_WIN && ix < (float)cols && iy >= -(float)LH_KLT_WIN && iy < (float)rows;
}

// ---- step 2: the four fixed-point weights of a position p with floor ip ----
LH_KLT_FN void lh_klt_weights(float px, float ipx, float py, float ipy, int w[4]) {
    const float a = px - ipx, b = py - ipy;
    w[0] = (int)rintf(((1.f - a) * (1.f - b)) * 16384.f);
    w[1] = (int)rintf((a * (1.f - b)) * 16384.f);
    w[2] = (int)rintf(((1.f - a) * b) * 16384.f);
    w[3] = 16384 - w[0] - w[1] - w[2];
}

// ---- step 3: the bilinear sum of four taps and its descales (arithmetic shifts) ----
LH_KLT_FN int lh_klt_bil(int f00, int f01, int f10, int f11, const int w[4]) {
    return f00 * w[0] + f01 * w[1] + f10 * w[2] + f11 * w[3];
}
LH_KLT_FN int lh_klt_descale_img(int bil) { return (bil + 256) >> 9; }       // Iw, Jw: 32 x the grey value
LH_KLT_FN int lh_klt_descale_der(int bil) { return (bil + 8192) >> 14; }     // ix, iy

// (float)(double)S * 2^-20
LH_KLT_FN float lh_klt_sum_to_float(int64_t s) { return (float)(double)s * 9.5367431640625e-07f; }

LH_KLT_FN float lh_klt_div(float a, float b) { return (float)((double)a / (double)b); }
LH_KLT_FN float lh_klt_sqrt(float a) { return (float)sqrt((double)a); }

// ---- step 4: the structure tensor of the window; false: the level fails ----
struct lh_klt_tensor { float A11, A12, A22, D; };
LH_KLT_FN bool lh_klt_make_tensor(const int64_t S[3], double min_eig_threshold, lh_klt_tensor* t) {
    const float A11 = lh_klt_sum_to_float(S[0]), A12 = lh_klt_sum_to_float(S[1]), A22 = lh_klt_sum_to_float(S[2]);
    const float D = A11 * A22 - A12 * A12;
    const float d = A11 - A22;
    const float min_eig = lh_klt_div((A22 + A11) - lh_klt_sqrt(d * d + (4.f * A12) * A12), 242.f);
    t->A11 = A11; t->A12 = A12; t->A22 = A22;
    if ((double)min_eig < min_eig_threshold || D < FLT_EPSILON) return false;
    t->D = lh_klt_div(1.f, D);
    return true;
}

// ---- step 5.4: the update of one iteration from the mismatch sums ----
LH_KLT_FN void lh_klt_delta(const lh_klt_tensor& t, const int64_t B[2], float* dx, float* dy) {
    const float b1 = lh_klt_sum_to_float(B[0]), b2 = lh_klt_sum_to_float(B[1]);
    *dx = (t.A12 * b2 - t.A22 * b1) * t.D;
    *dy = (t.A12 * b1 - t.A11 * b2) * t.D;
}

// ---- steps 5.5 - 5.8: apply the update; true: the loop ends (by epsilon, or by oscillation) ----
LH_KLT_FN bool lh_klt_advance(int j, float dx, float dy, double eps2, float* qx, float* qy, float* k2x, float* k2y,
                             float* prev_x, float* prev_y) {
    *qx += dx;
    *qy += dy;
    *k2x = *qx + (float)LH_KLT_HALF;
    *k2y = *qy + (float)LH_KLT_HALF;
    if ((double)dx * (double)dx + (double)dy * (double)dy <= eps2) return true;
    if (j > 0 && fabs((double)(dx + *prev_x)) < 0.01 && fabs((double)(dy + *prev_y)) < 0.01) {
        *k2x -= 0.5f * dx;
        *k2y -= 0.5f * dy;
        return true;
    }
    *prev_x = dx;
    *prev_y = dy;
    return false;
}

// One point through every level, coarse to fine.  Every decision is taken here, on exact window sums that `sums`
// supplies: a serial loop on the host, one wave's lanes on the device (where all lanes run this code on the same
// values, so control flow is wave-uniform).
//   void sums.window(level, ipx, ipy, w, S)    steps 3 and the sums of 4: keeps Iw, ix, iy of the level; S = S11, S12, S22
//   void sums.mismatch(level, iqx, iqy, w, B)  steps 5.2 and 5.3: B = B1, B2
// (gx, gy): the guess, kp2 with has_initial and kp1 without.
template <class Sums>
LH_KLT_FN void lh_klt_track_point(Sums& sums, int n_levels, const int32_t* cols, const int32_t* rows, float k1x, float k1y,
                                  float gx, float gy, int max_iters, double eps2, double min_eig_threshold, float* out_x,
                                  float* out_y, int* status) {
    float k2x = gx, k2y = gy;
    int ok = 1;
    for (int l = n_levels - 1; l >= 0; --l) {
        const float sc = l == 0 ? 1.f : l == 1 ? 0.5f : l == 2 ? 0.25f : 0.125f;   // (float)(1 / 2^l)
        float px = k1x * sc, py = k1y * sc;
        float qx = l == n_levels - 1 ? k2x * sc : 2.f * k2x, qy = l == n_levels - 1 ? k2y * sc : 2.f * k2y;
        k2x = qx;
        k2y = qy;
        int w[4];
        px -= (float)LH_KLT_HALF;
        py -= (float)LH_KLT_HALF;
        const float ipx = floorf(px), ipy = floorf(py);
        if (!lh_klt_in_range(ipx, ipy, cols[l], rows[l])) {
            if (l == 0) ok = 0;
            continue;
        }
        lh_klt_weights(px, ipx, py, ipy, w);
        int64_t S[3];
        sums.window(l, (int)ipx, (int)ipy, w, S);
        lh_klt_tensor t;
        if (!lh_klt_make_tensor(S, min_eig_threshold, &t)) {
            if (l == 0) ok = 0;
            continue;
        }
        qx -= (float)LH_KLT_HALF;
        qy -= (float)LH_KLT_HALF;
        float prev_x = 0.f, prev_y = 0.f;
        for (int j = 0; j < max_iters; ++j) {
            const float iqx = floorf(qx), iqy = floorf(qy);
            if (!lh_klt_in_range(iqx, iqy, cols[l], rows[l])) {
                if (l == 0) ok = 0;
                break;
            }
            lh_klt_weights(qx, iqx, qy, iqy, w);
            int64_t B[2];
            sums.mismatch(l, (int)iqx, (int)iqy, w, B);
            float dx, dy;
            lh_klt_delta(t, B, &dx, &dy);
            if (lh_klt_advance(j, dx, dy, eps2, &qx, &qy, &k2x, &k2y, &prev_x, &prev_y)) break;
        }
    }
    *out_x = k2x;
    *out_y = k2y;
    *status = ok;
}

#endif  // LH_KLT_IMPL
