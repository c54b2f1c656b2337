// lh_gftt.h — Shi-Tomasi corner detection (Frontend::DetectFeatures, src/frontend_lego.cpp:292-310, i.e.
// cv::GFTTDetector with blockSize 3, ksize 3, no Harris): the kernels' arguments, shared with the host side,
// and the per-pixel arithmetic.
//
// The arithmetic is exact: integer Sobel gradients, integer 3x3 sums of their products, D = (A-C)^2 + 4 B^2
// in int64, and lambda = (double)(A+C) - sqrt((double)D) with one correctly rounded fp64 square root and one
// subtraction.  It is plain C++ on one pixel's own data, written once for the kernels
// (lh_gftt.hip) and for any host compiler (a CPU probe runs the very same operations).
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define LH_GFTT_FN __host__ __device__ inline
#else
#define LH_GFTT_FN inline
#endif

// lh_gftt_args.state: one byte per pixel
#define LH_GFTT_S_NONE 0       // not a candidate
#define LH_GFTT_S_OPEN 1       // a candidate, undecided
#define LH_GFTT_S_TAKEN 2      // accepted
#define LH_GFTT_S_DROPPED 3    // rejected: a stronger accepted candidate lies within min_distance

struct lh_gftt_ctl {
    unsigned long long max_key;   // lh_gftt_key of the largest lambda over allowed pixels; 0: no allowed pixel
    uint32_t n_cand, n_acc;
    uint32_t open[3];             // nonzero: some candidate is still undecided after selection round j, in slot j % 3
    uint32_t pad;
};

struct lh_gftt_args {
    int32_t cols, rows;
    const uint8_t* img;           // [rows][cols]
    uint8_t* allow;               // [rows][cols] nonzero: allowed (the caller's mask, minus the exclusion boxes)
    int32_t n_exclude;
    const float* exclude_pt;      // [n_exclude][2]
    float exclude_half;
    double quality, min_dist2;    // quality_level; min_distance^2 (fp64 product)
    int32_t reach;                // ceil(min_distance) - 1: the largest |dx| at a distance < min_distance; < 0: no suppression
    int32_t limit;                // corners written at most
    double* eig;                  // [rows][cols] lambda
    uint8_t* state;               // [rows][cols] LH_GFTT_S_*
    uint32_t* cand;               // [n_cand] raster indices, in no particular order
    uint32_t* acc_idx;            // [n_acc] the accepted candidates, in no particular order
    double* acc_lam;
    float* kp;                    // [limit][2] accepted corners in descending (lambda, index)
    double* response;             // [limit]
    lh_gftt_ctl* ctl;
};

// BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba) of p in [-(n-1), 2(n-1)], n >= 2; anything further out is
// clamped into the image (no caller's result depends on such a tap).
LH_GFTT_FN int lh_gftt_reflect(int p, int n) {
    if (p < 0) p = -p;
    if (p > n - 1) p = 2 * (n - 1) - p;
    return p < 0 ? 0 : (p > n - 1 ? n - 1 : p);
}

// Sobel 3x3 of the taps t[3][3] (t[dy+1][dx+1]): x kernel [-1 0 1; -2 0 2; -1 0 1], y kernel its transpose.
LH_GFTT_FN void lh_gftt_sobel(const int (&t)[3][3], int* gx, int* gy) {
    *gx = (t[0][2] - t[0][0]) + 2 * (t[1][2] - t[1][0]) + (t[2][2] - t[2][0]);
    *gy = (t[2][0] - t[0][0]) + 2 * (t[2][1] - t[0][1]) + (t[2][2] - t[0][2]);
}

// lambda of the 2x2 structure matrix [A B; B C] of integer block sums: 2 * 3060^2 times cv::cornerMinEigenVal's.
LH_GFTT_FN double lh_gftt_lambda(int32_t A, int32_t B, int32_t C) {
    const int64_t d = (int64_t)A - C, b = B;
    const int64_t D = d * d + 4 * b * b;   // <= 4.4e14: exact, and exactly a double
    return (double)(A + C) - sqrt((double)D);
}

// The Sobel gradients at image position (x, y) inside the image, its taps extended by REFLECT_101.
LH_GFTT_FN void lh_gftt_gradient_at(const uint8_t* img, int cols, int rows, int64_t step, int x, int y, int* gx, int* gy) {
    int t[3][3];
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx)
            t[dy + 1][dx + 1] = img[(int64_t)lh_gftt_reflect(y + dy, rows) * step + lh_gftt_reflect(x + dx, cols)];
    lh_gftt_sobel(t, gx, gy);
}

// lambda at pixel (x, y) straight from the definition: the gradient products summed over the 3x3 block, the
// product images extended by REFLECT_101 (boxFilter, normalize = false).  The tiled kernel computes the same
// integers from LDS.
LH_GFTT_FN double lh_gftt_lambda_at(const uint8_t* img, int cols, int rows, int64_t step, int x, int y) {
    int32_t A = 0, B = 0, C = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            int gx, gy;
            lh_gftt_gradient_at(img, cols, rows, step, lh_gftt_reflect(x + dx, cols), lh_gftt_reflect(y + dy, rows), &gx, &gy);
            A += gx * gx;
            B += gx * gy;
            C += gy * gy;
        }
    return lh_gftt_lambda(A, B, C);
}

// One axis of an exclusion box: [rint(p - w), rint(p + w)] (float32 arithmetic, round half to even, as
// cv::Point2f -> cv::Point), both ends inclusive, clipped to [0, n - 1].  Empty (*lo > *hi) when it misses
// the image or p is not a number.
LH_GFTT_FN void lh_gftt_box_axis(float p, float w, int n, int* lo, int* hi) {
    const float a = p - w, b = p + w;
    const float fa = rintf(a), fb = rintf(b);
    if (!(fb >= 0.0f) || !(fa <= (float)(n - 1)) || !(fa <= fb)) {
        *lo = 0;
        *hi = -1;
        return;
    }
    *lo = fa > 0.0f ? (int)fa : 0;
    *hi = fb < (float)(n - 1) ? (int)fb : n - 1;
}

// An order-preserving map of a double (not a NaN) onto unsigned integers above 0: the masked maximum is
// folded with integer atomics, and 0 stands for "no allowed pixel".
LH_GFTT_FN unsigned long long lh_gftt_key(double v) {
    unsigned long long u;
    __builtin_memcpy(&u, &v, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
LH_GFTT_FN double lh_gftt_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    __builtin_memcpy(&v, &u, 8);
    return v;
}

// (lambda, raster index) descending: the order cv::goodFeaturesToTrack walks its candidates in (OpenCV 4's
// greaterThanPtr: equal values go to the larger address first).
LH_GFTT_FN bool lh_gftt_stronger(double la, uint32_t ia, double lb, uint32_t ib) {
    return la > lb || (la == lb && ia > ib);
}
