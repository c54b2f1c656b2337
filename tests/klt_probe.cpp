// klt_probe.cpp — lego-slam_amd/csrc/lh_klt.h compiled for the host (tests/test_klt_cpu.py builds it with
// -ffp-contract=off): the whole tracker on plain arrays, the kernels' arithmetic with serial loops where the device
// has lanes (scripts/klt_time.py times it on one thread beside the device).
#include <vector>

#define LH_KLT_IMPL
#include "lh_klt.h"

namespace {

struct Pyramid {
    std::vector<std::vector<uint8_t>> own;   // levels 1..
    lh_klt_levels lv{};
    int n = 0;
};

void pyr_down(const uint8_t* src, int cols, int rows, int64_t step, uint8_t* dst) {
    const int dc = (cols + 1) / 2, dr = (rows + 1) / 2;
    for (int y = 0; y < dr; ++y)
        for (int x = 0; x < dc; ++x) dst[(int64_t)y * dc + x] = lh_klt_pyr_pixel(src, cols, rows, step, x, y);
}

void build(Pyramid& p, const uint8_t* img, int cols, int rows, int64_t step, int max_level) {
    p.n = lh_klt_level_sizes(cols, rows, max_level, p.lv.cols, p.lv.rows);
    p.lv.data[0] = img;
    p.lv.step[0] = step;
    p.own.resize(p.n);
    for (int l = 1; l < p.n; ++l) {
        p.own[l].resize((size_t)p.lv.cols[l] * p.lv.rows[l]);
        pyr_down(p.lv.data[l - 1], p.lv.cols[l - 1], p.lv.rows[l - 1], p.lv.step[l - 1], p.own[l].data());
        p.lv.data[l] = p.own[l].data();
        p.lv.step[l] = p.lv.cols[l];
    }
}

// the window sums of one point, pixel by pixel
struct SerialSums {
    const lh_klt_levels &I, &J;
    int iw[LH_KLT_WIN * LH_KLT_WIN], dx[LH_KLT_WIN * LH_KLT_WIN], dy[LH_KLT_WIN * LH_KLT_WIN];

    static int byte_at(const lh_klt_levels& v, int l, int x, int y) {
        return v.data[l][(int64_t)lh_klt_reflect(y, v.rows[l]) * v.step[l] + lh_klt_reflect(x, v.cols[l])];
    }
    void deriv_at(int l, int x, int y, int* gx, int* gy) const {   // 0 outside the image
        *gx = *gy = 0;
        if (x < 0 || y < 0 || x >= I.cols[l] || y >= I.rows[l]) return;
        int nb[3][3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) nb[r][c] = byte_at(I, l, x + c - 1, y + r - 1);
        lh_klt_scharr(nb, gx, gy);
    }
    void window(int l, int ipx, int ipy, const int w[4], int64_t S[3]) {
        S[0] = S[1] = S[2] = 0;
        for (int y = 0; y < LH_KLT_WIN; ++y)
            for (int x = 0; x < LH_KLT_WIN; ++x) {
                const int k = y * LH_KLT_WIN + x, X = ipx + x, Y = ipy + y;
                iw[k] = lh_klt_descale_img(lh_klt_bil(byte_at(I, l, X, Y), byte_at(I, l, X + 1, Y), byte_at(I, l, X, Y + 1),
                                                      byte_at(I, l, X + 1, Y + 1), w));
                int gx[4], gy[4];
                deriv_at(l, X, Y, &gx[0], &gy[0]);
                deriv_at(l, X + 1, Y, &gx[1], &gy[1]);
                deriv_at(l, X, Y + 1, &gx[2], &gy[2]);
                deriv_at(l, X + 1, Y + 1, &gx[3], &gy[3]);
                dx[k] = lh_klt_descale_der(lh_klt_bil(gx[0], gx[1], gx[2], gx[3], w));
                dy[k] = lh_klt_descale_der(lh_klt_bil(gy[0], gy[1], gy[2], gy[3], w));
                S[0] += (int64_t)dx[k] * dx[k];
                S[1] += (int64_t)dx[k] * dy[k];
                S[2] += (int64_t)dy[k] * dy[k];
            }
    }
    void mismatch(int l, int iqx, int iqy, const int w[4], int64_t B[2]) {
        B[0] = B[1] = 0;
        for (int y = 0; y < LH_KLT_WIN; ++y)
            for (int x = 0; x < LH_KLT_WIN; ++x) {
                const int k = y * LH_KLT_WIN + x, X = iqx + x, Y = iqy + y;
                const int diff = lh_klt_descale_img(lh_klt_bil(byte_at(J, l, X, Y), byte_at(J, l, X + 1, Y), byte_at(J, l, X, Y + 1),
                                                               byte_at(J, l, X + 1, Y + 1), w)) - iw[k];
                B[0] += (int64_t)diff * dx[k];
                B[1] += (int64_t)diff * dy[k];
            }
    }
};

}  // namespace

extern "C" {

int klt_level_count(int cols, int rows, int max_level) {
    int32_t c[LH_KLT_MAX_LEVELS], r[LH_KLT_MAX_LEVELS];
    return lh_klt_level_sizes(cols, rows, max_level, c, r);
}

void klt_pyr_down(const uint8_t* src, int cols, int rows, int64_t step, uint8_t* dst) { pyr_down(src, cols, rows, step, dst); }

// kp2: the guess on entry with has_initial.  Returns 0, or 1 on a bad argument.
int klt_track(const uint8_t* img1, const uint8_t* img2, int cols, int rows, int64_t step, int n, const float* kp1, float* kp2,
              uint8_t* success, int has_initial, int max_level, int max_iters, double epsilon, double min_eig) {
    if (cols < LH_KLT_MIN_SIZE || rows < LH_KLT_MIN_SIZE || step < cols || max_level < 0 || max_level > 3 || max_iters < 1)
        return 1;
    Pyramid p1, p2;
    build(p1, img1, cols, rows, step, max_level);
    build(p2, img2, cols, rows, step, max_level);
    SerialSums sums{p1.lv, p2.lv, {}, {}, {}};
    for (int i = 0; i < n; ++i) {
        const float gx = has_initial ? kp2[2 * i] : kp1[2 * i], gy = has_initial ? kp2[2 * i + 1] : kp1[2 * i + 1];
        int ok;
        lh_klt_track_point(sums, p1.n, p1.lv.cols, p1.lv.rows, kp1[2 * i], kp1[2 * i + 1], gx, gy, max_iters, epsilon * epsilon,
                           min_eig, &kp2[2 * i], &kp2[2 * i + 1], &ok);
        success[i] = (uint8_t)ok;
    }
    return 0;
}

}  // extern "C"
