// lh_klt.hip — CDNA4 (gfx950) kernels of the pyramidal KLT tracker (lh_klt_track, include/lego_ba.h),
// cv::calcOpticalFlowPyrLK's scalar path with an 11 x 11 window as lh_klt.h defines it:
//   k_klt_pyr    one level of the 5 x 5 pyrDown of one image, bytes in and bytes out: a workgroup makes a 16 x 16 tile
//                of the level, the horizontal pass into an LDS tile of 35 x 16 sums, the vertical pass out of it;
//   k_klt_track  one wave per keypoint runs lh_klt_track_point, every level coarse to fine.  The 121 window pixels go
//                over the 64 lanes (a lane owns pixels `lane` and `lane + 64`) and keep Iw, ix, iy of the level in
//                registers.  I comes from a 14 x 14-byte LDS tile around ip (REFLECT_101 on the bytes), its Scharr
//                derivatives are taken on the fly into a 12 x 12 LDS tile (zero at a position outside the image); J
//                comes from a 32 x 24-byte LDS window staged around the level's first q, or, once q has left it,
//                from global memory with the same REFLECT_101 indexing.  The five window sums are integer wave
//                reductions (a lane's partial of two pixels fits int32, the totals need int64): exact, so their order
//                is free and every lane holds the same totals.  Every float step and every decision is lh_klt.h's, run
//                by all lanes on those totals: control flow is wave-uniform and the result is bitwise the host
//                build's by construction.  No floating-point atomic, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LH_KLT_IMPL
#include "lh_launch.h"

#pragma clang fp contract(off)

// ---- one pyramid level of one image ----
#define KP_T 16                   // output tile
#define KP_R (2 * KP_T + 3)       // source rows under it
__global__ __launch_bounds__(KP_T * KP_T) void k_klt_pyr(const uint8_t* __restrict__ src, int sw, int sh, int64_t sstep,
                                                          uint8_t* __restrict__ dst, int dw, int dh) {
    __shared__ uint16_t hsum[KP_R][KP_T];   // <= 16 * 255
    const int x0 = blockIdx.x * KP_T, y0 = blockIdx.y * KP_T;
    for (int e = threadIdx.x; e < KP_R * KP_T; e += KP_T * KP_T) {
        const int r = e / KP_T, c = e % KP_T;
        // rows and columns past the level (a partial tile) are clamped reads that nothing uses
        const uint8_t* row = src + (int64_t)lh_klt_reflect(2 * y0 - 2 + r, sh) * sstep;
        hsum[r][c] = (uint16_t)lh_klt_pyr_row(row, sw, min(x0 + c, dw - 1));
    }
    __syncthreads();
    const int tx = threadIdx.x % KP_T, ty = threadIdx.x / KP_T;
    const int x = x0 + tx, y = y0 + ty;
    if (x < dw && y < dh)
        dst[(int64_t)y * dw + x] =
            lh_klt_pyr_col(hsum[2 * ty][tx], hsum[2 * ty + 1][tx], hsum[2 * ty + 2][tx], hsum[2 * ty + 3][tx], hsum[2 * ty + 4][tx]);
}

// ---- the tracker, one wave per keypoint ----
#define KW 4                      // keypoints (waves) per workgroup
#define KT_I 14                   // I tile: ip - 1 .. ip + 12
#define KT_D 12                   // derivative tile: ip .. ip + 11
#define KT_WW 32                  // J window
#define KT_WH 24
#define KT_WX 10                  // the first q's corner sits at (KT_WX, KT_WY) of the window: q may then move
#define KT_WY 6                   // +-10 columns and +-6 rows before its taps leave it

namespace {

__device__ __forceinline__ void wave_sync() {   // LDS written by one lane, read by another of the same wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The wave's total of one int32 partial per lane, every lane getting it.  The sums are exact integers, so the order
// is free.  |ix|, |iy| <= 4081 and |Iw|, |Jw| <= 8161 (w11 may round to -1), and a half-wave holds at most 64 of the
// 121 pixels: its sum is at most 64 * 8161 * 4081 = 2.13e9 < 2^31.  So five stages run in int32 and the last one,
// across the halves, in int64 (a mismatch total passes 2^31).
__device__ __forceinline__ int half_sum(int v) {
#pragma unroll
    for (int m = 1; m <= 16; m <<= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int64_t wave_sum(int v) {
    v = half_sum(v);
    return (int64_t)v + (int64_t)__shfl_xor(v, 32);
}

__device__ __forceinline__ int byte_at(const lh_klt_levels& v, int l, int x, int y) {
    return v.data[l][(int64_t)lh_klt_reflect(y, v.rows[l]) * v.step[l] + lh_klt_reflect(x, v.cols[l])];
}

struct WaveSums {
    const lh_klt_levels &I, &J;
    uint8_t* ti;       // [KT_I * KT_I]
    short2* td;        // [KT_D * KT_D] (Ix, Iy)
    uint8_t* win;      // [KT_WH * KT_WW]
    int lane;
    int win_level, wx0, wy0;
    int iw[2], dx[2], dy[2];   // pixels lane and lane + 64 of the 11 x 11 window, row-major

    __device__ void window(int l, int ipx, int ipy, const int w[4], int64_t S[3]) {
        wave_sync();   // the last level's reads of the tiles are done
        for (int k = lane; k < KT_I * KT_I; k += 64)
            ti[k] = (uint8_t)byte_at(I, l, ipx - 1 + k % KT_I, ipy - 1 + k / KT_I);
        wave_sync();
        for (int k = lane; k < KT_D * KT_D; k += 64) {
            const int c = k % KT_D, r = k / KT_D;
            int gx = 0, gy = 0;
            if ((unsigned)(ipx + c) < (unsigned)I.cols[l] && (unsigned)(ipy + r) < (unsigned)I.rows[l]) {
                int nb[3][3];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) nb[a][b] = ti[(r + a) * KT_I + c + b];
                lh_klt_scharr(nb, &gx, &gy);
            }
            td[k] = make_short2((short)gx, (short)gy);   // |.| <= 4080
        }
        wave_sync();
        int s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int k = lane + 64 * t;
            iw[t] = dx[t] = dy[t] = 0;
            if (k < LH_KLT_WIN * LH_KLT_WIN) {
                const int x = k % LH_KLT_WIN, y = k / LH_KLT_WIN;
                const uint8_t* p = ti + (y + 1) * KT_I + x + 1;
                iw[t] = lh_klt_descale_img(lh_klt_bil(p[0], p[1], p[KT_I], p[KT_I + 1], w));
                const short2* d = td + y * KT_D + x;
                const short2 d00 = d[0], d01 = d[1], d10 = d[KT_D], d11 = d[KT_D + 1];
                dx[t] = lh_klt_descale_der(lh_klt_bil(d00.x, d01.x, d10.x, d11.x, w));
                dy[t] = lh_klt_descale_der(lh_klt_bil(d00.y, d01.y, d10.y, d11.y, w));
                s11 += dx[t] * dx[t];
                s12 += dx[t] * dy[t];
                s22 += dy[t] * dy[t];
            }
        }
        S[0] = wave_sum(s11);
        S[1] = wave_sum(s12);
        S[2] = wave_sum(s22);
    }

    __device__ void mismatch(int l, int iqx, int iqy, const int w[4], int64_t B[2]) {
        if (win_level != l) {   // the level's first q: stage J around it
            win_level = l;
            wx0 = iqx - KT_WX;
            wy0 = iqy - KT_WY;
            wave_sync();
            for (int k = lane; k < KT_WH * KT_WW; k += 64)
                win[k] = (uint8_t)byte_at(J, l, wx0 + k % KT_WW, wy0 + k / KT_WW);
            wave_sync();
        }
        const int c0 = iqx - wx0, r0 = iqy - wy0;
        const bool staged = (unsigned)c0 <= KT_WW - KT_D && (unsigned)r0 <= KT_WH - KT_D;   // all 12 x 12 taps inside
        int b1 = 0, b2 = 0;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int k = lane + 64 * t;
            if (k < LH_KLT_WIN * LH_KLT_WIN) {
                const int x = k % LH_KLT_WIN, y = k / LH_KLT_WIN;
                int j00, j01, j10, j11;
                if (staged) {
                    const uint8_t* p = win + (r0 + y) * KT_WW + c0 + x;
                    j00 = p[0]; j01 = p[1]; j10 = p[KT_WW]; j11 = p[KT_WW + 1];
                } else {
                    j00 = byte_at(J, l, iqx + x, iqy + y);
                    j01 = byte_at(J, l, iqx + x + 1, iqy + y);
                    j10 = byte_at(J, l, iqx + x, iqy + y + 1);
                    j11 = byte_at(J, l, iqx + x + 1, iqy + y + 1);
                }
                const int diff = lh_klt_descale_img(lh_klt_bil(j00, j01, j10, j11, w)) - iw[t];
                b1 += diff * dx[t];
                b2 += diff * dy[t];
            }
        }
        B[0] = wave_sum(b1);
        B[1] = wave_sum(b2);
    }
};

}  // namespace

__global__ __launch_bounds__(64 * KW) void k_klt_track(lh_klt_args a) {
    __shared__ uint8_t tile_i[KW][KT_I * KT_I + 12];   // 208 bytes: 16-byte aligned rows of the array
    __shared__ short2 tile_d[KW][KT_D * KT_D];
    __shared__ uint8_t window[KW][KT_WH * KT_WW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * KW + wv;
    if (i >= a.n_points) return;   // wave-uniform: no barrier below spans waves
    WaveSums sums{a.I, a.J, tile_i[wv], tile_d[wv], window[wv], lane, -1, 0, 0, {0, 0}, {0, 0}, {0, 0}};
    const float k1x = a.kp1[2 * i], k1y = a.kp1[2 * i + 1];
    const float gx = a.has_initial ? a.kp2[2 * i] : k1x, gy = a.has_initial ? a.kp2[2 * i + 1] : k1y;
    float ox, oy;
    int ok;
    lh_klt_track_point(sums, a.n_levels, a.I.cols, a.I.rows, k1x, k1y, gx, gy, a.max_iters, a.eps2, a.min_eig, &ox, &oy, &ok);
    if (lane == 0) {
        a.kp2[2 * i] = ox;
        a.kp2[2 * i + 1] = oy;
        a.success[i] = (uint8_t)ok;
    }
}

extern "C" {

hipError_t lh_launch_klt_pyr(hipStream_t st, const uint8_t* src, int sw, int sh, int64_t sstep, uint8_t* dst, int dw, int dh) {
    if (dw <= 0 || dh <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_klt_pyr, dim3((unsigned)((dw + KP_T - 1) / KP_T), (unsigned)((dh + KP_T - 1) / KP_T)), dim3(KP_T * KP_T),
                       0, st, src, sw, sh, sstep, dst, dw, dh);
    return hipGetLastError();
}

hipError_t lh_launch_klt_track(hipStream_t st, const lh_klt_args* a) {
    if (a->n_points <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_klt_track, dim3((unsigned)((a->n_points + KW - 1) / KW)), dim3(64 * KW), 0, st, *a);
    return hipGetLastError();
}

}  // extern "C"
