// lh_gftt.hip — Shi-Tomasi corner detection on the device (lh_detect_features; the arithmetic: lh_gftt.h).
//
//   k_gftt_boxes    one workgroup per exclusion point: clears its box in the allow image
//   k_gftt_eig      32 x 8 pixel tiles: the tile and a 2-pixel halo of bytes into LDS, the Sobel gradients on the
//                   tile and a 1-pixel halo, the 3x3 sums of their products, lambda; the maximum over allowed
//                   pixels folded with integer atomics on an order-preserving key (max is exact in any order)
//   k_gftt_cand     threshold, 3x3 non-maximum test and mask per interior pixel; the candidates' raster indices
//                   compacted in arrival order, which nothing below depends on
//   k_gftt_round    one selection round, one wave per undecided candidate: it scans the state bytes of the pixels
//                   within min_distance, a word at a time, for stronger candidates.  One of them accepted: rejected.  All of them rejected:
//                   accepted.  Otherwise it stays open for the next round.  A state never changes once decided
//                   and every decision rests on decided states alone, so the result is the serial greedy walk's
//                   whatever a round sees of the decisions made beside it.
//   k_gftt_accepted the accepted candidates compacted (arrival order again)
//   k_gftt_rank     each accepted corner counts the accepted corners stronger than itself: that count is its
//                   place in the output, written if it is below the limit (one wave per corner, its lanes
//                   striding the list)
//
// No floating-point atomic touches a value that reaches the output.
#include <hip/hip_runtime.h>

#include "lh_launch.h"

#define GF_TW 32
#define GF_TH 8
#define GF_BLOCK 256
#define GF_GRID 1024   // grid-stride kernels: their lists' lengths are known on the device only

__global__ __launch_bounds__(GF_BLOCK) void k_gftt_boxes(lh_gftt_args a) {
    const int b = blockIdx.x;
    int x0, x1, y0, y1;
    lh_gftt_box_axis(a.exclude_pt[2 * b], a.exclude_half, a.cols, &x0, &x1);
    lh_gftt_box_axis(a.exclude_pt[2 * b + 1], a.exclude_half, a.rows, &y0, &y1);
    if (x0 > x1 || y0 > y1) return;
    const int w = x1 - x0 + 1;
    const int n = w * (y1 - y0 + 1);   // within the image: below 2^31
    for (int i = threadIdx.x; i < n; i += GF_BLOCK) a.allow[(int64_t)(y0 + i / w) * a.cols + x0 + i % w] = 0;
}

__global__ __launch_bounds__(GF_BLOCK) void k_gftt_eig(lh_gftt_args a) {
    __shared__ uint8_t s_img[GF_TH + 4][GF_TW + 4];
    __shared__ short s_gx[GF_TH + 2][GF_TW + 2], s_gy[GF_TH + 2][GF_TW + 2];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * GF_TW, y0 = blockIdx.y * GF_TH;
    // LDS position (ry, rx) holds the image at the reflected coordinate of (y0 - 2 + ry, x0 - 2 + rx)
    for (int i = tid; i < (GF_TH + 4) * (GF_TW + 4); i += GF_BLOCK) {
        const int ry = i / (GF_TW + 4), rx = i % (GF_TW + 4);
        s_img[ry][rx] = a.img[(int64_t)lh_gftt_reflect(y0 - 2 + ry, a.rows) * a.cols + lh_gftt_reflect(x0 - 2 + rx, a.cols)];
    }
    __syncthreads();
    // the gradient at (y0 - 1 + gy, x0 - 1 + gx); a position one past the image is the gradient at its mirror
    // position inside (the product images are what REFLECT_101 extends), whose own taps lie within the loaded
    // region: the mirror of -1 is 1, with taps 0..2, and the mirror of n is n - 2, with taps n - 3..n - 1
    for (int i = tid; i < (GF_TH + 2) * (GF_TW + 2); i += GF_BLOCK) {
        const int gy = i / (GF_TW + 2), gx = i % (GF_TW + 2);
        const int cx = x0 - 1 + gx, cy = y0 - 1 + gy;
        int vx = 0, vy = 0;
        if (cx >= -1 && cx <= a.cols && cy >= -1 && cy <= a.rows) {
            const int px = lh_gftt_reflect(cx, a.cols) - (x0 - 2), py = lh_gftt_reflect(cy, a.rows) - (y0 - 2);
            if (px >= 1 && px <= GF_TW + 2 && py >= 1 && py <= GF_TH + 2) {   // always, for a gradient a pixel of this tile uses
                int t[3][3];
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) t[dy][dx] = s_img[py - 1 + dy][px - 1 + dx];
                lh_gftt_sobel(t, &vx, &vy);
            }
        }
        s_gx[gy][gx] = (short)vx;
        s_gy[gy][gx] = (short)vy;
    }
    __syncthreads();
    const int lx = tid % GF_TW, ly = tid / GF_TW;
    const int x = x0 + lx, y = y0 + ly;
    unsigned long long key = 0;
    if (x < a.cols && y < a.rows) {
        int32_t A = 0, B = 0, C = 0;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int gx = s_gx[ly + dy][lx + dx], gy = s_gy[ly + dy][lx + dx];
                A += gx * gx;
                B += gx * gy;
                C += gy * gy;
            }
        const double lam = lh_gftt_lambda(A, B, C);
        const int64_t p = (int64_t)y * a.cols + x;
        a.eig[p] = lam;
        if (a.allow[p]) key = lh_gftt_key(lam);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(key, m, 64);
        key = o > key ? o : key;
    }
    // one atomic per workgroup: thousands on one address would serialise in the L2
    __shared__ unsigned long long s_key[GF_BLOCK / 64];
    if ((tid & 63) == 0) s_key[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < GF_BLOCK / 64; ++w) key = s_key[w] > key ? s_key[w] : key;
        if (key) atomicMax(&a.ctl->max_key, key);
    }
}

__global__ __launch_bounds__(GF_BLOCK) void k_gftt_cand(lh_gftt_args a) {
    __shared__ uint32_t s_count, s_base;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * GF_BLOCK + threadIdx.x;
    const bool inside = p < (int64_t)a.rows * a.cols;
    const int x = inside ? (int)(p % a.cols) : 0, y = inside ? (int)(p / a.cols) : 0;
    const unsigned long long mk = a.ctl->max_key;
    const double lmax = mk ? lh_gftt_unkey(mk) : 0.0;
    bool top = false;
    if (inside && lmax > 0.0 && x >= 1 && x <= a.cols - 2 && y >= 1 && y <= a.rows - 2 && a.allow[p]) {
        const double l = a.eig[p];
        if (l > a.quality * lmax) {
            top = true;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) top = top && l >= a.eig[p + (int64_t)dy * a.cols + dx];
        }
    }
    // a slot in the workgroup's share of the list, then one global atomic per workgroup
    const uint32_t slot = top ? atomicAdd(&s_count, 1u) : 0u;
    __syncthreads();
    if (threadIdx.x == 0 && s_count) s_base = atomicAdd(&a.ctl->n_cand, s_count);
    __syncthreads();
    if (top) a.cand[s_base + slot] = (uint32_t)p;
    if (inside) a.state[p] = top ? (a.reach < 0 ? LH_GFTT_S_TAKEN : LH_GFTT_S_OPEN) : LH_GFTT_S_NONE;
}

__global__ __launch_bounds__(GF_BLOCK) void k_gftt_round(lh_gftt_args a, int round) {
    lh_gftt_ctl* ctl = a.ctl;
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->open[(round + 1) % 3] = 0;   // the next round's flag; nobody reads it now
    const uint32_t n = ctl->n_cand;
    if ((round ? ctl->open[(round - 1) % 3] : n) == 0) return;
    __shared__ int s_open;
    if (threadIdx.x == 0) s_open = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * (GF_BLOCK / 64);
    int left_open = 0;
    for (uint32_t c = blockIdx.x * (GF_BLOCK / 64) + (threadIdx.x >> 6); c < n; c += waves) {
        const uint32_t p = a.cand[c];
        if (a.state[p] != LH_GFTT_S_OPEN) continue;
        const double lam = a.eig[p];
        const int x = (int)(p % (uint32_t)a.cols), y = (int)(p / (uint32_t)a.cols);
        const int xa = max(x - a.reach, 0), xb = min(x + a.reach, a.cols - 1);
        const int ya = max(y - a.reach, 0), yb = min(y + a.reach, a.rows - 1);
        // the window's state bytes, four to an aligned word (a candidate in 9 to 30 pixels: most words are zero);
        // a wave takes four rows at a time, sixteen lanes to a row
        const uint32_t* state32 = (const uint32_t*)a.state;   // padded by a word past the image
        int taken = 0, open = 0;
        for (int qy = ya + (lane >> 4); qy <= yb; qy += 4) {
            const uint32_t first = (uint32_t)qy * (uint32_t)a.cols + (uint32_t)xa, last = first + (uint32_t)(xb - xa);
            for (uint32_t wd = (first >> 2) + (lane & 15); wd <= (last >> 2); wd += 16) {
                const uint32_t v = state32[wd];
                if (!v) continue;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t s = (v >> (8 * k)) & 0xffu, q = 4 * wd + k;
                    if ((s != LH_GFTT_S_OPEN && s != LH_GFTT_S_TAKEN) || q < first || q > last) continue;
                    const int64_t dx = (int)(q - first) + xa - x, dy = qy - y;
                    if (!((double)(dx * dx + dy * dy) < a.min_dist2)) continue;
                    if (!lh_gftt_stronger(a.eig[q], q, lam, p)) continue;   // (p itself is not stronger than p)
                    if (s == LH_GFTT_S_TAKEN) taken = 1;
                    else open = 1;
                }
            }
        }
        taken = __any(taken);
        open = __any(open);
        if (lane == 0) {
            if (taken) a.state[p] = LH_GFTT_S_DROPPED;
            else if (!open) a.state[p] = LH_GFTT_S_TAKEN;
            else left_open = 1;
        }
    }
    // one plain store per workgroup (every writer stores the same 1): an atomic per open candidate, thousands on
    // one address in the first rounds, would serialise in the L2
    if (left_open) s_open = 1;
    __syncthreads();
    if (threadIdx.x == 0 && s_open) ctl->open[round % 3] = 1;
}

__global__ __launch_bounds__(GF_BLOCK) void k_gftt_accepted(lh_gftt_args a) {
    const uint32_t n = a.ctl->n_cand;
    for (uint32_t c = blockIdx.x * GF_BLOCK + threadIdx.x; c < n; c += gridDim.x * GF_BLOCK) {
        const uint32_t p = a.cand[c];
        if (a.state[p] != LH_GFTT_S_TAKEN) continue;
        const uint32_t k = atomicAdd(&a.ctl->n_acc, 1u);
        a.acc_idx[k] = p;
        a.acc_lam[k] = a.eig[p];
    }
}

__global__ __launch_bounds__(GF_BLOCK) void k_gftt_rank(lh_gftt_args a) {
    const uint32_t n = a.ctl->n_acc;
    const int lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * (GF_BLOCK / 64);
    for (uint32_t i = blockIdx.x * (GF_BLOCK / 64) + (threadIdx.x >> 6); i < n; i += waves) {   // one wave per corner
        const double lam = a.acc_lam[i];
        const uint32_t idx = a.acc_idx[i];
        uint32_t rank = 0;
        for (uint32_t j = lane; j < n; j += 64) rank += lh_gftt_stronger(a.acc_lam[j], a.acc_idx[j], lam, idx) ? 1u : 0u;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) rank += __shfl_xor(rank, m, 64);
        if (lane == 0 && rank < (uint32_t)a.limit) {
            a.kp[2 * rank] = (float)(idx % (uint32_t)a.cols);
            a.kp[2 * rank + 1] = (float)(idx / (uint32_t)a.cols);
            a.response[rank] = lam;
        }
    }
}

// The eigenvalue image, the masked maximum and the candidates (a->ctl zeroed by the caller on the same stream).
extern "C" hipError_t lh_launch_gftt_front(hipStream_t st, const lh_gftt_args* a) {
    if (a->n_exclude > 0) hipLaunchKernelGGL(k_gftt_boxes, dim3((unsigned)a->n_exclude), dim3(GF_BLOCK), 0, st, *a);
    hipLaunchKernelGGL(k_gftt_eig, dim3((unsigned)((a->cols + GF_TW - 1) / GF_TW), (unsigned)((a->rows + GF_TH - 1) / GF_TH)),
                       dim3(GF_BLOCK), 0, st, *a);
    const int64_t px = (int64_t)a->rows * a->cols;
    hipLaunchKernelGGL(k_gftt_cand, dim3((unsigned)((px + GF_BLOCK - 1) / GF_BLOCK)), dim3(GF_BLOCK), 0, st, *a);
    return hipGetLastError();
}

// Selection rounds first .. first + count - 1.
extern "C" hipError_t lh_launch_gftt_rounds(hipStream_t st, const lh_gftt_args* a, int first, int count) {
    for (int r = first; r < first + count; ++r) hipLaunchKernelGGL(k_gftt_round, dim3(GF_GRID), dim3(GF_BLOCK), 0, st, *a, r);
    return hipGetLastError();
}

// The accepted corners in descending (lambda, index), the first a->limit of them.
extern "C" hipError_t lh_launch_gftt_order(hipStream_t st, const lh_gftt_args* a) {
    hipLaunchKernelGGL(k_gftt_accepted, dim3(GF_GRID), dim3(GF_BLOCK), 0, st, *a);
    hipLaunchKernelGGL(k_gftt_rank, dim3(GF_GRID), dim3(GF_BLOCK), 0, st, *a);
    return hipGetLastError();
}
