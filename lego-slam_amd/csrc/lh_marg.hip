// lh_marg.hip — the kernels of lh_marginalize (include/lego_ba.h; arguments and the scheme: lh_marg.h).
//   k_marg_mask      one wave per sub-batch, one lane per observation (k_lin's decomposition): a lane-group ballot
//                    decides whether the landmark has a valid edge to pose m; the observation words are copied with
//                    LH_META_VALID cleared on the edges of every other landmark, on which the host then runs
//                    k_lin<T, false> and k_reduce (mode 0) unchanged;
//   k_marg_assemble  one workgroup: the packed pair blocks plus the earlier prior into the lower triangle of A
//                    (global, L2-resident), b likewise; the 6x6 factor of A[m, m]; Y = C^-1 A[m, :], y = C^-1 b[m];
//   k_marg_schur     one thread per entry of H_prior = A[r, r] - Y^T Y (each entry from the lower triangle's value
//                    and a sum that is symmetric in its operands, so the transpose is equal by bits), and b_prior.
// Every sum has a fixed order, so two calls return the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lh_launch.h"
#include "lh_dev.h"

#pragma clang fp contract(fast)

constexpr int MAT = 1024;                 // k_marg_assemble's threads

__global__ __launch_bounds__(256) void k_marg_mask(lh_marg_mask_args a) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sb = blockIdx.x * LH_WAVES + wave;
    if (sb >= a.n_sb) return;   // (wave-uniform; no workgroup barrier below)
    const lh_subbatch S = a.sbs[sb];
    const int lg = S.lg, nlm = S.n_lm;
    const int ls = lane >> lg, gj = lane & ((1 << lg) - 1);
    const bool lmok = ls < nlm;
    const bool lead = gj == 0 && lmok;
    const int o = sb * 64 + lane;
    const uint32_t meta = a.obs_meta[o];
    const bool has = (meta & LH_META_VALID) != 0u;
    const uint64_t tmask = __ballot(has && (int)LH_META_POSE(meta) == a.marg_pose);
    const uint64_t gmask = (lg >= 6) ? ~0ull : (((1ull << (1 << lg)) - 1ull) << (lane & ~((1 << lg) - 1)));
    const bool in = (tmask & gmask) != 0ull;
    a.meta_out[o] = in ? meta : (meta & ~LH_META_VALID);
    const int n_lm = __popcll(__ballot(lead && in)), n_edge = __popcll(__ballot(has && in));
    const int n_out = __popcll(__ballot(lead && !in));
    if (lead) {
        const int l = a.lm_perm[sb * LH_SB_LM + ls];
        if (l >= 0) a.lm_marg[l] = in ? 1 : 0;
    }
    if (lane < 3) a.counts[3 * (size_t)sb + lane] = lane == 0 ? n_lm : (lane == 1 ? n_edge : n_out);
}

__device__ __forceinline__ bool marg_fixed(const uint64_t* __restrict__ fixed_bits, int p) {
    return ((fixed_bits[p >> 6] >> (p & 63)) & 1ull) != 0ull;
}

__global__ __launch_bounds__(MAT) void k_marg_assemble(lh_marg_args a) {
    __shared__ double s_a[36], s_c[36];
    __shared__ int s_cnt[3][MAT / 64];
    __shared__ int s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n6 = 6 * a.P, m = a.marg_pose;
    const bool elim = !marg_fixed(a.fixed_bits, m);
    const lh_rs_layout LY = lh_rs_make(a.P, a.npairs);
    for (int i = tid; i < n6 * n6; i += MAT) a.A[i] = 0.0;
    __syncthreads();
    // the lower triangle of A_M from the pair blocks (block b holds S(6p + i, 6q + j), p <= q, at 36 b + 6 i + j: its
    // lower slot is (6q + j, 6p + i))
    for (int e = tid; e < a.npairs * 36; e += MAT) {
        const int b = e / 36, k = e - 36 * b, i = k / 6, j = k - 6 * i;
        const int p = a.pair_pq[2 * b], q = a.pair_pq[2 * b + 1];
        if (p >= a.P || q >= a.P || (p == q && i < j)) continue;
        const int fr = 6 * p + i, fc = 6 * q + j;
        a.A[(size_t)max(fr, fc) * n6 + min(fr, fc)] = a.rs[LY.off_S + e];   // (p < q: fr < fc; p == q: fr >= fc)
    }
    __syncthreads();
    // the earlier prior, a fixed pose's rows and columns zero (problem.cpp:343-351)
    if (a.prior_H) {
        for (int i = tid; i < n6 * n6; i += MAT) {
            const int r = i / n6, c = i - n6 * r;
            if (c > r || marg_fixed(a.fixed_bits, r / 6) || marg_fixed(a.fixed_bits, c / 6)) continue;
            a.A[i] = a.A[i] + a.prior_H[i];
        }
    }
    if (tid < n6) {
        double v = a.rs[LY.off_bs + tid];
        if (a.prior_b && !marg_fixed(a.fixed_bits, tid / 6)) v += a.prior_b[tid];
        a.b[tid] = v;
    }
    // the counts over the sub-batches (integers: any order gives the same sums)
    int c0 = 0, c1 = 0, c2 = 0;
    for (int i = tid; i < a.n_sb; i += MAT) { c0 += a.counts[3 * i]; c1 += a.counts[3 * i + 1]; c2 += a.counts[3 * i + 2]; }
    for (int off = 32; off > 0; off >>= 1) { c0 += __shfl_xor(c0, off); c1 += __shfl_xor(c1, off); c2 += __shfl_xor(c2, off); }
    if (lane == 0) { s_cnt[0][wave] = c0; s_cnt[1][wave] = c1; s_cnt[2][wave] = c2; }
    __syncthreads();   // (also orders A's and b's global stores before the loads below: one CU, one L1)
    if (tid < 36) {
        const int i = tid / 6, j = tid - 6 * i;
        s_a[tid] = a.A[(size_t)(6 * m + max(i, j)) * n6 + 6 * m + min(i, j)];
    }
    __syncthreads();
    if (tid == 0) {
        double minp = 0.0, maxp = 0.0;
        s_bad = elim ? lh_marg_chol6(s_a, s_c, &minp, &maxp) : -1;
        int n0 = 0, n1 = 0, n2 = 0;
        for (int w = 0; w < MAT / 64; ++w) { n0 += s_cnt[0][w]; n1 += s_cnt[1][w]; n2 += s_cnt[2][w]; }
        a.res[LH_MARG_R_BAD] = (double)s_bad;
        a.res[LH_MARG_R_MINP] = minp;
        a.res[LH_MARG_R_MAXP] = maxp;
        a.res[LH_MARG_R_ELIM] = elim ? 1.0 : 0.0;
        a.res[LH_MARG_R_NDEG] = a.rs[LY.off_sc + LH_SC_NDEG] - (double)n2;
        a.res[LH_MARG_R_NLM] = (double)n0;
        a.res[LH_MARG_R_NEDGE] = (double)n1;
        a.res[7] = 0.0;
    }
    __syncthreads();
    if (!elim || s_bad >= 0) return;
    // Y(:, c) = C^-1 A[m, c] (A symmetric: its lower slot), one thread per column; y = C^-1 b[m]
    if (tid < n6) {
        double x[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int r = 6 * m + k;
            x[k] = a.A[(size_t)max(r, tid) * n6 + min(r, tid)];
        }
        lh_marg_fwd6(s_c, x, 1);
#pragma unroll
        for (int k = 0; k < 6; ++k) a.Y[(size_t)k * n6 + tid] = x[k];
    } else if (tid == n6) {
        double x[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) x[k] = a.b[6 * m + k];
        lh_marg_fwd6(s_c, x, 1);
#pragma unroll
        for (int k = 0; k < 6; ++k) a.y[k] = x[k];
    }
}

// H_prior(r, c) = A(r, c) - sum_k Y(k, r) Y(k, c) off m's rows and columns (A alone when m is fixed), +0.0 on them;
// the last workgroup: b_prior
__global__ __launch_bounds__(256) void k_marg_schur(lh_marg_args a) {
    if (a.res[LH_MARG_R_BAD] >= 0.0) return;
    const bool elim = a.res[LH_MARG_R_ELIM] != 0.0;
    const int n6 = 6 * a.P, m = a.marg_pose;
    const int nb = (n6 * n6 + 255) / 256;
    if ((int)blockIdx.x == nb) {
        for (int r = threadIdx.x; r < n6; r += 256) {
            double v = 0.0;
            if (r / 6 != m) v = elim ? lh_marg_update(a.b[r], a.Y + r, a.y, n6, 1) : a.b[r] + 0.0;
            a.b_prior[r] = v;
        }
        return;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n6 * n6) return;
    const int r = i / n6, c = i - n6 * r;
    double v = 0.0;
    if (r / 6 != m && c / 6 != m) {
        const double av = a.A[(size_t)max(r, c) * n6 + min(r, c)];
        v = elim ? lh_marg_update(av, a.Y + r, a.Y + c, n6, n6) : av + 0.0;
    }
    a.H_prior[i] = v;
}

extern "C" {

hipError_t lh_launch_marg_mask(hipStream_t st, const lh_marg_mask_args* a) {
    if (a->n_sb <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_marg_mask, dim3((a->n_sb + LH_WAVES - 1) / LH_WAVES), dim3(256), 0, st, *a);
    return hipGetLastError();
}

// A, the factor of A[m, m], and the prior (a->P <= LH_PMAX_WIN, 0 <= a->marg_pose < a->P)
hipError_t lh_launch_marg_prior(hipStream_t st, const lh_marg_args* a) {
    if (a->P <= 0 || a->P > LH_PMAX_WIN || a->marg_pose < 0 || a->marg_pose >= a->P) return hipErrorInvalidValue;
    const int n6 = 6 * a->P;
    hipLaunchKernelGGL(k_marg_assemble, dim3(1), dim3(MAT), 0, st, *a);
    hipLaunchKernelGGL(k_marg_schur, dim3((n6 * n6 + 255) / 256 + 1), dim3(256), 0, st, *a);
    return hipGetLastError();
}

}  // extern "C"
