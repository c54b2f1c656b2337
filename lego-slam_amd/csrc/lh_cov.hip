// lh_cov.hip — the kernels of lh_covariance (include/lego_ba.h; arguments and the scheme: lh_cov.h).
//   k_cov_snapshot  the committed poses, pose tables and landmarks into a second set of lh_reset_args, on which the
//                   host then runs k_lin<T, false> and k_reduce (mode 0) unchanged;
//   k_cov_factor    one workgroup: the free rows of the packed S compacted into A (global, L2-resident), blocked
//                   right-looking Cholesky over 16-column panels staged in LDS;
//   k_cov_linv      W = L^-1, one workgroup per 16-column block column (the unit right-hand sides are independent);
//   k_cov_gram      Sigma[f, f] = W^T W, one workgroup per 16x16 tile of the lower triangle, mirrored on the store;
//   k_cov_lm        one wave per sub-batch, one lane per observation (k_lin's decomposition): H_lp per edge, the sum
//                   over the landmark's lane group, the record's factor on both sides.
// Every sum has a fixed order, so two calls return the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lh_launch.h"
#include "lh_dev.h"
#include "lh_edge.h"

#pragma clang fp contract(fast)

constexpr int CNB = LH_COV_NB;
constexpr int CPS = CNB + 1;              // LDS row stride of a 16-column panel (conflict-free column walks)
constexpr int CFT = 1024;                 // k_cov_factor's threads

__global__ __launch_bounds__(256) void k_cov_snapshot(lh_cov_snap_args a) {
    const int cur = __builtin_amdgcn_readfirstlane(a.ctrl->cur) & 1;
    const int i0 = blockIdx.x * 256 + threadIdx.x, st = gridDim.x * 256;
    const int nq = a.P * 12;
    for (int i = i0; i < nq; i += st) {
        const double v = a.qt[(size_t)cur * nq + i];
        a.qt_init[i] = v;
        a.qt_init[nq + i] = v;
    }
    for (int i = i0; i < a.npt; i += st) {
        const double v = a.ptab[(size_t)cur * a.npt + i];
        a.ptab_init[i] = v;
        a.ptab_init[a.npt + i] = v;
    }
    const double* rc = a.rec + (size_t)cur * a.nrec * LH_REC;
    for (int i = i0; i < 3 * a.nrec; i += st) {
        const int r = i / 3, k = i - 3 * r;
        const int l = a.lm_perm[r];
        if (l >= 0) a.lm[3 * (size_t)l + k] = rc[(size_t)r * LH_REC + LH_REC_X + k];
    }
}

// pose p is held: fixed in the window, or the call's anchor
__device__ __forceinline__ bool cov_held(const uint64_t* __restrict__ fixed_bits, int p, int anchor) {
    return ((fixed_bits[p >> 6] >> (p & 63)) & 1ull) != 0ull || p == anchor;
}

__global__ __launch_bounds__(CFT) void k_cov_factor(lh_cov_args a) {
    __shared__ double pan[LH_COV_NSMAX * CPS];   // the panel: rows k0 .. ns - 1, 16 columns
    __shared__ int s_map[LH_COV_NSMAX];           // row of the 6P -> compact row (-1: held)
    __shared__ int s_back[LH_COV_NSMAX];          // compact row -> row of the 6P
    __shared__ int s_bad;
    __shared__ double s_piv[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n6 = 6 * a.P, ns = a.ns;
    // the compaction: six rows per pose that is not held, in pose order
    if (tid < n6) {
        const int p = tid / 6;
        int before = 0;
        for (int q = 0; q < p; ++q) before += cov_held(a.fixed_bits, q, a.anchor) ? 0 : 1;
        const int m = cov_held(a.fixed_bits, p, a.anchor) ? -1 : 6 * before + (tid - 6 * p);
        s_map[tid] = m;
        a.rowmap[tid] = m;
        if (m >= 0) s_back[m] = tid;
    }
    if (tid == 0) { s_bad = -1; s_piv[0] = 0.0; s_piv[1] = 0.0; }
    int nfree = 0;
    for (int q = 0; q < a.P; ++q) nfree += cov_held(a.fixed_bits, q, a.anchor) ? 0 : 6;
    // A: zero, the identity on the padding rows; then the lower triangle of S[f, f] from the pair blocks (block b
    // holds S(6p + i, 6q + j), p <= q, at 36 b + 6 i + j: its lower slot is (6q + j, 6p + i))
    for (int i = tid; i < ns * ns; i += CFT) {
        const int r = i / ns, c = i - ns * r;
        a.A[i] = (r == c && r >= nfree) ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < a.npairs * 36; e += CFT) {
        const int b = e / 36, k = e - 36 * b, i = k / 6, j = k - 6 * i;
        const int p = a.pair_pq[2 * b], q = a.pair_pq[2 * b + 1];
        const int fr = s_map[6 * p + i], fc = s_map[6 * q + j];
        if (fr < 0 || fc < 0 || (p == q && i < j)) continue;
        a.A[(size_t)max(fr, fc) * ns + min(fr, fc)] = a.rs[e];   // (p < q: fr < fc; p == q: fr >= fc)
    }
    __syncthreads();
    double pmin = 0.0, pmax = 0.0;   // wave 0's, of the pivots so far
    for (int k0 = 0; k0 < ns; k0 += CNB) {
        const int m = ns - k0;       // the panel's rows
        for (int i = tid; i < m * CNB; i += CFT) {
            const int r = i >> 4, c = i & 15;
            pan[r * CPS + c] = a.A[(size_t)(k0 + r) * ns + k0 + c];
        }
        __syncthreads();
        if (wave == 0) {   // the 16x16 diagonal block, in LDS
            for (int j = 0; j < CNB; ++j) {
                const double d = pan[j * CPS + j];
                if (!(d > 0.0)) {
                    if (lane == 0) s_bad = s_back[min(k0 + j, nfree - 1)];
                    break;
                }
                if (k0 + j < nfree) {
                    pmin = (pmax == 0.0) ? d : fmin(pmin, d);
                    pmax = fmax(pmax, d);
                }
                const double l = sqrt(d);
                wave_sync();
                if (lane == j) pan[j * CPS + j] = l;
                if (lane > j && lane < CNB) pan[lane * CPS + j] = pan[lane * CPS + j] / l;
                wave_sync();
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int idx = lane + 64 * u, r = idx >> 4, c = idx & 15;
                    if (c > j && r >= c) pan[r * CPS + c] -= pan[r * CPS + j] * pan[c * CPS + j];
                }
                wave_sync();
            }
        }
        __syncthreads();
        if (s_bad >= 0) break;
        // the rows below: x L_dd^T = row, one thread per row
        if (tid < m - CNB) {
            double* row = pan + (CNB + tid) * CPS;
            double x[CNB];
#pragma unroll
            for (int c = 0; c < CNB; ++c) {
                double s = row[c];
#pragma unroll
                for (int k = 0; k < c; ++k) s -= x[k] * pan[c * CPS + k];
                x[c] = s / pan[c * CPS + c];
            }
#pragma unroll
            for (int c = 0; c < CNB; ++c) row[c] = x[c];
        }
        __syncthreads();
        // L's panel back, and the trailing block A_ij -= sum_c L_ic L_jc (i >= j >= k0 + 16)
        for (int i = tid; i < m * CNB; i += CFT) {
            const int r = i >> 4, c = i & 15;
            if (r >= c) a.A[(size_t)(k0 + r) * ns + k0 + c] = pan[r * CPS + c];
        }
        const int mt = m - CNB;
        for (int i = tid; i < mt * mt; i += CFT) {
            const int r = i / mt, c = i - mt * r;
            if (c > r) continue;
            const double* li = pan + (CNB + r) * CPS;
            const double* lj = pan + (CNB + c) * CPS;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < CNB; ++k) s += li[k] * lj[k];
            double* g = a.A + (size_t)(k0 + CNB + r) * ns + k0 + CNB + c;
            *g = *g - s;
        }
        __syncthreads();   // (also orders this panel's global stores before the next panel's loads: one CU, one L1)
    }
    if (tid == 0) {
        a.res[LH_COV_R_BAD] = (double)s_bad;
        a.res[LH_COV_R_MINP] = pmin;
        a.res[LH_COV_R_MAXP] = pmax;
        a.res[LH_COV_R_NFREE] = (double)nfree;
        a.res[LH_COV_R_NDEG] = a.rs[lh_rs_make(a.P, a.npairs).off_sc + LH_SC_NDEG];
        a.res[5] = 0.0; a.res[6] = 0.0; a.res[7] = 0.0;
    }
}

// W = L^-1 by block columns: workgroup jb solves L W(:, jb) = E_jb block row by block row; thread (r, c) of 256 owns
// entry (r, c) of the current 16x16 block.  The column's blocks stay in LDS for the rows below.
__global__ __launch_bounds__(256) void k_cov_linv(lh_cov_args a) {
    __shared__ double wcol[LH_COV_NSMAX * CPS];
    __shared__ double ld[CNB * CPS], tb[CNB * CPS];
    if (a.res[LH_COV_R_BAD] >= 0.0) return;
    const int tid = threadIdx.x, r = tid >> 4, c = tid & 15;
    const int ns = a.ns, nb = ns / CNB, jb = blockIdx.x;
    for (int ib = jb; ib < nb; ++ib) {
        const double* Lrow = a.A + (size_t)(CNB * ib + r) * ns;
        double acc = (ib == jb && r == c) ? 1.0 : 0.0;
        for (int kb = jb; kb < ib; ++kb) {
            const double* lr = Lrow + CNB * kb;
            const double* wc = wcol + (CNB * (kb - jb)) * CPS + c;
#pragma unroll
            for (int k = 0; k < CNB; ++k) acc -= lr[k] * wc[k * CPS];
        }
        tb[r * CPS + c] = acc;
        ld[r * CPS + c] = Lrow[CNB * ib + c];
        lds_barrier();
        if (tid < CNB) {   // column tid of the block: forward substitution through the diagonal block
            double x[CNB];
#pragma unroll
            for (int i = 0; i < CNB; ++i) {
                double s = tb[i * CPS + tid];
#pragma unroll
                for (int k = 0; k < i; ++k) s -= ld[i * CPS + k] * x[k];
                x[i] = s / ld[i * CPS + i];
            }
#pragma unroll
            for (int i = 0; i < CNB; ++i) wcol[(CNB * (ib - jb) + i) * CPS + tid] = x[i];
        }
        lds_barrier();
        a.W[(size_t)(CNB * ib + r) * ns + CNB * jb + c] = wcol[(CNB * (ib - jb) + r) * CPS + c];
    }
}

// Sigma[f, f] = W^T W: tile (I, J), I >= J, entry (r, c) = sum over k >= 16 I of W(k, 16 I + r) W(k, 16 J + c), k
// ascending; stored at the rows of the 6P and mirrored (a diagonal tile: its lower half only), and into the poses'
// diagonal blocks
__global__ __launch_bounds__(256) void k_cov_gram(lh_cov_args a) {
    __shared__ double sa[CNB * CPS], sb[CNB * CPS];
    __shared__ int s_back[2 * CNB];
    if (a.res[LH_COV_R_BAD] >= 0.0) return;
    const int tid = threadIdx.x, r = tid >> 4, c = tid & 15;
    const int ns = a.ns, nb = ns / CNB, n6 = 6 * a.P;
    int I = 0, t = blockIdx.x;   // tile t of the lower triangle, row-major
    while (t > I) { t -= I + 1; ++I; }
    const int J = t;
    const int nfree = (int)a.res[LH_COV_R_NFREE];
    // the tile's compact rows and columns back to rows of the 6P
    for (int i = tid; i < n6; i += 256) {
        const int m = a.rowmap[i];
        if (m >= CNB * I && m < CNB * I + CNB) s_back[m - CNB * I] = i;
        if (m >= CNB * J && m < CNB * J + CNB) s_back[CNB + m - CNB * J] = i;
    }
    double acc = 0.0;
    for (int kb = I; kb < nb; ++kb) {
        lds_barrier();
        sa[r * CPS + c] = a.W[(size_t)(CNB * kb + r) * ns + CNB * I + c];
        sb[r * CPS + c] = a.W[(size_t)(CNB * kb + r) * ns + CNB * J + c];
        lds_barrier();
#pragma unroll
        for (int k = 0; k < CNB; ++k) acc += sa[k * CPS + r] * sb[k * CPS + c];
    }
    const int fr = CNB * I + r, fc = CNB * J + c;
    if (fr >= nfree || fc >= nfree || (I == J && c > r)) return;
    const int gr = s_back[r], gc = s_back[CNB + c];
    a.full[(size_t)gr * n6 + gc] = acc;
    a.full[(size_t)gc * n6 + gr] = acc;
    if (gr / 6 == gc / 6) {
        double* blk = a.blocks + 36 * (gr / 6);
        blk[6 * (gr % 6) + gc % 6] = acc;
        blk[6 * (gc % 6) + gr % 6] = acc;
    }
}

// One wave per sub-batch, one lane per observation.  Each lane recomputes its edge's W, J_p, J_l at the committed
// state (what k_lin's back substitution does) and forms H_pl,e = J_p^T W J_l (6x3, zero for an edge to a held pose);
// then V_e = sum over the landmark's lanes e' of Sigma_pp[p(e), p(e')] H_pl,e' (Sigma_pp read through L2, not staged:
// DESIGN.md 2.12), M = sum_e H_lp,e V_e by the lane-group butterfly, and the lead lane applies the record's factor
// on both sides.
template <bool F32>
__global__ __launch_bounds__(256) void k_cov_lm(lh_cov_lm_args a, lh_params prm) {
    __shared__ double s_h[LH_WAVES][64 * 19];
    __shared__ int s_p[LH_WAVES][64];
    if (a.res[LH_COV_R_BAD] >= 0.0) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sb = blockIdx.x * LH_WAVES + wave;
    if (sb >= a.n_sb) return;   // (wave-uniform; no workgroup barrier below)
    const lh_subbatch S = a.sbs[sb];
    const int lg = S.lg, nlm = S.n_lm;
    const int ls = lane >> lg, gj = lane & ((1 << lg) - 1);
    const bool lmok = ls < nlm;
    const int o = sb * 64 + lane;
    const uint32_t meta = a.obs_meta[o];
    const float2 z = reinterpret_cast<const float2*>(a.obs_uv)[o];
    const double u = (double)z.x, v = (double)z.y;
    const bool has = (meta & LH_META_VALID) != 0u && lmok;
    const int p = min((int)LH_META_POSE(meta), a.P - 1), cam = min((int)LH_META_CAM(meta), prm.ncam - 1);
    const bool live = has && a.rowmap[6 * p] >= 0;
    const int ri = sb * LH_SB_LM + (lmok ? ls : 0);
    const double* rec = a.rec + (size_t)ri * LH_REC;
    const double X[3] = {rec[LH_REC_X], rec[LH_REC_X + 1], rec[LH_REC_X + 2]};
    double hpl[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) hpl[i] = 0.0;
    if (live) {
        const double* pt = a.ptab + (size_t)(p * prm.ncam + cam) * LH_PT;
        const double* e = a.ext + cam * LH_EXT;
        const bool ext_id = (prm.ext_identity >> cam) & 1, ext_rot = (prm.ext_rot_identity >> cam) & 1;
        EdgeEval E;
        double Pc[3];
        edge_residual(pt, e, ext_id, ext_rot, X, u, v, prm, E.r0, E.r1, Pc);
        edge_robust(E, prm);
        if constexpr (F32) edge_eval_f<false, true>(pt, e, ext_id, ext_rot, X, u, v, prm, E);
        else edge_jac_pc(Pc, pt + LH_PT_RT, e, ext_rot, prm, E.Jp, E.Jl);
        double WJl[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            WJl[c] = E.W00 * E.Jl[c] + E.W01 * E.Jl[3 + c];
            WJl[3 + c] = E.W10 * E.Jl[c] + E.W11 * E.Jl[3 + c];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) hpl[3 * i + c] = jdot(E.Jp, i, WJl[c], WJl[3 + c]);
    }
    double* sh = s_h[wave];
    int* sp = s_p[wave];
#pragma unroll
    for (int i = 0; i < 18; ++i) sh[lane * 19 + i] = hpl[i];
    sp[lane] = live ? p : -1;
    wave_sync();
    // V = sum_e' Sigma(p, p(e')) H_pl,e', e' over the lane group in lane order
    double V[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) V[i] = 0.0;
    const int g0 = lane - gj, G = 1 << lg;
    if (live) {
        const int n6 = 6 * a.P;
        for (int j = 0; j < G; ++j) {
            const int q = sp[g0 + j];
            if (q < 0) continue;
            const double* h = sh + (g0 + j) * 19;
            const double* sg = a.full + (size_t)(6 * p) * n6 + 6 * q;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const double s = sg[(size_t)i * n6 + k];
#pragma unroll
                    for (int c = 0; c < 3; ++c) V[3 * i + c] += s * h[3 * k + c];
                }
        }
    }
    // M (upper triangle) = sum_e H_lp,e V_e
    double M[6];
    {
        int k = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int d = c; d < 3; ++d) {
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < 6; ++i) s += hpl[3 * i + c] * V[3 * i + d];
                M[k++] = s;
            }
    }
    group_sum(M, lg);
    if (gj == 0 && lmok) {
        const int l = a.lm_perm[ri];
        if (l >= 0) {
            const double cl[6] = {rec[LH_REC_L], rec[LH_REC_L + 1], rec[LH_REC_L + 2],
                                  rec[LH_REC_L + 3], rec[LH_REC_L + 4], rec[LH_REC_L + 5]};
            double out[9];
            lh_cov_lm_finish(cl, M, out);
            const bool deg = !(cl[0] == cl[0]);   // the record's marker of a rank-deficient H_ll (k_lin)
            double* dst = a.lm_cov + 9 * (size_t)l;
#pragma unroll
            for (int i = 0; i < 9; ++i) dst[i] = deg ? __builtin_nan("") : out[i];
        }
    }
}

extern "C" {

hipError_t lh_launch_cov_snapshot(hipStream_t st, const lh_cov_snap_args* a) {
    const int n = a->npt > 3 * a->nrec ? a->npt : 3 * a->nrec;
    const int blocks = n < 256 ? 1 : (n / 256 < 1024 ? n / 256 : 1024);
    hipLaunchKernelGGL(k_cov_snapshot, dim3(blocks), dim3(256), 0, st, *a);
    return hipGetLastError();
}

// Sigma_pp of the free rows: the factor, W = L^-1, W^T W (a->ns = ceil16(n_free) > 0, at most LH_COV_NSMAX)
hipError_t lh_launch_cov_pose(hipStream_t st, const lh_cov_args* a) {
    if (a->ns <= 0 || a->ns > LH_COV_NSMAX || a->ns % CNB != 0 || 6 * a->P > LH_COV_NSMAX) return hipErrorInvalidValue;
    const int nb = a->ns / CNB;
    hipLaunchKernelGGL(k_cov_factor, dim3(1), dim3(CFT), 0, st, *a);
    hipLaunchKernelGGL(k_cov_linv, dim3(nb), dim3(256), 0, st, *a);
    hipLaunchKernelGGL(k_cov_gram, dim3(nb * (nb + 1) / 2), dim3(256), 0, st, *a);
    return hipGetLastError();
}

hipError_t lh_launch_cov_lm(hipStream_t st, const lh_cov_lm_args* a, lh_params prm) {
    if (a->n_sb <= 0) return hipSuccess;
    const dim3 g((a->n_sb + LH_WAVES - 1) / LH_WAVES);
    if (prm.precision == 1) hipLaunchKernelGGL(k_cov_lm<true>, g, dim3(256), 0, st, *a, prm);
    else hipLaunchKernelGGL(k_cov_lm<false>, g, dim3(256), 0, st, *a, prm);
    return hipGetLastError();
}

}  // extern "C"
