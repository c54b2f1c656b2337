// lh_ldlt.h — the reduced system's solves in one workgroup's LDS (k_ctrl, k_ctrl_b and the LDL^T probe; the
// micro-benchmark tools/ubench_ctrl_chain.hip): the layout, the 8x8 block factor, the blocked LDL^T's tile work for
// an LdsSys (here) or a BandSys (lh_ctrl_b.hip), the back substitution, and the three solves lds_ldlt_solve,
// lds_ldlt_solve_nd and lds_pcg_solve.
#pragma once
#include "lh_common.h"
#include "lh_dev.h"

#pragma clang fp contract(fast)

constexpr int CT = 1024;      // threads of a workgroup that runs these solves (k_ctrl, k_ctrl_b, k_ctrl_p): 16 waves
constexpr int NP = LH_NPAD;   // padded system size; row NP of A holds the right-hand side
constexpr int AS = LH_NPAD + 2;   // LDS row stride, = 2 mod 32 doubles: a 16x4 tile fragment (lane (i, k) at row i,
                              // column k) hits 32 distinct 8-byte bank pairs per half-wave (ds_read_b64 banks
                              // (a/4) mod 64 over lanes 0-31 / 32-63); the odd stride 129 put rows i and i + 1 at
                              // columns k + 1 and k on one pair (two-way conflicts on every tile read)
constexpr int NBLK = LH_NPAD / 8;

// Per-block products of the 8x8 diagonal-block factor (LDS, shared by all waves).
struct LdltBlockLds {
    double N[4][64];          // N = (Delta L^T)^-1 of the block being eliminated (row-major), by step parity
                              // (the two-chain schedule: chain c uses N[2c + parity])
    double ND[NBLK][64];      // N Delta = L_bb^-T of every block (row-major): trailing-update operand
                              // and the back substitution's block solve
    double z[NP];             // z = D^-1 L^-1 b (zero where |D| <= DBL_MIN)
};
// one instance per kernel, whichever schedule runs
__device__ __forceinline__ LdltBlockLds& ldlt_lds() {
    __shared__ __attribute__((aligned(16))) LdltBlockLds F;
    return F;
}

// 64-bit broadcast of lane L of each 16-lane row: one v_mov_b64_dpp row_newbcast (gfx950 allows 64-bit DPP
// for row_newbcast).  The factor and the back substitution are issue-bound chains of these (a lone wave
// issues a dependent f64 op every ~7-10 cycles), so one move instead of two 32-bit halves is what counts.
template <int L>
__device__ __forceinline__ double bcast16(double v) {
    const long long x = __builtin_amdgcn_update_dpp((long long)0, __double_as_longlong(v), 0x150 + L, 0xf, 0xf, true);
    return __longlong_as_double(x);
}

// Column Q of the 8x8 factor: the pivot from lane Q by broadcast, its reciprocal (v_rcp_f64 and two
// Newton steps), the column's entries and the trailing updates of the lane's row.  (A cubic correction
// folded into the quotient, three dependent FMAs instead of five, measured the same ~1.8k cycles per
// block alone, tools/ubench_ctrl_chain.hip: the chain is bound by issue, not by this latency.)
// SAFE: Eigen ldlt_inplace's zero-pivot rule (no scaling where !pivot_is_valid: Delta = 1) on the chain;
// the fast form takes every pivot as valid and factor_block8_v redoes the block in the safe form when one
// was not (a fixed pose under STRATEGY1), so valid blocks get the same bits with three fewer dependent
// instructions per column.
template <int Q, bool SAFE>
__device__ __forceinline__ void factor_column(double (&R)[8], double (&dl)[8]) {
    const double d = bcast16<Q>(R[Q]);
    dl[Q] = SAFE ? (fabs(d) > 0.0 ? d : 1.0) : d;
    const double inv = fast_rcp(dl[Q]);
    const double coef = R[Q] * inv;
    double u[8];
    // W[j][Q] = lane j's R[Q], read before R[Q] becomes coef
    if (Q < 1) u[1] = bcast16<1>(R[Q]);
    if (Q < 2) u[2] = bcast16<2>(R[Q]);
    if (Q < 3) u[3] = bcast16<3>(R[Q]);
    if (Q < 4) u[4] = bcast16<4>(R[Q]);
    if (Q < 5) u[5] = bcast16<5>(R[Q]);
    if (Q < 6) u[6] = bcast16<6>(R[Q]);
    if (Q < 7) u[7] = bcast16<7>(R[Q]);
#pragma unroll
    for (int j = Q + 1; j < 8; ++j) R[j] -= coef * u[j];
    R[Q] = coef;
}

// Where the blocked LDL^T keeps its operands (the same code serves both controllers):
//  LdsSys  (k_ctrl, n <= LH_NPAD): the whole system in LDS, row stride AS, the rhs as row NP, L^T in
//          the upper triangle (L[r][c] at A[c][r]) for the back substitution;
//  BandSys (k_ctrl_b, banded windows past LH_PMAX poses): a 128-row circular window of the lower band in LDS,
//          L rows to global memory; lh_ctrl_b.hip.
struct LdsSys {
    // the trailing stores rewrite the entries outside the update with their own value (one exec mask
    // for the four stores; k_ctrl 28.09 / 28.04 -> 27.46 / 27.54 us); in k_ctrl_b's busier LDS (the
    // stream loaders' writes) the extra stores measured slower, so BandSys keeps the per-entry masks
    static constexpr bool rewrite_masked = true;
    double* A;
    __device__ __forceinline__ double& at(int r, int c) const { return A[r * AS + c]; }
    __device__ __forceinline__ double& rhs(int r) const { return A[NP * AS + r]; }
    __device__ __forceinline__ void store_l(int r, int c, double v) const { A[c * AS + r] = v; }
    // indices as stored: a 16-row tile row or 8-column block starts at a multiple of 8, so wrapping its
    // base once wraps every row / column of it (no carry into the base)
    __device__ __forceinline__ int wrap(int x) const { return x; }
    __device__ __forceinline__ double& atw(int r, int c) const { return A[r * AS + c]; }
};

// LDL^T of the 8x8 diagonal block at (k0, k0) of A by one wave, Eigen ldlt_inplace order (L = W
// where pivot_is_valid fails).  In each 16-lane row (four identical replicas), lane r < 8 holds
// row r of the block and lane 8 + r row r of the identity: the same column eliminations turn
// the first into L and the second into N = (Delta L^T)^-1, Delta = diag(D, 1 where invalid), so
// one instruction stream computes both.  Column q's pivot and entries move by DPP broadcast.
// Writes D on A's diagonal and L^T above it (L[r][c] at A[c][r]), N, and ND = N Delta = L^-T.
// For a row a below the block, l = a N is its forward substitution through the block and
// l Delta its partially eliminated entries, so the trailing update of rows i, j is
// L_i Delta L_j^T = T_i a_j^T with T_i = L_i ND^T.
// v: row r = lane & 7 of the block (entries past the diagonal unused)
template <class S>
__device__ __forceinline__ void factor_block8_v(const S& A, const double (&v)[8], double* __restrict__ No,
                                                double* __restrict__ NDo, int k0, int lane) {
    const int p = lane & 15, r = p & 7;
    const bool ident = p >= 8;
    double R[8], dl[8];
    const int kw = A.wrap(k0);
#pragma unroll
    for (int q = 0; q < 8; ++q) R[q] = ident ? (q == r ? 1.0 : 0.0) : v[q];
    factor_column<0, false>(R, dl);
    factor_column<1, false>(R, dl);
    factor_column<2, false>(R, dl);
    factor_column<3, false>(R, dl);
    factor_column<4, false>(R, dl);
    factor_column<5, false>(R, dl);
    factor_column<6, false>(R, dl);
    factor_column<7, false>(R, dl);
    bool ok = true;   // every pivot valid (the pivots are the same in every lane)
#pragma unroll
    for (int q = 0; q < 8; ++q) ok = ok && fabs(dl[q]) > 0.0;
    if (!__builtin_amdgcn_readfirstlane(ok)) {   // rare: redo the block with the zero-pivot rule
#pragma unroll
        for (int q = 0; q < 8; ++q) R[q] = ident ? (q == r ? 1.0 : 0.0) : v[q];
        factor_column<0, true>(R, dl);
        factor_column<1, true>(R, dl);
        factor_column<2, true>(R, dl);
        factor_column<3, true>(R, dl);
        factor_column<4, true>(R, dl);
        factor_column<5, true>(R, dl);
        factor_column<6, true>(R, dl);
        factor_column<7, true>(R, dl);
    }
    if (lane < 8) {
        if constexpr (S::rewrite_masked) {
            // no branch per store: the entries below the diagonal go to the row's padding column
            // (LH_NPAD, never read)
#pragma unroll
            for (int q = 0; q < 8; ++q) A.atw(kw + q, q <= r ? kw + r : LH_NPAD) = (q == r) ? dl[q] : R[q];
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q <= r) A.atw(kw + q, kw + r) = (q == r) ? dl[q] : R[q];
        }
    } else if (lane < 16) {
        double2* n2 = reinterpret_cast<double2*>(No + 8 * r);
        double2* d2 = reinterpret_cast<double2*>(NDo + 8 * r);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            n2[q] = double2{R[2 * q], R[2 * q + 1]};
            d2[q] = double2{R[2 * q] * dl[2 * q], R[2 * q + 1] * dl[2 * q + 1]};
        }
    }
}
template <class S>
__device__ __forceinline__ void factor_block8(const S& A, double* __restrict__ No, double* __restrict__ NDo, int k0,
                                              int lane) {
    const int r = lane & 7, kw = A.wrap(k0);
    double v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = A.atw(kw + r, kw + q);   // upper entries: garbage confined to this lane's upper part
    factor_block8_v(A, v, No, NDo, k0, lane);
}

// Step k0 of the elimination for the 16-row tile row at rb (one wave): with the raw block column
// a_I = A[rb..rb+15][k0..k0+7] (rows below k0+8 only; the block's own rows are masked),
//   L_I^T = N^T a_I^T              (MFMA; lands in A-operand layout: lane (li, lk) holds L[li][lk], L[li][lk+4])
//   T_I^T = ND L_I^T               (T_I = L_I Delta N^T, again in A-operand layout)
//   L^T -> A[k0+c][i]              (upper triangle; only when store_l)
//   b_i -= T_I . b_blk             (forward substitution of the rhs row; only when store_l)
//   A_IJ -= T_I a_J^T  for the tile columns J in [jb0, jb1) except skip_cb (lower part, cols >= m0).
// Every operand is the block column as it was before this step: no panel pass and no barrier
// between the elimination of the column and the trailing update.
template <class S>
__device__ __forceinline__ void ldlt_tile_row(const S& A, const double* __restrict__ N, const double* __restrict__ ND,
                                              int k0, int rb, int jb0, int jb1, int skip_cb, bool store_l, int lane) {
    const int li = lane & 15, lk = lane >> 4, m0 = k0 + 8;
    const int rbw = A.wrap(rb), kw = A.wrap(k0);
    const bool lo = li < 8;
    // every LDS read of this tile row is issued up front (tiles are disjoint and this step's
    // writes never touch block column k0, so no read here can see a write of this step)
    // (unconditional reads, selected after: no exec-masked branches between the loads)
    const double n0 = N[lk * 8 + (li & 7)], n1 = N[(lk + 4) * 8 + (li & 7)];
    const double d0 = ND[(li & 7) * 8 + lk], d1 = ND[(li & 7) * 8 + 4 + lk];
    const double a0 = A.atw(rbw + li, kw + lk), a1 = A.atw(rbw + li, kw + 4 + lk);
    const double na0 = lo ? n0 : 0.0, na1 = lo ? n1 : 0.0, da0 = lo ? d0 : 0.0, da1 = lo ? d1 : 0.0;
    int cb = (jb0 == skip_cb) ? jb0 + 16 : jb0;
    double b0 = 0.0, b1 = 0.0, old[4] = {0.0, 0.0, 0.0, 0.0};
    if (cb < jb1) {
        const int cbw = A.wrap(cb);
        b0 = A.atw(cbw + li, kw + lk);
        b1 = A.atw(cbw + li, kw + 4 + lk);
#pragma unroll
        for (int q = 0; q < 4; ++q) old[q] = A.atw(rbw + li, cbw + lk + 4 * q);
    }
    __builtin_amdgcn_sched_barrier(0);   // every load above is in flight before the first wait
    v4d l = {0.0, 0.0, 0.0, 0.0};
    l = __builtin_amdgcn_mfma_f64_16x16x4f64(na0, a0, l, 0, 0, 0);
    l = __builtin_amdgcn_mfma_f64_16x16x4f64(na1, a1, l, 0, 0, 0);
    // l[q] = L[rb+li][k0+lk+4q] (q = 0, 1)
    v4d t = {0.0, 0.0, 0.0, 0.0};
    t = __builtin_amdgcn_mfma_f64_16x16x4f64(da0, l[0], t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f64_16x16x4f64(da1, l[1], t, 0, 0, 0);
    // t[q] = T[rb+li][lk+4q] (q = 0, 1)
    if (store_l) {
        const double rb0 = (li == 0) ? A.rhs(k0 + lk) : 0.0, rb1 = (li == 0) ? A.rhs(k0 + 4 + lk) : 0.0;
        double rold[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) rold[q] = A.rhs(rb + lk + 4 * q);
        if (rb + li >= m0) {
            A.store_l(rb + li, k0 + lk, l[0]);
            A.store_l(rb + li, k0 + 4 + lk, l[1]);
        }
        v4d u = {0.0, 0.0, 0.0, 0.0};
        u = __builtin_amdgcn_mfma_f64_16x16x4f64(t[0], rb0, u, 0, 0, 0);
        u = __builtin_amdgcn_mfma_f64_16x16x4f64(t[1], rb1, u, 0, 0, 0);
        // u[q] = (T b_blk)[rb+lk+4q] in column li = 0
        if (li == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = rb + lk + 4 * q;
                if (row >= m0) A.rhs(row) = rold[q] - u[q];
            }
        }
    }
    // trailing tiles, software-pipelined: the next tile's operands are in flight during this one's MFMAs
    while (cb < jb1) {
        const int cbw_cur = A.wrap(cb);
        int nc = cb + 16;
        if (nc == skip_cb) nc += 16;
        double nb0 = 0.0, nb1 = 0.0, nold[4] = {0.0, 0.0, 0.0, 0.0};
        if (nc < jb1) {
            const int ncw = A.wrap(nc);
            nb0 = A.atw(ncw + li, kw + lk);
            nb1 = A.atw(ncw + li, kw + 4 + lk);
#pragma unroll
            for (int q = 0; q < 4; ++q) nold[q] = A.atw(rbw + li, ncw + lk + 4 * q);
        }
        // the update transposed, (a_J T_I^T)^T: lane (li, lk) gets row li, columns lk + 4q of the tile, the
        // same fragment shape as the operand reads (conflict-free at this stride); the products are the
        // same, so are the bits
        v4d acc = {0.0, 0.0, 0.0, 0.0};
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(b0, t[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(b1, t[1], acc, 0, 0, 0);
        const int row = rb + li;
        // entries outside the update (left of m0, above the diagonal) get their own value back: no other
        // wave writes them this step, and the four stores share one exec mask instead of four branches
        if constexpr (S::rewrite_masked) {
            if (row >= m0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int col = cb + lk + 4 * q;
                    A.atw(rbw + li, cbw_cur + lk + 4 * q) = (col >= m0 && col <= row) ? old[q] - acc[q] : old[q];
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int col = cb + lk + 4 * q;
                if (row >= m0 && col >= m0 && col <= row) A.atw(rbw + li, cbw_cur + lk + 4 * q) = old[q] - acc[q];
            }
        }
        cb = nc;
        b0 = nb0; b1 = nb1;
#pragma unroll
        for (int q = 0; q < 4; ++q) old[q] = nold[q];
    }
}

// Wave 0's share of step k0: the trailing update of the diagonal tile at rb (the one holding block
// k0 + 8), the head of every step's critical chain (this, then the next block's factor).  The
// operands are ldlt_tile_row's with a_J = a_I (the tile is its own column), so the eight LDS reads go
// out in one batch, unconditionally (N / ND rows past 7 read the neighbouring in-bounds LDS and are
// dropped by the select), and the only waits are the one round trip and the MFMA chain.
template <class S>
__device__ __forceinline__ void diag_tile(const S& A, const double* __restrict__ N, const double* __restrict__ ND,
                                          int k0, int rb, int lane) {
    const int li = lane & 15, lk = lane >> 4, m0 = k0 + 8;
    const int rbw = A.wrap(rb), kw = A.wrap(k0);
    const bool lo = li < 8;
    const double n0 = N[lk * 8 + (li & 7)], n1 = N[(lk + 4) * 8 + (li & 7)];
    const double d0 = ND[(li & 7) * 8 + lk], d1 = ND[(li & 7) * 8 + 4 + lk];
    const double a0 = A.atw(rbw + li, kw + lk), a1 = A.atw(rbw + li, kw + 4 + lk);
    double old[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) old[q] = A.atw(rbw + li, rbw + lk + 4 * q);
    __builtin_amdgcn_sched_barrier(0);   // the scheduler otherwise sinks the loads between the MFMAs
    v4d l = {0.0, 0.0, 0.0, 0.0};
    l = __builtin_amdgcn_mfma_f64_16x16x4f64(lo ? n0 : 0.0, a0, l, 0, 0, 0);
    l = __builtin_amdgcn_mfma_f64_16x16x4f64(lo ? n1 : 0.0, a1, l, 0, 0, 0);
    v4d t = {0.0, 0.0, 0.0, 0.0};
    t = __builtin_amdgcn_mfma_f64_16x16x4f64(lo ? d0 : 0.0, l[0], t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f64_16x16x4f64(lo ? d1 : 0.0, l[1], t, 0, 0, 0);
    v4d acc = {0.0, 0.0, 0.0, 0.0};   // transposed, as in ldlt_tile_row
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, t[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, t[1], acc, 0, 0, 0);
    const int row = rb + li;
    // as ldlt_tile_row: the entries outside the update are rewritten with their own value (above the
    // diagonal this wave's factor writes L^T next; rows above m0 are the store unit's, left alone)
    if constexpr (S::rewrite_masked) {
        if (row >= m0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int col = rb + lk + 4 * q;
                A.atw(rbw + li, rbw + lk + 4 * q) = (col >= m0 && col <= row) ? old[q] - acc[q] : old[q];
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = rb + lk + 4 * q;
            if (row >= m0 && col >= m0 && col <= row) A.atw(rbw + li, rbw + lk + 4 * q) = old[q] - acc[q];
        }
    }
}

// k_ctrl's two-chain steps (lh_ctrl_nd_plan): one tile row's unit applying up to two sources, the blocks
// the two chains eliminate this step.  For each source s in smask | stmask: L_s = a_s N_s, T_s = L_s ND_s^T
// with the rows above its block (< m0_s) zeroed, so they contribute nothing; stmask: L_s^T stored for the
// tile row and the rhs row updated by every stored source at once (two units never update one rhs row
// in a step); then A_IJ -= sum_{s in smask} T_s a_{s,J}^T over the tiles [jb0, jb1), a_{s,J}'s rows above
// the block zeroed likewise.  Entries above every applied source's block are left alone.
struct NdSrc {
    const double* N;
    const double* ND;
    int k0;
};
__device__ __forceinline__ void nd_tile_row(double* __restrict__ A, const NdSrc (&src)[2], int smask, int stmask, int rb,
                                            int jb0, int jb1, int lane) {
    const int li = lane & 15, lk = lane >> 4;
    const bool lo = li < 8;
    double t0[2], t1[2];
    int mm = 1 << 20;
    double ru[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        t0[q] = 0.0; t1[q] = 0.0;
        if (!(((smask | stmask) >> q) & 1)) continue;   // a stored source need not reach the unit's tiles
        const int k0 = src[q].k0, m0 = k0 + 8;
        mm = min(mm, m0);
        const double* N = src[q].N;
        const double* ND = src[q].ND;
        const double na0 = lo ? N[lk * 8 + li] : 0.0, na1 = lo ? N[(lk + 4) * 8 + li] : 0.0;
        const double da0 = lo ? ND[li * 8 + lk] : 0.0, da1 = lo ? ND[li * 8 + 4 + lk] : 0.0;
        const double a0 = A[(rb + li) * AS + k0 + lk], a1 = A[(rb + li) * AS + k0 + 4 + lk];
        v4d l = {0.0, 0.0, 0.0, 0.0};
        l = __builtin_amdgcn_mfma_f64_16x16x4f64(na0, a0, l, 0, 0, 0);
        l = __builtin_amdgcn_mfma_f64_16x16x4f64(na1, a1, l, 0, 0, 0);
        v4d t = {0.0, 0.0, 0.0, 0.0};
        t = __builtin_amdgcn_mfma_f64_16x16x4f64(da0, l[0], t, 0, 0, 0);
        t = __builtin_amdgcn_mfma_f64_16x16x4f64(da1, l[1], t, 0, 0, 0);
        const bool below = rb + li >= m0;
        t0[q] = below ? t[0] : 0.0;
        t1[q] = below ? t[1] : 0.0;
        if ((stmask >> q) & 1) {
            if (below) {
                A[(k0 + lk) * AS + rb + li] = l[0];
                A[(k0 + 4 + lk) * AS + rb + li] = l[1];
            }
            const double rb0 = (li == 0) ? A[NP * AS + k0 + lk] : 0.0, rb1 = (li == 0) ? A[NP * AS + k0 + 4 + lk] : 0.0;
            v4d u = {0.0, 0.0, 0.0, 0.0};
            u = __builtin_amdgcn_mfma_f64_16x16x4f64(t0[q], rb0, u, 0, 0, 0);
            u = __builtin_amdgcn_mfma_f64_16x16x4f64(t1[q], rb1, u, 0, 0, 0);
#pragma unroll
            for (int w = 0; w < 4; ++w) ru[w] += u[w];
        }
    }
    if (stmask && li == 0) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int row = rb + lk + 4 * w;
            if (row >= mm) A[NP * AS + row] -= ru[w];
        }
    }
    for (int cb = jb0; cb < jb1; cb += 16) {
        double old[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) old[w] = A[(rb + li) * AS + cb + lk + 4 * w];
        v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (!((smask >> q) & 1)) continue;
            const int k0 = src[q].k0, m0 = k0 + 8;
            const bool cin = cb + li >= m0;
            const double b0 = cin ? A[(cb + li) * AS + k0 + lk] : 0.0, b1 = cin ? A[(cb + li) * AS + k0 + 4 + lk] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(b0, t0[q], acc, 0, 0, 0);   // transposed
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(b1, t1[q], acc, 0, 0, 0);
        }
        const int row = rb + li;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int col = cb + lk + 4 * w;
            if (row >= mm && col >= mm && col <= row) A[row * AS + col] = old[w] - acc[w];
        }
    }
}

// Back substitution x = L^-T z for block KB (compile-time, so every lane index below is an
// immediate), one wave: y holds rows lane (y0) and lane + 64 (y1), already reduced by every block
// above KB.  x_b = ND_b y_b: the block's 8 y values sit in lanes KB..KB+7 (mod 64), inside one
// 16-lane row, and reach that row's lanes by DPP broadcast; lane KB+v computes x_b[v], so it
// holds its own row's result.  Every row r above the block then takes y_r -= sum_v L[KB+v][r]
// x_b[v] (L^T row r in the upper triangle), x_b broadcast by readlane.  No LDS writes: the
// compiler may hoist every block's operand loads.
// The LDS operands of the back substitution never change while it runs, so no load waits for the
// chain: the caller loads block b-1's ND_b row while block b computes, and each block issues its L^T
// loads before its first DPP broadcast (all unconditional: a block past nb reads in-bounds padding it
// never uses).  Loading them after the runtime nb guard put two dependent LDS round trips on the
// chain per block: the compiler does not hoist loads across those branches.
template <int KB>
__device__ __forceinline__ void backsub_load_nd(const LdltBlockLds& F, int lane, double (&nd)[8]) {
#pragma unroll
    for (int w = 0; w < 8; ++w) nd[w] = F.ND[KB >> 3][(lane & 7) * 8 + w];
}

// Back substitution x = L^-T z for block KB (compile-time, so every lane index below is an
// immediate), one wave: y holds rows lane (y0) and lane + 64 (y1), already reduced by every block
// above KB.  x_b = ND_b y_b: the block's 8 y values sit in lanes KB..KB+7 (mod 64), inside one
// 16-lane row, and reach that row's lanes by DPP broadcast; lane KB+v computes x_b[v], so it
// holds its own row's result.  Every row r above the block then takes y_r -= sum_v L[KB+v][r]
// x_b[v] (L^T row r in the upper triangle), x_b broadcast by readlane.
template <int KB>
__device__ __forceinline__ void backsub_block(const double* __restrict__ A, const double (&nd)[8], int nb, int lane,
                                              double& y0, double& y1) {
    constexpr bool HI = KB >= 64;
    constexpr int KL = KB & 63, R16 = KL & 15;
    double l0[8], l1[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) l0[v] = A[lane * AS + KB + v];
    if (HI) {
#pragma unroll
        for (int v = 0; v < 8; ++v) l1[v] = A[(lane + 64) * AS + KB + v];
    }
    // the loads stay ahead of the broadcasts (left alone, the scheduler sinks them past the nb branch to
    // their first use, after x_b, and the LDS round trip lands on the chain)
    __builtin_amdgcn_sched_barrier(0);
    if (KB >= nb) return;
    const double ys = HI ? y1 : y0;
    double yb[8];
    yb[0] = bcast16<R16 + 0>(ys); yb[1] = bcast16<R16 + 1>(ys); yb[2] = bcast16<R16 + 2>(ys); yb[3] = bcast16<R16 + 3>(ys);
    yb[4] = bcast16<R16 + 4>(ys); yb[5] = bcast16<R16 + 5>(ys); yb[6] = bcast16<R16 + 6>(ys); yb[7] = bcast16<R16 + 7>(ys);
    const double xv = ((nd[0] * yb[0] + nd[1] * yb[1]) + (nd[2] * yb[2] + nd[3] * yb[3])) +
                      ((nd[4] * yb[4] + nd[5] * yb[5]) + (nd[6] * yb[6] + nd[7] * yb[7]));
    double xb[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) xb[v] = readlane_d(xv, KL + v);
    const double s0 = ((l0[0] * xb[0] + l0[1] * xb[1]) + (l0[2] * xb[2] + l0[3] * xb[3])) +
                      ((l0[4] * xb[4] + l0[5] * xb[5]) + (l0[6] * xb[6] + l0[7] * xb[7]));
    if (HI) {
        const double s1 = ((l1[0] * xb[0] + l1[1] * xb[1]) + (l1[2] * xb[2] + l1[3] * xb[3])) +
                          ((l1[4] * xb[4] + l1[5] * xb[5]) + (l1[6] * xb[6] + l1[7] * xb[7]));
        y0 -= s0;
        y1 = (lane + 64 < KB) ? y1 - s1 : ((lane + 64 < KB + 8) ? xv : y1);
    } else {
        y0 = (lane < KB) ? y0 - s0 : ((lane < KB + 8) ? xv : y0);
    }
}

// Phase 4 of both LDL^T schedules: x = L^-T z over every block, descending, one wave (y0 / y1: rows
// lane / lane + 64 of z in, of x out, in the factor's order).
__device__ __forceinline__ void ldlt_backsub(const double* __restrict__ A, const LdltBlockLds& F, int nb, int lane,
                                             double& y0, double& y1) {
    double nda[8], ndb[8];
    backsub_load_nd<120>(F, lane, nda);
    backsub_load_nd<112>(F, lane, ndb);
    backsub_block<120>(A, nda, nb, lane, y0, y1);
    backsub_load_nd<104>(F, lane, nda);
    backsub_block<112>(A, ndb, nb, lane, y0, y1);
    backsub_load_nd<96>(F, lane, ndb);
    backsub_block<104>(A, nda, nb, lane, y0, y1);
    backsub_load_nd<88>(F, lane, nda);
    backsub_block<96>(A, ndb, nb, lane, y0, y1);
    backsub_load_nd<80>(F, lane, ndb);
    backsub_block<88>(A, nda, nb, lane, y0, y1);
    backsub_load_nd<72>(F, lane, nda);
    backsub_block<80>(A, ndb, nb, lane, y0, y1);
    backsub_load_nd<64>(F, lane, ndb);
    backsub_block<72>(A, nda, nb, lane, y0, y1);
    backsub_load_nd<56>(F, lane, nda);
    backsub_block<64>(A, ndb, nb, lane, y0, y1);
    backsub_load_nd<48>(F, lane, ndb);
    backsub_block<56>(A, nda, nb, lane, y0, y1);
    backsub_load_nd<40>(F, lane, nda);
    backsub_block<48>(A, ndb, nb, lane, y0, y1);
    backsub_load_nd<32>(F, lane, ndb);
    backsub_block<40>(A, nda, nb, lane, y0, y1);
    backsub_load_nd<24>(F, lane, nda);
    backsub_block<32>(A, ndb, nb, lane, y0, y1);
    backsub_load_nd<16>(F, lane, ndb);
    backsub_block<24>(A, nda, nb, lane, y0, y1);
    backsub_load_nd<8>(F, lane, nda);
    backsub_block<16>(A, ndb, nb, lane, y0, y1);
    backsub_load_nd<0>(F, lane, ndb);
    backsub_block<8>(A, nda, nb, lane, y0, y1);
    backsub_block<0>(A, ndb, nb, lane, y0, y1);
}

// The controller's step tail taken by the back-substitution wave from its registers (k_ctrl, LDL^T): the
// pose part of the gain denominator (isGoodStepInLM's scale, problem.cpp:528-533) summed over the wave
// (rows lane and lane + 64 of one lane first), the step stored for k_lin.  ctrl null: no tail (the probe).
struct LdltTail {
    lh_ctrl* ctrl;
    double* dxp;
    const double* bpv;
    const double* hdv;
    double lambda;
    int strategy;
    int rung;   // the lambda-ladder rung this controller workgroup solves (lh_ctrl.spose_l)
};
__device__ __forceinline__ void ldlt_tail(const LdltTail& tl, int n, int lane, double y0, double y1) {
    auto term = [&](int r, double d) {
        if (r >= n) return 0.0;
        if (tl.dxp) tl.dxp[r] = d;
        const double b = tl.bpv[r];
        return (tl.strategy == 0) ? d * (tl.lambda * d + b) : d * (tl.lambda * tl.hdv[r] * d + b);
    };
    double sp[1] = {term(lane, y0) + term(lane + 64, y1)};
    group_sum(sp, 6);
    if (lane == 0) tl.ctrl->spose_l[tl.rung] = sp[0];
}

// Phases 3-4 of k_ctrl on a padded system already in LDS (A lower + rhs row NP, zeros in the upper
// triangle): blocked LDL^T with the forward substitution, then the back substitution; xsol[perm[r]] =
// the solution's entry r < n (perm == nullptr: xsol[r]).  units: the per-step work units in LDS
// (lh_ctrl_units: the envelope of S decides which tile rows a step touches).  Shared with the
// k_ldlt_probe test hook.  Must be called by all CT threads.
//
// Step t eliminates block column k0 = 8t.  Interval t (one barrier each):
//   wave 0:       the trailing update of the diagonal tile holding block t+1 (when its envelope
//                 reaches block t), then the factor of block t+1 (N by step parity, ND per block);
//   waves 1-15:   their unit of step t: L_I (stored transposed), T_I, the rhs update and
//                 A_IJ -= T_I a_J^T over the unit's tile columns;
//   wave 12 first: z_t = b_t N_t (Eigen's solve tolerance applied).
// L lives in the upper triangle, so the raw block columns stay readable for the whole step.
__device__ __forceinline__ void lds_ldlt_solve(double* __restrict__ A, double* __restrict__ xsol, int n, int NE, int tid,
                                               const int* __restrict__ perm, const uint16_t* __restrict__ units,
                                               const LdltTail& tl = LdltTail{}, bool factored0 = false) {
    const int lane = tid & 63, wave = tid >> 6;
    LdltBlockLds& F = ldlt_lds();
    const int nb = (n + 7) & ~7;          // blocks past the last real row are identity: never eliminated
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const LdsSys SY{A};
    // this wave's unit words, lane t holding step t's: read once, so no step starts with an LDS round trip
    const uint32_t uwv = (lane < LH_NSTEP) ? units[wv * LH_NSTEP + lane] : 0u;
    if (!factored0) {   // (k_ctrl factors block 0 during its scatter)
        if (wv == 0) factor_block8(SY, F.N[0], F.ND[0], 0, lane);
        lds_barrier();
    }
    CSTAMP(5);
#ifdef LH_STAMPS
    // per-step split (diagnostic): wave 0's diagonal tile, its factor and its wait at the barrier;
    // the other waves' unit time and barrier wait (wave-cycles summed over waves)
    unsigned long long ss_[5] = {0, 0, 0, 0, 0}, sa_ = __builtin_amdgcn_s_memtime(), sb_;
    // per step t: [64 + t] wave 0's diagonal tile, [80 + t] its factor, [96 + t] its barrier wait
    // (sums over launches), [112 + t] the slowest other wave's unit in the worst launch (atomicMax of
    // cycles << 24 | unit word << 4 | wave)
    uint32_t su_ = 0;
#define LDLT_SSTAMP(i) do { __builtin_amdgcn_sched_barrier(0); sb_ = __builtin_amdgcn_s_memtime(); \
        ss_[i] += sb_ - sa_; \
        if (lane == 0 && (i) != 4) { \
            const int ti_ = min(k0 >> 3, 15); \
            if ((i) == 3) atomicMax(&lh_stamps[112 + ti_], ((sb_ - sa_) << 24) | ((unsigned long long)(su_ & 0xffffu) << 4) | (unsigned)wv); \
            else atomicAdd(&lh_stamps[64 + 16 * ((i) == 0 ? 0 : (i) == 1 ? 1 : 2) + ti_], sb_ - sa_); } \
        sa_ = sb_; __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define LDLT_SSTAMP(i)
#endif
    for (int k0 = 0; k0 < nb; k0 += 8) {
        const int t = k0 >> 3, par = t & 1, m0 = k0 + 8;
        const double* N = F.N[par];
        const double* ND = F.ND[t];
        if (wv == 12 && lane < 8) {       // z_t = b_t N_t, zeroed where |D| <= DBL_MIN (LDLT::_solve_impl)
            double z = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) z += A[NP * AS + k0 + q] * N[q * 8 + lane];
            const double d = A[(k0 + lane) * AS + k0 + lane];
            F.z[k0 + lane] = fabs(d) > 2.2250738585072014e-308 ? z : 0.0;
        }
        if (m0 < nb) {
            const int g0 = m0 >> 4;               // tile row/col of the next diagonal block
            const uint32_t uw = __builtin_amdgcn_readlane(uwv, t);
#ifdef LH_STAMPS
            su_ = uw;
#endif
            if (wv == 0) {
                if (uw & LH_UNIT_VALID) {
                    diag_tile(SY, N, ND, k0, 16 * g0, lane);
                    wave_sync();
                }
                LDLT_SSTAMP(0);
                factor_block8(SY, F.N[par ^ 1], F.ND[t + 1], m0, lane);
                LDLT_SSTAMP(1);
            } else if (uw & LH_UNIT_VALID) {
                const int I = g0 + (uw & 7), jb0 = g0 + ((uw >> 3) & 7), jb1 = g0 + ((uw >> 6) & 15);
                ldlt_tile_row(SY, N, ND, k0, 16 * I, 16 * jb0, 16 * jb1, -1, (uw & LH_UNIT_STORE) != 0, lane);
            }
            if (wv != 0) LDLT_SSTAMP(3);
        }
        lds_barrier();
        if (wv == 0) LDLT_SSTAMP(2); else LDLT_SSTAMP(4);
    }
#ifdef LH_STAMPS
    if (lane == 0) {
        if (wv == 0) {
            atomicAdd(&lh_stamps[46], ss_[0]);
            atomicAdd(&lh_stamps[47], ss_[1]);
            atomicAdd(&lh_stamps[48], ss_[2]);
            atomicAdd(&lh_stamps[51], 1ull);
        } else {
            atomicAdd(&lh_stamps[49], ss_[3]);
            atomicAdd(&lh_stamps[50], ss_[4]);
        }
    }
#endif
    CSTAMP(6);

    // ---------------- 4. back substitution x = L^-T z, blocks descending, one wave ----------------
    if (wv == 0) {
        double y0 = (lane < nb) ? F.z[lane] : 0.0, y1 = (lane + 64 < nb) ? F.z[lane + 64] : 0.0;
        ldlt_backsub(A, F, nb, lane, y0, y1);
        if (perm) {
            if (lane < n) xsol[perm[lane]] = y0;
            if (lane + 64 < n) xsol[perm[lane + 64]] = y1;
        } else {
            if (lane < NE) xsol[lane] = y0;
            if (lane + 64 < NE) xsol[lane + 64] = y1;
        }
        if (tl.ctrl) ldlt_tail(tl, n, lane, y0, y1);
    }
    lds_barrier();
    CSTAMP(7);
}

// Phases 3-4 of k_ctrl, two-chain schedule (lh_ctrl_nd_plan): the system is in LDS in
// the order [long part | short part | separator] (lh_nd_pos), the two parts decoupled, so their LDL^T
// are independent chains.  Step t eliminates chain 0's block c0(t) (the long part's blocks, then the
// separator's) and chain 1's block c1(t) (the short part's, while they last); one barrier per step.
//   wave 0 / wave 1: the next diagonal tile of chain 0 / 1 (every source of the step reaching it), then
//                    that chain's next factor (N by chain and step parity, ND per block);
//   other waves:     their unit (nd_tile_row: up to both sources per tile, tile rows and columns absolute);
//   wave 12 / 13:    z of chain 0's / 1's block first.
// The back substitution is the one-chain one over the factor order; x goes out in natural order.
__device__ __forceinline__ void lds_ldlt_solve_nd(double* __restrict__ A, double* __restrict__ xsol, int n, int tid,
                                                  const uint16_t* __restrict__ units, const lh_params& prm) {
    const int lane = tid & 63, wave = tid >> 6;
    LdltBlockLds& F = ldlt_lds();
    const int nb = (n + 7) & ~7;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int P = prm.P, a = prm.nd_a, sep = prm.nd_s, lf = prm.nd_long_first, T = prm.nd_steps;
    const int b = P - a - sep;
    const int nl_blk = 6 * (lf ? a : b) / 8, ns_blk = 6 * (lf ? b : a) / 8;
    auto c0 = [&](int t) { return t < nl_blk ? t : t + ns_blk; };          // chain 0's block at step t
    auto c1 = [&](int t) { return t < ns_blk ? nl_blk + t : -1; };        // chain 1's (-1: done)
    const LdsSys SY{A};
    const uint32_t uwv = (lane < LH_NSTEP) ? units[wv * LH_NSTEP + lane] : 0u;   // lane t: step t's unit word
    if (wv == 0) factor_block8(SY, F.N[0], F.ND[c0(0)], 8 * c0(0), lane);
    if (wv == 1 && ns_blk > 0) factor_block8(SY, F.N[2], F.ND[c1(0)], 8 * c1(0), lane);
    lds_barrier();
    CSTAMP(5);
    for (int t = 0; t < T; ++t) {
        const int par = t & 1, ka = c0(t), kb = c1(t);
        const NdSrc src[2] = {{F.N[par], F.ND[ka], 8 * ka}, {F.N[2 + par], F.ND[kb < 0 ? 0 : kb], 8 * kb}};
        if ((wv == 12 || (wv == 13 && kb >= 0)) && lane < 8) {   // z of the step's blocks (LDLT::_solve_impl)
            const int q0 = wv == 12 ? 0 : 1, k0 = src[q0].k0;
            const double* N = src[q0].N;
            double z = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) z += A[NP * AS + k0 + q] * N[q * 8 + lane];
            const double d = A[(k0 + lane) * AS + k0 + lane];
            F.z[k0 + lane] = fabs(d) > 2.2250738585072014e-308 ? z : 0.0;
        }
        const uint32_t uw = __builtin_amdgcn_readlane(uwv, t);
        const int smask = (uw >> 10) & 3, stmask = (uw >> 12) & 3;
        if (wv < 2) {
            const int nx = wv == 0 ? c0(t + 1) : c1(t + 1);
            const bool live = wv == 0 ? (t + 1 < T) : (kb >= 0 && nx >= 0);
            if (uw & LH_UNIT_VALID) {
                const int I = uw & 7;
                nd_tile_row(A, src, smask, 0, 16 * I, 16 * I, 16 * I + 16, lane);
                wave_sync();
            }
            if (live) factor_block8(SY, F.N[2 * wv + (par ^ 1)], F.ND[nx], 8 * nx, lane);
        } else if (uw & LH_UNIT_VALID) {
            const int I = uw & 7, jb0 = (uw >> 3) & 7, jb1 = (uw >> 6) & 15;
            nd_tile_row(A, src, smask, stmask, 16 * I, 16 * jb0, 16 * jb1, lane);
        }
        lds_barrier();
    }
    CSTAMP(6);
    if (wv == 0) {
        double y0 = (lane < nb) ? F.z[lane] : 0.0, y1 = (lane + 64 < nb) ? F.z[lane + 64] : 0.0;
        ldlt_backsub(A, F, nb, lane, y0, y1);
        // factor row r -> natural row 6 nat(r / 6) + r mod 6
        if (lane < n) xsol[6 * lh_nd_nat(lane / 6, P, a, sep, lf) + lane % 6] = y0;
        if (lane + 64 < n) xsol[6 * lh_nd_nat((lane + 64) / 6, P, a, sep, lf) + (lane + 64) % 6] = y1;
    }
    lds_barrier();
    CSTAMP(7);
}

// Phases 3-4 of k_ctrl, PCG variant (lh_options.linear_solver = LH_SOLVER_PCG): Jacobi-preconditioned
// conjugate gradients on the same permuted, padded system (A lower triangle + rhs row NP).  This is
// the solver the reference left commented out (problem.cpp:421-422 -> Problem::PCGSolver :584-614)
// with its stop rule, ||r|| <= 1e-6 ||b|| (:597), and iteration cap, 2 * rows (:422), but corrected:
// the reference never adds the first step alpha*p to x (:595-596); here every step is applied.
// A zero diagonal entry (STRATEGY1 with a fixed pose: 0 + lambda*0) preconditions with 0 instead of
// Eigen's inf (which would turn the whole step into NaN).
// Layout: eight waves, the system cached in registers.  Wave w < 8 owns rows 16w .. 16w + 15; lane l
// holds row 16w + (l & 15) at columns 32 (l >> 4) + j, j < 32 (32 doubles).  A matrix-vector product is
// then 32 FMAs per lane on 16-byte broadcast reads of the vector, and a 2-level butterfly (lane ^ 16, 32) over
// the four lanes sharing a row; each row's scalars (x, r, z, p, q, 1/d) are replicated over those
// lanes.  Two workgroup barriers per step, the CG recurrence regrouped so that one product serves a
// step: with z published, q = A p = A z + beta q_prev and p = z + beta p_prev (the same iteration,
// rounded differently: parity to tolerance, as before).  The dot products are fixed-order sums
// (16-row wave butterflies, then the 8 wave partials in order), so a solve is bitwise repeatable.
// Waves 8-15 only keep the barrier count and the stop test (the r.r total, the same bits).  Per step
// the SIMD issue is what costs: all 16 waves doing the row scalars' replicated work took 1.85 us per
// step on C3; the round-2 layout (one wave, the system in LDS, an n-long FMA chain per row) ~2.5 us;
// round 1 (eight threads per row, three barriers) ~3 us.
// At most max_it steps (callers pass the reference cap + 1: its first step precedes its loop).
// Returns the iteration count.  Must be called by all CT threads; xsol[r] = x in pivot order.
__device__ __forceinline__ int lds_pcg_solve(double* __restrict__ A, double* __restrict__ xsol, double* __restrict__ pv,
                                             double* __restrict__ s_red2, int n, int tid, double tol_rel, int max_it) {
    constexpr int PW = 8;   // PCG waves
    static_assert(CT / 64 >= PW && NP == 16 * PW, "8 waves x 16 rows, 4 column blocks x 32");
    const int lane = tid & 63, wave = tid >> 6;
    const bool act = wave < PW;
    const int row = 16 * wave + (lane & 15), k = lane >> 4;
    const bool vr = act && row < n;
    double a[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const int c = 32 * k + j;
        a[j] = (vr && c < n) ? A[max(row, c) * AS + min(row, c)] : 0.0;   // S(i, j) = A[max * AS + min]
    }
    const double d = vr ? A[row * AS + row] : 0.0;
    const double id = (d != 0.0) ? 1.0 / d : 0.0;
    double r = vr ? A[NP * AS + row] : 0.0;
    double x = 0.0, z = r * id, p = 0.0, q = 0.0, beta = 0.0;
    double* red_pq = s_red2;                                            // [PW] wave partials of p.q
    double2* red_zr = reinterpret_cast<double2*>(s_red2 + 16);          // [PW] of (r.z, r.r)
    auto rows16 = [&](double v) {       // the wave's 16 rows (every lane gets the sum)
        double t[1] = {v};
        group_sum(t, 4);
        return t[0];
    };
    auto total = [&](const double* red) {   // in wave order
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < PW; ++w) t += red[w];
        return t;
    };
    auto total2 = [&](double& tz, double& tr) {
        tz = 0.0;
        tr = 0.0;
#pragma unroll
        for (int w = 0; w < PW; ++w) {
            const double2 t = red_zr[w];
            tz += t.x;
            tr += t.y;
        }
    };
    if (act) {
        if (k == 0 && row < NP) pv[row] = z;
        const double wrz = rows16(r * z), wrr = rows16(r * r);
        if (lane == 0) red_zr[wave] = double2{wrz, wrr};
    }
    lds_barrier();
    double rz, rr0;
    total2(rz, rr0);
    const double bnorm = sqrt(rr0);
    const double thr = tol_rel * bnorm;
    int it = 0;
    if (bnorm > 0.0) {
#pragma clang loop unroll(disable)
        while (it < max_it) {
            if (act) {
                // s = A z (z published in pv), then q = s + beta q, p = z + beta p
                double sp[4] = {0.0, 0.0, 0.0, 0.0};
                const double2* pz = reinterpret_cast<const double2*>(pv + 32 * k);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const double2 v = pz[j];
                    sp[(2 * j) & 3] += a[2 * j] * v.x;
                    sp[(2 * j + 1) & 3] += a[2 * j + 1] * v.y;
                }
                double sv = (sp[0] + sp[1]) + (sp[2] + sp[3]);
                sv = xor16_sum(sv);
                sv = xor32_sum(sv);
                q = sv + beta * q;
                p = z + beta * p;
                const double wpq = rows16(vr ? p * q : 0.0);
                if (lane == 0) red_pq[wave] = wpq;
            }
            lds_barrier();
            if (act) {
                const double alpha = rz / total(red_pq);
                x += alpha * p;
                r -= alpha * q;
                z = r * id;
                const double wrz = rows16(vr ? r * z : 0.0), wrr = rows16(vr ? r * r : 0.0);
                if (lane == 0) red_zr[wave] = double2{wrz, wrr};
                if (k == 0 && row < NP) pv[row] = z;
            }
            lds_barrier();
            ++it;
            double rzn, rrn;
            total2(rzn, rrn);
            if (!(sqrt(rrn) > thr)) break;   // also stops on NaN; the same bits in every wave
            beta = rzn / rz;
            rz = rzn;
        }
    }
    if (k == 0 && vr) xsol[row] = x;
    lds_barrier();
    return it;
}
