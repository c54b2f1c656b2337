// lh_cov.h — marginal covariances of a solved window (lh_covariance, include/lego_ba.h): the
// arguments of lh_cov.hip's kernels, shared with the host side, and the one piece of its arithmetic that is plain
// C++ (a landmark's 3x3 from its cached Cholesky factor), which tests/test_cov_cpu.py also compiles with g++.
//
// The pose part.  S = H_pp - H_pl H_ll^-1 H_lp at the returned state (k_lin<T, false> + k_reduce mode 0 on a copy of
// that state: no lambda anywhere).  The rows of the poses that are not held, compacted (lh_cov_args.rowmap), are
// factored S[f, f] = L L^T without pivoting in global memory (stride ns = ceil16(n_free), identity on the padding
// rows), W = L^-1 by block columns, and Sigma[f, f] = W^T W; held rows and columns stay +0.0.
//
// The landmark part.  Sigma_l = H_ll^-1 + H_ll^-1 M H_ll^-1, M = sum over the landmark's edges e, e' of
// H_lp,e Sigma_pp[p(e), p(e')] H_pl,e'.  With the record's factor H_ll = C C^T and N = C^-1 this is
// N^T (I + N M N^T) N (lh_cov_lm_finish).
#pragma once
#include <stdint.h>

#include "lh_common.h"

#define LH_COV_NB 16                         // block size of the factorisation, of W's block columns and of the Gram tiles
#define LH_COV_NSMAX (6 * LH_PMAX_WIN)       // rows at most (384: a multiple of LH_COV_NB)

// the result block the kernels fill (doubles; written with vector stores, one download with the arrays)
#define LH_COV_R_BAD 0        // first row (of the 6P) whose pivot was not > 0, else -1
#define LH_COV_R_MINP 1       // smallest and largest pivot L_ii^2 of the rows factored
#define LH_COV_R_MAXP 2
#define LH_COV_R_NFREE 3      // rows factored
#define LH_COV_R_NDEG 4       // rank-deficient landmarks of the linearisation (k_reduce's LH_SC_NDEG)
#define LH_COV_R_N 8

// k_cov_snapshot: the committed state of the last solve as a second set of lh_reset_args
struct lh_cov_snap_args {
    const lh_ctrl* ctrl;        // the solve's controller (cur: the committed side)
    const double* qt;           // [2][P][12] its poses
    const double* ptab;         // [2][npt] its pose tables
    const double* rec;          // [2][nrec][LH_REC] its landmark records
    const int32_t* lm_perm;     // [nrec] record -> window landmark (-1: padding)
    int32_t P, npt, nrec;
    double* qt_init;            // [2][P][12] out: the committed poses in both slots
    double* ptab_init;          // [2][npt] out: the committed tables in both slots
    double* lm;                 // [L][3] out: the committed positions of the landmarks that have a record
};

// k_cov_factor, k_cov_linv, k_cov_gram
struct lh_cov_args {
    const double* rs;           // the packed reduced system (lh_rs_make) of the linearisation
    const uint16_t* pair_pq;    // [npairs][2]
    const uint64_t* fixed_bits;
    int32_t P, npairs, anchor;
    int32_t ns;                 // ceil16(n_free): the stride of A and W
    int32_t* rowmap;            // [6P] row of the 6P -> row of S[f, f], -1 for a held pose's
    double* A;                  // [ns][ns] S[f, f] (lower), then its factor L
    double* W;                  // [ns][ns] L^-1 (block columns; blocks above the diagonal are not written)
    double* full;               // [6P][6P] Sigma_pp, zeroed by the caller
    double* blocks;             // [P][36] its diagonal blocks, zeroed by the caller
    double* res;                // [LH_COV_R_N]
};

// k_cov_lm
struct lh_cov_lm_args {
    const lh_subbatch* sbs;
    const float* obs_uv;
    const uint32_t* obs_meta;
    const double* rec;          // [nrec][LH_REC] the linearisation's records (X and the factor of H_ll)
    const double* ptab;         // [P * ncam][LH_PT] the committed pose tables
    const double* ext;
    const int32_t* lm_perm;
    const int32_t* rowmap;      // [6P] (a held pose: -1 at its first row)
    const double* full;         // [6P][6P] Sigma_pp
    const double* res;
    double* lm_cov;             // [L][9], pre-filled with NaN (a landmark without a record keeps it)
    int32_t n_sb, P;
};

// Sigma_l = N^T (I + N M N^T) N from the record's factor cl = {1/C00, C10, 1/C11, C20, C21, 1/C22} (LH_REC_L) and the
// upper triangle m = {M00, M01, M02, M11, M12, M22}; out row-major 3x3, one triangle computed and mirrored
LH_HD static inline void lh_cov_lm_finish(const double* cl, const double* m, double* out) {
    const double n00 = cl[0], n11 = cl[2], n22 = cl[5];
    const double n10 = -(cl[1] * n00) * n11;
    const double n21 = -(cl[4] * n11) * n22;
    const double n20 = -(cl[3] * n00 + cl[4] * n10) * n22;
    // B = N M (rows), T = B N^T (upper), R = I + T
    const double b00 = n00 * m[0], b01 = n00 * m[1], b02 = n00 * m[2];
    const double b10 = n10 * m[0] + n11 * m[1], b11 = n10 * m[1] + n11 * m[3], b12 = n10 * m[2] + n11 * m[4];
    const double b20 = n20 * m[0] + n21 * m[1] + n22 * m[2], b21 = n20 * m[1] + n21 * m[3] + n22 * m[4];
    const double b22 = n20 * m[2] + n21 * m[4] + n22 * m[5];
    const double r00 = 1.0 + b00 * n00;
    const double r01 = b00 * n10 + b01 * n11;
    const double r02 = b00 * n20 + b01 * n21 + b02 * n22;
    const double r11 = 1.0 + (b10 * n10 + b11 * n11);
    const double r12 = b10 * n20 + b11 * n21 + b12 * n22;
    const double r22 = 1.0 + (b20 * n20 + b21 * n21 + b22 * n22);
    // Q = R N (R symmetric), out = N^T Q (upper, mirrored)
    const double q00 = r00 * n00 + r01 * n10 + r02 * n20, q01 = r01 * n11 + r02 * n21, q02 = r02 * n22;
    const double q10 = r01 * n00 + r11 * n10 + r12 * n20, q11 = r11 * n11 + r12 * n21, q12 = r12 * n22;
    const double q20 = r02 * n00 + r12 * n10 + r22 * n20, q21 = r12 * n11 + r22 * n21, q22 = r22 * n22;
    const double o00 = n00 * q00 + n10 * q10 + n20 * q20;
    const double o01 = n00 * q01 + n10 * q11 + n20 * q21;
    const double o02 = n00 * q02 + n10 * q12 + n20 * q22;
    const double o11 = n11 * q11 + n21 * q21;
    const double o12 = n11 * q12 + n21 * q22;
    const double o22 = n22 * q22;
    out[0] = o00; out[1] = o01; out[2] = o02;
    out[3] = o01; out[4] = o11; out[5] = o12;
    out[6] = o02; out[7] = o12; out[8] = o22;
}
