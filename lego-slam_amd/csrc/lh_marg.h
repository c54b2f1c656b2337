// lh_marg.h — marginalising a keyframe of a solved window into a pose prior (lh_marginalize, include/lego_ba.h;
// DESIGN.md 2.13): the arguments of lh_marg.hip's kernels, shared with the host side, and the elimination's arithmetic
// in plain C++ (the 6x6 Cholesky factor, the forward substitution, one entry's rank-6 update), which
// tests/test_marg_cpu.py also compiles with g++.
//
// The system.  M: the landmarks with a valid edge to pose m.  k_marg_mask clears LH_META_VALID, in a copy of the
// observation words, on every edge of a landmark outside M; k_lin<T, false> + k_reduce (mode 0, guard 1) on that copy
// then form the lambda-free packed system of M's edges alone (a landmark without a valid edge takes k_lin's
// rank-deficient path and adds nothing).  k_marg_assemble scatters the packed blocks, plus an earlier prior, into the
// lower triangle of A [6P][6P] and factors A[m, m] = C C^T; k_marg_schur forms A[r, r] - Y^T Y, Y = C^-1 A[m, r].
#pragma once
#include <stdint.h>

#include "lh_common.h"

// the result block the kernels fill (doubles; written with vector stores, one download with the arrays)
#define LH_MARG_R_BAD 0       // first row (0..5) of A[m, m] whose pivot was not > 0, else -1
#define LH_MARG_R_MINP 1      // smallest and largest pivot C_ii^2 (0 when m is fixed: nothing is factored)
#define LH_MARG_R_MAXP 2
#define LH_MARG_R_ELIM 3      // 1: m was eliminated; 0: m is fixed (conditioning)
#define LH_MARG_R_NDEG 4      // rank-deficient landmarks of M (k_reduce's LH_SC_NDEG less the landmarks masked out)
#define LH_MARG_R_NLM 5       // landmarks of M
#define LH_MARG_R_NEDGE 6     // their valid edges
#define LH_MARG_R_N 8

// k_marg_mask
struct lh_marg_mask_args {
    const lh_subbatch* sbs;
    const uint32_t* obs_meta;   // [n_sb][64] the window's observation words
    const int32_t* lm_perm;     // [nrec] record -> window landmark (-1: padding)
    uint32_t* meta_out;         // [n_sb][64] out: the words with LH_META_VALID cleared outside M
    int32_t* counts;            // [n_sb][3] out: the sub-batch's landmarks of M, their valid edges, landmarks masked out
    uint8_t* lm_marg;           // [L] out (zeroed by the caller): 1 for a landmark of M
    int32_t n_sb, P, marg_pose;
};

// k_marg_assemble, k_marg_schur
struct lh_marg_args {
    const double* rs;           // the packed reduced system (lh_rs_make) of the masked linearisation
    const uint16_t* pair_pq;    // [npairs][2]
    const uint64_t* fixed_bits;
    const int32_t* counts;      // [n_sb][3] k_marg_mask's
    const double* prior_H;      // [6P][6P] an earlier prior (lower triangle read) or null
    const double* prior_b;      // [6P] or null
    int32_t P, npairs, marg_pose, n_sb;
    double* A;                  // [6P][6P] A_M + the earlier prior, lower triangle
    double* b;                  // [6P]
    double* Y;                  // [6][6P] C^-1 A[m, :]
    double* y;                  // [6] C^-1 b[m]
    double* H_prior;            // [6P][6P] out
    double* b_prior;            // [6P] out
    double* res;                // [LH_MARG_R_N]
};

// A = C C^T of the symmetric 6x6 a (row-major, its lower triangle read), without pivoting: c row-major, its lower
// triangle written.  Returns the first row whose pivot was not > 0 (c is then not to be used), else -1; minp, maxp:
// the smallest and largest pivot C_ii^2 of the rows factored.
LH_HD static inline int lh_marg_chol6(const double* a, double* c, double* minp, double* maxp) {
    double lo = 0.0, hi = 0.0;
    for (int j = 0; j < 6; ++j) {
        double d = a[6 * j + j];
        for (int k = 0; k < j; ++k) d -= c[6 * j + k] * c[6 * j + k];
        if (!(d > 0.0)) { *minp = lo; *maxp = hi; return j; }
        lo = (j == 0 || d < lo) ? d : lo;
        hi = d > hi ? d : hi;
        const double l = __builtin_sqrt(d);
        c[6 * j + j] = l;
        for (int i = j + 1; i < 6; ++i) {
            double s = a[6 * i + j];
            for (int k = 0; k < j; ++k) s -= c[6 * i + k] * c[6 * j + k];
            c[6 * i + j] = s / l;
        }
    }
    *minp = lo; *maxp = hi;
    return -1;
}

// x <- C^-1 x (forward substitution through the lower triangle of c), six entries `stride` apart
LH_HD static inline void lh_marg_fwd6(const double* c, double* x, int stride) {
    for (int i = 0; i < 6; ++i) {
        double s = x[(long)i * stride];
        for (int k = 0; k < i; ++k) s -= c[6 * i + k] * x[(long)k * stride];
        x[(long)i * stride] = s / c[6 * i + i];
    }
}

// a - sum_k yr[k stride] yc[k stride], k ascending: one entry of A[r, r] - Y^T Y (yr, yc: the entry's row's and
// column's columns of Y), and of b[r] - Y^T y.  Exchanging yr and yc gives the same bits; -0.0 never comes out.
LH_HD static inline double lh_marg_update(double a, const double* yr, const double* yc, int sr, int sc) {
    double s = a;
    for (int k = 0; k < 6; ++k) s -= yr[(long)k * sr] * yc[(long)k * sc];
    return s + 0.0;
}
