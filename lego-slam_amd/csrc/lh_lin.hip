// lh_lin.hip — k_lin, the first kernel of an LM trial of lego::Problem::solve (src/lego/base/problem.cpp:179-220).
//   k_lin     landmark chunks: back-substitute the pending pose step into the
//             landmarks, evaluate chi2 at the candidate state and relinearise
//             there (residual, SE(3)/point Jacobians, Huber weights, H_pp, H_pl,
//             H_ll, b), eliminate the landmarks (Schur) — the landmark part as
//             an f64 MFMA SYRK over a chunk window — and emit one slab per chunk.
// k_reduce and the controllers (lh_kernels.hip and the files it includes) follow.  Every reduction has a fixed order, so a solve is bitwise
// reproducible.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "lh_launch.h"
#include "lh_dev.h"
#include "lh_edge.h"

#pragma clang fp contract(fast)

// ============================================================================
// k_lin: one workgroup (4 waves) per landmark chunk; one sub-batch (<= 8
// landmarks, <= 64 observations, one observation per lane) per wave at a time.
// ============================================================================
// LDS strides of k_lin's window pose tables and landmark-record stage, padded off the global
// ones so the entries lanes read at once fall in distinct bank groups: 26 doubles = 52 dwords puts
// 16 (slot, camera) entries on 16 distinct 4-bank groups (24 gave 4), 18 = 36 dwords puts the 8
// records of a sub-batch on 8 (16 gave 2).  Both keep 16-byte alignment for b128 loads.
#define LH_PT_LDS 26
#define LH_REC_LDS 18

template <int T>
struct LinCfg {
    static constexpr int NT = T * (T + 1) / 2;          // upper MFMA tiles of the window
    // G row stride: >= 16T and = 16 mod 32 doubles (conflict-free b64 fragment loads)
    static constexpr int GS = (T == 1) ? 16 : (T <= 3 ? 48 : (T <= 5 ? 80 : 112));
    static constexpr int UMAX = (16 * T) / 6;           // window poses that fit 16T rows
    // the chunk slab as combined in LDS: NT tiles | UMAX x 33 per-pose sums | 4 scalars (written out
    // as pair rows and the chunk scalars)
    static constexpr int LS_TASK = NT * 256, LS_SC = LS_TASK + UMAX * LH_TASKS, LS = LS_SC + 8;
    // per-wave LDS scratch: pose-sum image [slot][landmark][33], G image [24][GS], the record
    // stage (8 x LH_REC_LDS), and (over the 4 waves) the two combine slabs
    static constexpr int A_ = UMAX * LH_SB_LM * LH_TASKS, B_ = 3 * LH_SB_LM * GS, C_ = (2 * LS + 3) / 4;
    static constexpr int SCR = ((A_ > B_ ? (A_ > C_ ? A_ : C_) : (B_ > C_ ? B_ : C_)) + 1) & ~1;
};

// a landmark record's 16-byte pieces (rec_rsrc: a buffer descriptor over the record buffer)
__device__ __forceinline__ void st_rec2(double2* p, double2 v, __amdgpu_buffer_rsrc_t rsrc, const double* base) {
    if constexpr (LH_WT_REC) {
        const int off = (int)((const char*)p - (const char*)base);
        typedef int v4i __attribute__((ext_vector_type(4)));
        v4i x;
        __builtin_memcpy(&x, &v, 16);
        __builtin_amdgcn_raw_buffer_store_b128(x, rsrc, off, 0, 16);   // aux 16: sc1 (write-through)
    } else {
        *p = v;
    }
}

static_assert(offsetof(lh_chunk, sb_end) == 4 && offsetof(lh_chunk, U) == 8, "k_lin reads the chunk header as dwords");

// ---- back-substitution of the pending pose step (problem.cpp:426-429) for one sub-batch: the lane's edge term
//      J_l^T W J_p dx (at the committed linearisation: pt the committed pose table, d the slot's step), summed over
//      the landmark's lane group, then the landmark's update from its cached factor cl (VertexXYZ::add) and the
//      lead lane's gain-scale term (isGoodStepInLM's scale) ----
// (1) the edge's weight and Jacobians at the committed linearisation: pt the committed pose table, X the
//     committed landmark (a live edge only)
template <bool F32>
__device__ __forceinline__ void backsub_jac(const double* __restrict__ pt, const double* __restrict__ e, bool ext_id,
                                            bool ext_rot, double u, double v, int wfl, const double (&X)[3],
                                            const lh_params& prm, EdgeEval& E) {
    if constexpr (F32) {   // fp64 residual and weight (as below), fp32 Jacobians
        if (wfl) {
            E.W00 = 1.0; E.W01 = 0.0; E.W10 = 0.0; E.W11 = 1.0;
        } else {
            double Pc[3];
            edge_residual(pt, e, ext_id, ext_rot, X, u, v, prm, E.r0, E.r1, Pc);
            edge_robust(E, prm);
        }
        edge_eval_f<false, true>(pt, e, ext_id, ext_rot, X, u, v, prm, E);
    } else {
        double Pc[3];
        if (wfl) {   // an inlier at the committed linearisation: W = I, no residual needed
            E.W00 = 1.0; E.W01 = 0.0; E.W10 = 0.0; E.W11 = 1.0;
            edge_pc(pt, e, ext_id, ext_rot, X, Pc);
        } else {
            edge_residual(pt, e, ext_id, ext_rot, X, u, v, prm, E.r0, E.r1, Pc);
            edge_robust(E, prm);
        }
        edge_jac_pc(Pc, pt + LH_PT_RT, e, ext_rot, prm, E.Jp, E.Jl);
    }
}
// (2) the step d's term J_l^T W J_p d over the landmark's lane group, the landmark's update from its cached factor
//     cl, and the lead lane's gain-scale term at lambda.  The multiply-adds are explicit fused ones: where the
//     compiler contracts a * b + c * d it picks the product to fuse by the products' use counts, which depend on the
//     code around the call, and the batch path (one Jacobian, several steps) and the trial path must round alike.
//     The forms below are the ones the trial path was compiled to (the pre-split build's bits, scripts/lib_bitwise.py).
__device__ __forceinline__ void backsub_apply(const EdgeEval& E, bool live, const double* __restrict__ d, int lg,
                                              bool lmok, bool lead, const double (&cl)[12], double lambda,
                                              const lh_params& prm, double (&X)[3], double& scale_acc) {
    double v3[3] = {0.0, 0.0, 0.0};
    if (live) {
        double jd0 = 0.0, jd1 = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            if (!jz(0, a)) jd0 = __builtin_fma(E.Jp[a], d[a], jd0);
            if (!jz(1, a)) jd1 = __builtin_fma(E.Jp[6 + a], d[a], jd1);
        }
        const double y0 = __builtin_fma(E.W01, jd1, E.W00 * jd0), y1 = __builtin_fma(E.W11, jd1, E.W10 * jd0);
#pragma unroll
        for (int c = 0; c < 3; ++c) v3[c] = __builtin_fma(E.Jl[c], y0, E.Jl[3 + c] * y1);
    }
    group_sum(v3, lg);
    const double s0 = v3[0], s1 = v3[1], s2 = v3[2];
    if (lmok) {
        // the cached factor holds 1/L_ii on the diagonal
        const double i00 = cl[0], l10 = cl[1], i11 = cl[2], l20 = cl[3], l21 = cl[4], i22 = cl[5];
        const double b0 = cl[6], b1 = cl[7], b2 = cl[8];
        const double t0 = b0 - s0, t1 = b1 - s1, t2 = b2 - s2;
        const double y0 = t0 * i00, y1 = __builtin_fma(-l10, y0, t1) * i11;
        const double y2 = __builtin_fma(-l21, y1, __builtin_fma(-l20, y0, t2)) * i22;
        double d2 = y2 * i22, d1 = __builtin_fma(-l21, d2, y1) * i11;
        double d0 = __builtin_fma(-l20, d2, __builtin_fma(-l10, d1, y0)) * i00;
        if (prm.guard && !(i00 == i00)) { d0 = d1 = d2 = 0.0; }   // skipped degenerate landmark
        double x0 = X[0], x1 = X[1], x2 = X[2];
        if (isfinite(d0) && isfinite(d1) && isfinite(d2)) { x0 += d0; x1 += d1; x2 += d2; }   // VertexXYZ::add
        if (lead) {
            double q0, q1, q2;
            if (prm.strategy == 0) {
                q0 = __builtin_fma(lambda, d0, b0); q1 = __builtin_fma(lambda, d1, b1); q2 = __builtin_fma(lambda, d2, b2);
            } else {
                q0 = __builtin_fma(lambda * cl[9], d0, b0); q1 = __builtin_fma(lambda * cl[10], d1, b1);
                q2 = __builtin_fma(lambda * cl[11], d2, b2);
            }
            const double sc = __builtin_fma(d2, q2, __builtin_fma(d0, q0, d1 * q1));
            scale_acc += sc;
        }
        X[0] = x0; X[1] = x1; X[2] = x2;
    }
}
template <bool F32>
__device__ __forceinline__ void lin_backsub(const double* __restrict__ pt, const double* __restrict__ e,
                                            const double* __restrict__ d, bool live, bool ext_id, bool ext_rot, double u,
                                            double v, int wfl, int lg, bool lmok, bool lead, const double (&cl)[12],
                                            double lambda, const lh_params& prm, double (&X)[3], double& scale_acc) {
    EdgeEval E;
    if (live) backsub_jac<F32>(pt, e, ext_id, ext_rot, u, v, wfl, X, prm, E);
    backsub_apply(E, live, d, lg, lmok, lead, cl, lambda, prm, X, scale_acc);
}

// A batch group's candidate pose tables (k_lin's batch path, all threads): item i < gn U is rung i / U's candidate
// pose of slot i % U, from the committed pose pm (slot's pose cpose[slot]) and the rung's step (LDS wd + 6 U r),
// staged in LDS cand; then item j < gn U ncam builds the table of (rung, slot, camera) into LDS tabs + per_tab r,
// as k_lin's own candidate build does.  LDS operands as offsets into the dynamic LDS; out of line, so that its
// registers are not the trial path's.  NTH: the workgroup's threads.
template <int NTH>
__device__ __attribute__((noinline)) void lin_cand_batch(const double* __restrict__ pm, const uint16_t* __restrict__ cpose,
                                                         int pmax1, int U, int ncam, int gn, int o_wd, int o_cand,
                                                         int o_tabs, int per_tab, int o_wext) {
    extern __shared__ __attribute__((aligned(16))) double dsm[];
    const int tid = threadIdx.x;
    for (int i = tid; i < gn * U; i += NTH) {
        const int r = i / U, sl = i - r * U;
        const uint32_t pp = min((uint32_t)cpose[sl], (uint32_t)pmax1);
        double pmc[12], To[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) pmc[k] = pm[pp * 12 + k];
        d_pose_candidate(pmc, dsm + o_wd + 6 * U * r + 6 * sl, To);
#pragma unroll
        for (int k = 0; k < 12; ++k) dsm[o_cand + 12 * i + k] = To[k];
    }
    lds_barrier();
    for (int i = tid; i < gn * U * ncam; i += NTH) {
        const int r = i / (U * ncam), j = i - r * U * ncam, sl = j / ncam, c = j - sl * ncam;
        double To[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) To[k] = dsm[o_cand + 12 * (r * U + sl) + k];
        d_pose_table(To, dsm + o_wext + c * LH_EXT, dsm + o_tabs + per_tab * r + (sl * ncam + c) * LH_PT_LDS);
    }
}

#ifndef LH_LIN_OCC
#define LH_LIN_OCC 2   // k_lin<T <= 3> workgroups per CU the registers are budgeted for
#endif
// NW: the workgroup's waves.  4: up to LH_LIN_OCC workgroups share a CU.  8 (T <= 3 only, the planner's choice for a
// window that fills the GPU, lh_plan.cpp): one workgroup holds a CU's whole share, its 8 waves at k_lin's ~210 VGPRs
// fill the register file, so no second workgroup joins and waves w and w + 4 are the two of one SIMD (the HW_ID
// period DESIGN.md 2.2 records).  Sub-batch i of the chunk runs on wave i mod NW, so the waves that run one
// sub-batch more than the others (the first n mod NW) sit on distinct SIMDs whenever n mod 8 <= 4.
template <int T, bool TRIAL, bool F32, int NW>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 1 : ((T <= 3) ? LH_LIN_OCC : 1)) void k_lin(
    const lh_chunk* __restrict__ chunks, const lh_subbatch* __restrict__ sbs, const float* __restrict__ obs_uv,
    const uint32_t* __restrict__ obs_meta, double* __restrict__ rec, double* __restrict__ pose_tab,
    const double* __restrict__ ext, const lh_ctrl* __restrict__ ctrl, const double* __restrict__ dxp,
    double* __restrict__ edge_rho, double* __restrict__ rows, double* __restrict__ csc,
    const uint32_t* __restrict__ crow, uint8_t* __restrict__ wflag, long nslots,
    lh_params prm, int nrec, const uint64_t* __restrict__ fixed_bits, int chunk_base,
    double* __restrict__ pose_mat, int writer, lh_reset_args rst) {
    using Cfg = LinCfg<T>;
    static_assert(NW == 4 || (NW == 8 && T <= 3), "4 waves, or 8 for T <= 3");
    constexpr int NTH = 64 * NW;   // threads
    extern __shared__ __attribute__((aligned(16))) double dsm[];

    // The prologue's global loads go out in two dependent rounds: (1) the controller words and the
    // chunk header (scalar), then every independent vector load, the first sub-batch's prefetch
    // included; (2) the pose-table and pose-step values, whose addresses need the chunk's pose slots.
    // Written as per-element loops, each loop iteration waited for its own loads (ten serialised
    // round trips before the first sub-batch).
    // the initial linearisation restarts the solve (rst, its writer block below): the controller is not read
    const int done = TRIAL ? __builtin_amdgcn_readfirstlane(ctrl->done) : 0;
    const int cur = TRIAL ? __builtin_amdgcn_readfirstlane(ctrl->cur) : 0;
    // the re-linearisation of an evaluate-only acceptance (ctrl->relin, ctrl_lm_step): no back substitution and
    // no candidate; the committed landmarks and pose tables are linearised into the candidate side, which the
    // chain's decision commits (the writer copies the committed poses and tables across first)
    const bool relin = TRIAL && __builtin_amdgcn_readfirstlane(ctrl->relin) != 0;
    // the evo word: a trial of the final LM iteration or after a rejection (ctrl_lm_step) only evaluates, and above
    // its low byte the rung count of a batch of such trials (k_reduce's decision; the batch path after the tables)
    const int evw = TRIAL ? __builtin_amdgcn_readfirstlane(ctrl->evo) : 0;
    const int nbatch = max(evw >> 8, 1);
    // the pending step: lambda-ladder rung ctrl->lad's (the rung the last decision moved to; 0 after a factor)
    if (TRIAL) dxp += (size_t)__builtin_amdgcn_readfirstlane(ctrl->lad) * prm.n;
    // The candidate poses of a trial (VertexPose::add of the step k_ctrl solved) are built here, not in
    // the serial controller: every chunk builds its own window's candidate pose tables (wave 3, below),
    // and block 0 of one launch per trial (writer) stores every candidate pose and its tables, which a
    // later trial reads as committed and the caller as the result.
    if (!TRIAL && writer && blockIdx.x == 0) {   // the restart (what a separate reset kernel did)
        // (ctrl and dxp are read-only to every trial launch; in this launch no other block reads them, and
        // the controller words written here are read by the later kernels of the chain)
        int* c = reinterpret_cast<int*>(const_cast<lh_ctrl*>(ctrl));
        for (int i = threadIdx.x; i < (int)(sizeof(lh_ctrl) / sizeof(int)); i += NTH) c[i] = 0;   // cur = 0
        for (int i = threadIdx.x; i < rst.nqt; i += NTH) pose_mat[i] = rst.qt_init[i];
        for (int i = threadIdx.x; i < rst.nptab; i += NTH) pose_tab[i] = rst.ptab_init[i];
        for (int i = threadIdx.x; i < rst.ndxp; i += NTH) const_cast<double*>(dxp)[i] = 0.0;
        return;
    }
    if (TRIAL && writer && blockIdx.x == 0) {
        if (done || nbatch > 1) return;   // (a batch writes no candidate: its accepted rung is re-run in full)
        const int P = prm.P, nc = prm.ncam, cnd = 1 - cur;
        if (relin) {
            for (int i = threadIdx.x; i < P * 12; i += NTH) pose_mat[(size_t)cnd * P * 12 + i] = pose_mat[(size_t)cur * P * 12 + i];
            for (int i = threadIdx.x; i < P * nc * LH_PT; i += NTH)
                pose_tab[(size_t)cnd * P * nc * LH_PT + i] = pose_tab[(size_t)cur * P * nc * LH_PT + i];
            return;
        }
        for (int p = threadIdx.x; p < P; p += NTH) {
            double Tc[12], To[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) Tc[i] = pose_mat[(size_t)cur * P * 12 + p * 12 + i];
            d_pose_candidate(Tc, dxp + 6 * p, To);
#pragma unroll
            for (int i = 0; i < 12; ++i) pose_mat[(size_t)cnd * P * 12 + p * 12 + i] = To[i];
            for (int c = 0; c < nc; ++c)
                d_pose_table(To, ext + LH_EXT * c, pose_tab + (size_t)cnd * P * nc * LH_PT + (p * nc + c) * LH_PT);
        }
        return;
    }
    const int chunk = chunk_base + blockIdx.x - (writer ? 1 : 0);
    // a trial of the final LM iteration (ctrl->evo, ctrl_lm_step): back substitution and the
    // candidate's evaluation only (landmark positions, rho0 per edge, chi2 and the gain scale)
    const bool evo = evw != 0;
    const double lambda = TRIAL ? ctrl->lambda : 0.0;
    const uint32_t* __restrict__ chw = reinterpret_cast<const uint32_t*>(chunks + chunk);
    const uint32_t sb_begin = __builtin_amdgcn_readfirstlane(chw[0]), sb_end = __builtin_amdgcn_readfirstlane(chw[1]);
    const int U = (int)(__builtin_amdgcn_readfirstlane(chw[2]) & 0xffu);   // lh_chunk: {sb_begin, sb_end, U, T, ...}
    const uint32_t item_base = chunks[chunk].item_base;
    if (done) return;
    const int cand = 1 - cur;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: scalar loads, scalar loop
    const int ncam = prm.ncam;
    const int PT = prm.P * ncam * LH_PT;
    const uint16_t* __restrict__ cpose = chunks[chunk].pose;

    double* scr = dsm + wave * Cfg::SCR;
    // the chunk's window, LDS-resident: committed and candidate pose tables per (slot, camera),
    // the pending pose step per slot, the camera extrinsics
    double* wt_c = dsm + NW * Cfg::SCR;
    double* wt_n = wt_c + Cfg::UMAX * ncam * LH_PT_LDS;     // a chunk of T tiles has U <= UMAX poses
    double* wdx = wt_n + Cfg::UMAX * ncam * LH_PT_LDS;
    double* wext = wdx + Cfg::UMAX * 6;
    // after the pair-row map: the flag raised when wave 3 has built the candidate tables
    int* cflag = reinterpret_cast<int*>(wext + ncam * LH_EXT + (Cfg::UMAX * (Cfg::UMAX + 1) / 2 + 1) / 2);
    double pmc[12];
    // the wave that builds the candidate pose tables.  4 waves: 3 or 2 by block parity, so the two chunks sharing a
    // CU build them on different SIMDs (measured 37.7 -> 37.5 us per k_lin against wave 3 in both).  8 waves: the
    // last one, which never runs more sub-batches than another wave.
    const int cwave = NW - 1 - (NW == 4 ? (blockIdx.x & 1) : 0);

    const double2* __restrict__ rc2 = reinterpret_cast<const double2*>(rec + (size_t)cur * nrec * LH_REC);
    // piece lane & 7 of sub-batch sbx's record (lane >> 3); the initial linearisation reads only X, from the window
    auto rec_piece = [&](int sbx) -> double2 {
        if constexpr (TRIAL) {
            return rc2[(size_t)sbx * 64 + lane];
        } else {
            const int q = lane & 7, l = rst.lm_perm[sbx * LH_SB_LM + (lane >> 3)];
            if (q > 1 || l < 0) return double2{0.0, 0.0};
            const double* X = rst.lm_in + 3 * (size_t)l;
            return q == 0 ? double2{X[0], X[1]} : double2{X[2], 0.0};
        }
    };
    double* __restrict__ rn = rec + (size_t)cand * nrec * LH_REC;
    // a descriptor over both record buffers (write-through record stores, LH_WT_REC)
    const __amdgpu_buffer_rsrc_t rec_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(rec, 0, (int)((size_t)2 * nrec * LH_REC * sizeof(double)), 0x00020000);

    v4d acc[Cfg::NT];
#pragma unroll
    for (int t = 0; t < Cfg::NT; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
    // per-pose sums: lane l owns the (slot, task) cells c = l + 64 i, c = 33 slot + task (all 64 lanes)
    constexpr int NCELL = (Cfg::UMAX * LH_TASKS + 63) / 64;
    double task[NCELL];
#pragma unroll
    for (int u = 0; u < NCELL; ++u) task[u] = 0.0;
    double chi_acc = 0.0, scale_acc = 0.0, maxd = 0.0, ndeg = 0.0;
    STAMP_DECL

    // prefetch of the first sub-batch: observation words and the 8 landmark records.  The
    // prefetch is unconditional (index clamped to the chunk) so the compiler can keep it in
    // flight with counted vmcnt waits across the iteration.
    const int sb_last = (int)sb_end - 1;
    int sb = (int)sb_begin + wave;
    // wflag[buffer][slot]: 1 where the linearisation that produced that buffer's state found the edge
    // an inlier (e2 <= delta^2, or no robust kernel), i.e. its robust weight W is exactly I
    const uint8_t* __restrict__ wf_c = wflag + (size_t)cur * nslots;
    uint8_t* __restrict__ wf_n = wflag + (size_t)cand * nslots;
    uint32_t meta_n;
    double u_n, v_n;
    double2 r_n;
    int wfl_n = 0;
    lh_subbatch S_n;
    {
        const int sbc = min(sb, sb_last);
        const int o = sbc * 64 + lane;
        S_n = sbs[sbc];
        meta_n = obs_meta[o];
        if (TRIAL) wfl_n = wf_c[o];
        const float2 z = reinterpret_cast<const float2*>(obs_uv)[o];   // the float pixel, widened exactly
        u_n = (double)z.x;
        v_n = (double)z.y;
        r_n = rec_piece(sbc);
    }
    {
        // round 1: the pose slot of each table element this thread copies, the extrinsics, the
        // chunk's pair rows (written by the epilogue); round 2: the table values and the pose step.
        // Every load is unconditional, its index clamped into range (a conditional load becomes a
        // branch, and the wait at its join serialises the rounds again); only the LDS writes are guarded.
        static_assert(6 * Cfg::UMAX <= 256 && Cfg::UMAX * (Cfg::UMAX + 1) / 2 <= 256 && 4 * LH_EXT <= 256,
                      "one element per thread");
        constexpr int NTAB = (Cfg::UMAX * 4 * LH_PT + NTH - 1) / NTH;   // ncam <= 4
        const int per = ncam * LH_PT, ne = U * per, nrow = U * (U + 1) / 2;
        const int umax1 = max(U - 1, 0);
        const uint32_t pmax1 = (uint32_t)(prm.P - 1);
        int tsl[NTAB];
        uint32_t tp[NTAB];
#pragma unroll
        for (int k = 0; k < NTAB; ++k) {
            const int i = tid + NTH * k;
            tsl[k] = min(i / per, umax1);
            tp[k] = min((uint32_t)cpose[tsl[k]], pmax1);
        }
        const bool has_dx = TRIAL && tid < 6 * U;
        const int di = min(tid / 6, umax1);
        const uint32_t dp = min((uint32_t)cpose[di], pmax1);
        const double ev = ext[min(tid, ncam * LH_EXT - 1)];
        const uint32_t rw = crow[item_base + min(tid, max(nrow - 1, 0))];
        double tc[NTAB], tn[NTAB];
#pragma unroll
        for (int k = 0; k < NTAB; ++k) {
            const int i = tid + NTH * k;
            const size_t g = (size_t)tp[k] * per + min(max(i - tsl[k] * per, 0), per - 1);
            tc[k] = pose_tab[(size_t)cur * PT + g];
            tn[k] = TRIAL ? 0.0 : rst.ptab_init[(size_t)cand * PT + g];   // a trial builds its candidate tables
        }
        if (TRIAL && wave == cwave) {   // the committed pose of slot lane (lane < U)
            const uint32_t pp = min((uint32_t)cpose[min(lane, umax1)], pmax1);
#pragma unroll
            for (int i = 0; i < 12; ++i) pmc[i] = pose_mat[(size_t)cur * prm.P * 12 + pp * 12 + i];
        }
        const double dv = TRIAL ? dxp[6 * dp + (tid - 6 * (tid / 6))] : 0.0;
#pragma unroll
        for (int k = 0; k < NTAB; ++k) {
            const int i = tid + NTH * k;
            if (i < ne) {
                const int r = i - tsl[k] * per, ent = r / LH_PT;
                const int l = (tsl[k] * ncam + ent) * LH_PT_LDS + (r - ent * LH_PT);
                wt_c[l] = tc[k];
                if (!TRIAL) wt_n[l] = tn[k];
            }
        }
        if (has_dx) wdx[tid] = dv;
        if (tid < ncam * LH_EXT) wext[tid] = ev;
        uint32_t* wrow = reinterpret_cast<uint32_t*>(wext + ncam * LH_EXT);
        if (tid < nrow) wrow[tid] = rw;
        if (tid == 0) *cflag = 0;
    }
    lds_barrier();   // window tables
    if (TRIAL && nbatch > 1) {
        // ---- a batch: the evaluate-only trials of rungs lad .. lad + nbatch - 1 after a rejection,
        //      each evaluated as the evaluate-only path below evaluates one trial: the back substitution of the
        //      rung's step at the rung's lambda, the rung's candidate pose tables, rho0 per edge (edge_rho + r nslots)
        //      and the chunk's chi2 and gain scale (csc + (r n_chunks + chunk) 4).  The rungs of a group share one
        //      pass over the chunk's sub-batches: an edge's weight and Jacobians at the committed state are computed
        //      once, then each rung's step is applied and its candidate evaluated.  Each lane's chi2 and scale sums
        //      per rung stay in LDS (the same per-lane order as the single-trial path).  Nothing else is written:
        //      k_reduce decides the rungs in order, and the next chain re-runs an accepted rung as a full trial.
        //      LDS: the trial path's wave scratch [0, NW SCR), free here: record stages, rung lambdas, the combine's
        //      wave totals, then per rung of a group: the lanes' sums, candidate tables, step, candidate poses. ----
        double* stg = dsm + wave * (8 * LH_REC_LDS);               // this wave's landmark-record stage
        double* lam_l = dsm + NW * 8 * LH_REC_LDS;           // [LH_LAD] the rungs' lambdas
        double* wtot = lam_l + LH_LAD;                             // [LH_LAD][NW][2] wave totals
        double* gbase = wtot + LH_LAD * NW * 2;
        const int per_tab = U * ncam * LH_PT_LDS;
        const int per_rung = 2 * NW * 64 + per_tab + 6 * U + 12 * U;
        const int avail = NW * Cfg::SCR - (int)(gbase - dsm);
        static_assert(NW * Cfg::SCR - (NW * 8 * LH_REC_LDS + LH_LAD + LH_LAD * NW * 2) >=
                          2 * NW * 64 + Cfg::UMAX * 4 * LH_PT_LDS + 18 * Cfg::UMAX,
                      "a batch group of one rung (4 cameras) fits the wave scratch");
        const int G = max(1, min(nbatch, avail / per_rung));      // rungs per group
        double* acc_c = gbase;                                     // [G][NW][64] chi2 per lane
        double* acc_s = acc_c + G * NW * 64;                       // [G][NW][64] gain scale per lane
        double* tabs = acc_s + G * NW * 64;                        // [G][per_tab] candidate tables
        double* wd = tabs + G * per_tab;                           // [G][6 U] steps
        double* cand = wd + G * 6 * U;                             // [G][U][12] candidate poses
        if (tid == 0) {   // rung r's lambda: r more rejections' updates (ctrl_lm_step, ladder_read's order)
            double lam = lambda, ni = ctrl->ni;
            for (int r = 0; r < nbatch; ++r) {
                if (r > 0) {
                    if (prm.strategy == 0) { lam *= ni; ni *= 2.0; }
                    else lam = fmin(lam * 11.0, 1e7);
                }
                lam_l[r] = lam;
            }
        }
        for (int g0 = 0; g0 < nbatch; g0 += G) {
            const int gn = min(G, nbatch - g0);
            lds_barrier();   // (the previous group's combine is done with the LDS)
            for (int i = tid; i < gn * 6 * U; i += NTH) {
                const int r = i / (6 * U), k = i - r * 6 * U;
                wd[i] = dxp[(size_t)(g0 + r) * prm.n + 6 * (size_t)min((uint32_t)cpose[k / 6], (uint32_t)(prm.P - 1)) + k % 6];
            }
            for (int i = tid; i < gn * NW * 64; i += NTH) { acc_c[i] = 0.0; acc_s[i] = 0.0; }
            lds_barrier();
            lin_cand_batch<NTH>(pose_mat + (size_t)cur * prm.P * 12, cpose, prm.P - 1, U, ncam, gn, (int)(wd - dsm),
                           (int)(cand - dsm), (int)(tabs - dsm), per_tab, (int)(wext - dsm));
            lds_barrier();
            for (int sbi = (int)sb_begin + wave; sbi < (int)sb_end; sbi += NW) {
                const lh_subbatch S = S_n;
                const int lg = S.lg, nlm = S.n_lm;
                const int ls = lane >> lg, gj = lane & ((1 << lg) - 1);
                const bool lmok = ls < nlm;
                const bool lead = gj == 0 && lmok;
                const uint32_t meta = meta_n;
                const double u = u_n, v = v_n;
                const double2 rr = r_n;
                const int wfl = wfl_n;
                const int o = sbi * 64 + lane;
                {   // the next sub-batch's words: after the wave's last one, its first again (the next group's)
                    const int sbw = sbi + NW < (int)sb_end ? sbi + NW : (int)sb_begin + wave;
                    const int sbn = min(sbw, sb_last);
                    const int on = sbn * 64 + lane;
                    S_n = sbs[sbn];
                    meta_n = obs_meta[on];
                    wfl_n = wf_c[on];
                    const float2 z = reinterpret_cast<const float2*>(obs_uv)[on];
                    u_n = (double)z.x;
                    v_n = (double)z.y;
                    r_n = rec_piece(sbn);
                }
                reinterpret_cast<double2*>(stg)[(lane >> 3) * (LH_REC_LDS / 2) + (lane & 7)] = rr;
                wave_sync();
                const double* myrec = stg + (ls & 7) * LH_REC_LDS;
                const double X[3] = {myrec[LH_REC_X], myrec[LH_REC_X + 1], myrec[LH_REC_X + 2]};
                double cl[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) cl[i] = myrec[LH_REC_L + i];
                wave_sync();
                const bool has = (meta & LH_META_VALID) != 0u;
                const int p = LH_META_POSE(meta), cam = LH_META_CAM(meta), slot = LH_META_SLOT(meta);
                const bool pfixed = (fixed_bits[p >> 6] >> (p & 63)) & 1ull;
                const bool live = has && !pfixed;
                const double* e = wext + cam * LH_EXT;
                const bool ext_id = (prm.ext_identity >> cam) & 1;
                const bool ext_rot = (prm.ext_rot_identity >> cam) & 1;
                EdgeEval E;
                if (live) backsub_jac<F32>(wt_c + (slot * ncam + cam) * LH_PT_LDS, e, ext_id, ext_rot, u, v, wfl, X, prm, E);
                for (int r = 0; r < gn; ++r) {
                    double Xr[3] = {X[0], X[1], X[2]};
                    const int ai = (r * NW + wave) * 64 + lane;
                    double sa = acc_s[ai];
                    backsub_apply(E, live, wd + r * 6 * U + 6 * slot, lg, lmok, lead, cl, lam_l[g0 + r], prm, Xr, sa);
                    acc_s[ai] = sa;
                    if (has) {
                        const double* pt = tabs + r * per_tab + (slot * ncam + cam) * LH_PT_LDS;
                        EdgeEval Ec;
                        double Pc[3];
                        edge_residual(pt, e, ext_id, ext_rot, Xr, u, v, prm, Ec.r0, Ec.r1, Pc);
                        edge_robust(Ec, prm);
                        st_out(edge_rho + (size_t)(g0 + r) * nslots + o, Ec.rho0);
                        acc_c[ai] = acc_c[ai] + Ec.rho0;
                    }
                }
            }
            // each rung's wave totals (the single-trial path's butterflies), then its chunk scalars in that path's
            // combine order (below)
            for (int r = 0; r < gn; ++r) {
                const int ai = (r * NW + wave) * 64 + lane;
                double t3[3] = {acc_c[ai], acc_s[ai], 0.0};
                group_sum(t3, 6);
                if (lane == 0) { wtot[(r * NW + wave) * 2] = t3[0]; wtot[(r * NW + wave) * 2 + 1] = t3[1]; }
            }
            lds_barrier();
            for (int i = tid; i < gn * 4; i += NTH) {
                const int r = i >> 2, k = i & 3;
                const double* wt = wtot + r * NW * 2;
                double v = 0.0;
                if (k < 2) {
                    if constexpr (NW == 4) v = (wt[0 * 2 + k] + wt[2 * 2 + k]) + (wt[1 * 2 + k] + wt[3 * 2 + k]);
                    else v = ((wt[0 * 2 + k] + wt[4 * 2 + k]) + (wt[2 * 2 + k] + wt[6 * 2 + k])) +
                             ((wt[1 * 2 + k] + wt[5 * 2 + k]) + (wt[3 * 2 + k] + wt[7 * 2 + k]));
                }
                csc[((size_t)(g0 + r) * prm.n_chunks + chunk) * 4 + k] = v;
            }
        }
        return;
    }
    // A trial's candidate pose tables (wt_n): wave cwave composes the window's candidate poses (lane = slot)
    // and their tables (lane = (slot, camera)) while the other waves start their first back
    // substitution, which needs only the committed tables; they wait on cflag before their first
    // evaluation at the candidate.  The last waves run one sub-batch fewer than wave 0 in most chunks.
    if (TRIAL && !relin && wave == cwave) {
        if (lane < U) {
            double To[12];
            d_pose_candidate(pmc, wdx + 6 * lane, To);
#pragma unroll
            for (int i = 0; i < 12; ++i) scr[lane * 12 + i] = To[i];
        }
        wave_sync();
        if (lane < U * ncam) {
            const int sl = lane / ncam, c = lane - sl * ncam;
            double To[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) To[i] = scr[sl * 12 + i];
            d_pose_table(To, wext + c * LH_EXT, wt_n + (sl * ncam + c) * LH_PT_LDS);
        }
        __hip_atomic_store(cflag, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    bool tabs_ready = !TRIAL || relin;
    LSTAMP_DECL(TRIAL && !evo && !relin, (int)blockIdx.x - (writer ? 1 : 0), NW, wave)
    const double* wt_l = relin ? wt_c : wt_n;   // the tables the edges are evaluated and linearised at

    for (; sb < (int)sb_end; sb += NW) {
        const lh_subbatch S = S_n;       // scalar words, prefetched one sub-batch ahead (sb is wave-uniform)
        const int lg = S.lg, nlm = S.n_lm;
        const int ls = lane >> lg, gj = lane & ((1 << lg) - 1);
        const bool lmok = ls < nlm;
        const bool lead = gj == 0 && lmok;           // one lane per landmark writes its record
        const uint32_t meta = meta_n;
        const double u = u_n, v = v_n;
        const double2 rr = r_n;
        const int wfl = wfl_n;
        const int o = sb * 64 + lane;
        {
            const int sbn = min(sb + NW, sb_last);
            const int on = sbn * 64 + lane;
            S_n = sbs[sbn];
            meta_n = obs_meta[on];
            if (TRIAL) wfl_n = wf_c[on];
            const float2 z = reinterpret_cast<const float2*>(obs_uv)[on];
            u_n = (double)z.x;
            v_n = (double)z.y;
            r_n = rec_piece(sbn);
        }
        // landmark records through LDS: lane -> its landmark's record (records LH_REC_LDS apart)
        reinterpret_cast<double2*>(scr)[(lane >> 3) * (LH_REC_LDS / 2) + (lane & 7)] = rr;
        wave_sync();
        const double* myrec = scr + (ls & 7) * LH_REC_LDS;
        double X[3] = {myrec[LH_REC_X], myrec[LH_REC_X + 1], myrec[LH_REC_X + 2]};
        double cl[12];
        if (TRIAL) {
#pragma unroll
            for (int i = 0; i < 12; ++i) cl[i] = myrec[LH_REC_L + i];
        }
        wave_sync();
        if (!evo) {
            // the pose-sum image [landmark][slot][33] starts at zero: cells without a live
            // observation then add exact zeros, and the per-slot sums need no masks or branches
            double2* z = reinterpret_cast<double2*>(scr);
            constexpr int nz = (LH_SB_LM * Cfg::UMAX * LH_TASKS) / 2;
#pragma unroll
            for (int k = 0; k < (nz + 63) / 64; ++k)
                if (k * 64 + lane < nz) z[k * 64 + lane] = double2{0.0, 0.0};
        }
        wave_sync();

        const bool has = (meta & LH_META_VALID) != 0u;
        const int p = LH_META_POSE(meta), cam = LH_META_CAM(meta), slot = LH_META_SLOT(meta);
        const bool pfixed = (fixed_bits[p >> 6] >> (p & 63)) & 1ull;
        const bool live = has && !pfixed;
        const double* e = wext + cam * LH_EXT;
        const bool ext_id = (prm.ext_identity >> cam) & 1;
        const bool ext_rot = (prm.ext_rot_identity >> cam) & 1;

        // ---- back-substitution of the pending pose step (problem.cpp:426-429) ----
        if (TRIAL && !relin)
            lin_backsub<F32>(wt_c + (slot * ncam + cam) * LH_PT_LDS, e, wdx + 6 * slot, live, ext_id, ext_rot, u, v, wfl,
                             lg, lmok, lead, cl, lambda, prm, X, scale_acc);
        STAMP(0);
        if (!tabs_ready) {   // wave-uniform: once per wave
            while (__hip_atomic_load(cflag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) __builtin_amdgcn_s_sleep(1);
            tabs_ready = true;
        }

        if (evo) {   // the same evaluation as below, without the linearisation
            if (has) {
                const double* pt = wt_l + (slot * ncam + cam) * LH_PT_LDS;
                EdgeEval E;
                double Pc[3];
                edge_residual(pt, e, ext_id, ext_rot, X, u, v, prm, E.r0, E.r1, Pc);
                edge_robust(E, prm);
                st_out(edge_rho + o, E.rho0);
                chi_acc += E.rho0;
            }
            if (lead) {
                double* rw = rn + ((size_t)sb * LH_SB_LM + ls) * LH_REC;
                st_rec2(reinterpret_cast<double2*>(rw), double2{X[0], X[1]}, rec_rsrc, rec);
                st_out(rw + 2, X[2]);
            }
            continue;
        }

        // ---- evaluate and linearise at the candidate (problem.cpp:285-331, :523-526) ----
        // H_pp and b_p go straight to this lane's row of the pose-sum transpose
        double hll[6] = {0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0};
        double hpl[18];
#pragma unroll
        for (int i = 0; i < 18; ++i) hpl[i] = 0.0;
        // [landmark][slot][33]: unique writer; a wave's 16-lane store group covers distinct cells
        double* trow = scr + ((ls & 7) * Cfg::UMAX + slot) * LH_TASKS;
        if (has) {
            const double* pt = wt_l + (slot * ncam + cam) * LH_PT_LDS;
            EdgeEval E;
            double Pc[3];
            edge_residual(pt, e, ext_id, ext_rot, X, u, v, prm, E.r0, E.r1, Pc);
            edge_robust(E, prm);
            if constexpr (F32) edge_eval_f<false, true>(pt, e, ext_id, ext_rot, X, u, v, prm, E);
            else edge_jac_pc(Pc, pt + LH_PT_RT, e, ext_rot, prm, E.Jp, E.Jl);
            st_out(edge_rho + o, E.rho0);
            chi_acc += E.rho0;
            const bool inl = prm.huber_delta <= 0.0 || E.e2 <= prm.huber_delta * prm.huber_delta;
            wf_n[o] = inl ? 1 : 0;
            const double dr = (prm.huber_delta > 0.0) ? E.rho1 : 1.0;
            if (__ballot(!inl) == 0ull) lin_blocks<true>(E, pfixed, dr, hll, bl, hpl, trow);   // wave-uniform
            else lin_blocks<false>(E, pfixed, dr, hll, bl, hpl, trow);
        }
        STAMP(1);

        // ---- per-landmark H_ll, b_l over the lane group; Cholesky (redundant per lane) ----
        double h[9] = {hll[0], hll[1], hll[2], hll[3], hll[4], hll[5], bl[0], bl[1], bl[2]};
        group_sum(h, lg);
        // Cholesky of H_ll through reciprocal square roots: i_jj = 1/L_jj directly
        double i00 = fast_rsq(h[0]);
        const double l10 = h[1] * i00, l20 = h[2] * i00;
        const double a11 = h[3] - l10 * l10;
        const double i11 = fast_rsq(a11);
        const double l21 = (h[4] - l20 * l10) * i11;
        const double a22 = h[5] - l20 * l20 - l21 * l21;
        const double i22 = fast_rsq(a22);
        const bool pd = (h[0] > 0.0) && (a11 > 0.0) && (a22 > 0.0) && isfinite(i22) && isfinite(l21);
        // A landmark with one edge has a rank-2 H_ll: the reference's LU inverse (problem.cpp:399)
        // returns inf or rounding garbage for it.  Such a landmark (or a non-PD H_ll) poisons the
        // step like the inf does (guard 0: every trial is rejected, as the reference's solve is), or
        // is held fixed (guard 1).  The NaN reciprocal is the record's marker in both modes.
        const uint64_t vmask = __ballot(has);
        const uint64_t gmask = (lg >= 6) ? ~0ull : (((1ull << (1 << lg)) - 1ull) << (lane & ~((1 << lg) - 1)));
        const bool deg = !pd || __popcll(vmask & gmask) < 2;
        if (deg) i00 = __builtin_nan("");
        const double w0 = h[6] * i00, w1 = (h[7] - l10 * w0) * i11, w2 = (h[8] - l20 * w0 - l21 * w1) * i22;
        if (lead) {
            maxd = fmax(maxd, fmax(fabs(h[0]), fmax(fabs(h[3]), fabs(h[5]))));
            if (deg) ndeg += 1.0;
        }
        if (lmok) {
            // the record's eight 16-byte pieces from the landmark's lanes (every lane of the group holds the
            // same bits: butterfly totals, then the same arithmetic), piece q by lane q mod G: with G = 8 the
            // wave writes its 8 records as one contiguous 1 KB store (one piece per lane), whole 128-B lines
            // through the write-through path (8 pieces from the lead lane were 8 partial-line writes)
            double2* r2 = reinterpret_cast<double2*>(rn + ((size_t)sb * LH_SB_LM + ls) * LH_REC);
            for (int q = gj; q < 8; q += 1 << lg) {
                // piece q by a select tree on its bits (no divergent branches): 0 {X0, X1}, 1 {X2, i00},
                // 2 {l10, i11}, 3 {l20, l21}, 4 {i22, b0}, 5 {b1, b2}, 6 {H00, H11}, 7 {H22, 0}
                const bool q0 = q & 1, q1 = q & 2, q2 = q & 4;
                const double x01 = q0 ? X[2] : X[0], x23 = q0 ? l20 : l10, x45 = q0 ? h[7] : i22, x67 = q0 ? h[5] : h[0];
                const double y01 = q0 ? i00 : X[1], y23 = q0 ? l21 : i11, y45 = q0 ? h[8] : h[6], y67 = q0 ? 0.0 : h[3];
                const double x03 = q1 ? x23 : x01, x47 = q1 ? x67 : x45, y03 = q1 ? y23 : y01, y47 = q1 ? y67 : y45;
                st_rec2(r2 + q, double2{q2 ? x47 : x03, q2 ? y47 : y03}, rec_rsrc, rec);
            }
        }
        STAMP(2);

        // ---- per observation: G = H_pl L^-T and bsd = G w = H_pl H_ll^-1 b_l ----
        double G[18];
#pragma unroll
        for (int i = 0; i < 18; ++i) G[i] = 0.0;
        const bool gl = live && !(prm.guard && deg);
        if (gl) {
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double g0 = hpl[3 * a] * i00;
                const double g1 = (hpl[3 * a + 1] - l10 * g0) * i11;
                const double g2 = (hpl[3 * a + 2] - l20 * g0 - l21 * g1) * i22;
                G[3 * a] = g0; G[3 * a + 1] = g1; G[3 * a + 2] = g2;
                trow[27 + a] = g0 * w0 + g1 * w1 + g2 * w2;
            }
        }
        STAMP(3);

        // ---- per-pose sums (H_pp, b_p, bsd): the owner of cell (slot, task) adds it over every
        //      landmark observing the slot, in landmark (= lane) order ----
        wave_sync();
        {
            // every (landmark, slot) cell in landmark order: absent cells are +0.0, and adding
            // them leaves every sum bit-identical to adding the present cells only.  Cell c of
            // landmark l sits at scr[l * UMAX * 33 + c]: a wave's reads are contiguous.
#pragma unroll
            for (int i = 0; i < NCELL; ++i) {
                const int c = lane + 64 * i;
                if (c < U * LH_TASKS) {
                    double tv[LH_SB_LM];
#pragma unroll
                    for (int l = 0; l < LH_SB_LM; ++l) tv[l] = scr[l * Cfg::UMAX * LH_TASKS + c];
                    double sacc = task[i];
#pragma unroll
                    for (int l = 0; l < LH_SB_LM; ++l) sacc += tv[l];
                    task[i] = sacc;
                }
            }
        }
        wave_sync();
        STAMP(4);

        // ---- G rows into the window image [k][16T], then the MFMA SYRK ----
        {
            double2* z = reinterpret_cast<double2*>(scr);
            const int nz = (3 * LH_SB_LM * Cfg::GS) / 2;
            for (int i = lane; i < nz; i += 64) z[i] = double2{0.0, 0.0};
        }
        wave_sync();
        if (gl) {
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int j = 0; j < 3; ++j) scr[(3 * ls + j) * Cfg::GS + 6 * slot + a] = G[3 * a + j];
        }
        wave_sync();
        STAMP(5);
        const int nk = (3 * nlm + 3) >> 2;
        for (int s = 0; s < nk; ++s) {
            double f[T];
            const double* row = scr + (4 * s + (lane >> 4)) * Cfg::GS + (lane & 15);
#pragma unroll
            for (int R = 0; R < T; ++R) f[R] = row[16 * R];
            int t = 0;
#pragma unroll
            for (int R = 0; R < T; ++R)
#pragma unroll
                for (int Cc = R; Cc < T; ++Cc) {
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(f[R], f[Cc], acc[t], 0, 0, 0);
                    ++t;
                }
        }
        wave_sync();
        STAMP(6);
        LSTAMP_ROUND();
    }

    // ---- combine the waves in a fixed order and write the chunk slab.  NS = NW / 2 slabs in LDS: wave w < NS
    //      writes slab w, then wave w >= NS adds into slab w - NS, and the writers below add the slabs (s0..s3):
    //      4 waves (w0 + w2) + (w1 + w3); 8 waves ((w0 + w4) + (w2 + w6)) + ((w1 + w5) + (w3 + w7)), every slab the
    //      sum of one SIMD's two waves.  A wave without a sub-batch takes part with exact zeros. ----
    {   // the wave's totals: DPP and permlane butterflies (no LDS round trips); max |diag H_ll| likewise
        double t3[3] = {chi_acc, scale_acc, ndeg};
        group_sum(t3, 6);
        chi_acc = t3[0]; scale_acc = t3[1]; ndeg = t3[2];
        maxd = wave_max(maxd);
    }
    STAMP(9);
    lds_barrier();
    STAMP(8);
    constexpr int NS = NW / 2, LNS = NW == 8 ? 2 : 1;   // slabs, and log2 of them
    double* smem = dsm;
    if (evo) {   // the chunk's scalars only, combined in the same order as below
        for (int phase = 0; phase < 2; ++phase) {
            if ((wave >> LNS) == phase && lane == 0) {
                double* sc = smem + (wave & (NS - 1)) * 2;
                if (phase == 0) { sc[0] = chi_acc; sc[1] = scale_acc; }
                else { sc[0] += chi_acc; sc[1] += scale_acc; }
            }
            lds_barrier();
        }
        double* gs = csc + (size_t)chunk * 4;
        if constexpr (NW == 4) {
            if (tid < 2) gs[tid] = smem[tid] + smem[2 + tid];
        } else {
            if (tid < 2) gs[tid] = (smem[tid] + smem[4 + tid]) + (smem[2 + tid] + smem[6 + tid]);
        }
        if (tid == 2 || tid == 3) gs[tid] = 0.0;
        return;
    }
    static_assert(NW * Cfg::SCR >= NS * Cfg::LS, "the combine slabs fit the wave scratch");
    for (int phase = 0; phase < 2; ++phase) {
        if ((wave >> LNS) == phase) {
            double* sl = smem + (wave & (NS - 1)) * Cfg::LS;
            const bool first = phase == 0;
#pragma unroll
            for (int t = 0; t < Cfg::NT; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int idx = t * 256 + ((lane >> 4) + 4 * i) * 16 + (lane & 15);
                    sl[idx] = (first ? 0.0 : sl[idx]) + acc[t][i];
                }
#pragma unroll
            for (int i = 0; i < NCELL; ++i) {
                const int c = lane + 64 * i;
                if (c < U * LH_TASKS) {
                    const int idx = Cfg::LS_TASK + c;
                    sl[idx] = (first ? 0.0 : sl[idx]) + task[i];
                }
            }
            if (lane == 0) {
                double* sc = sl + Cfg::LS_SC;
                if (first) { sc[0] = chi_acc; sc[1] = scale_acc; sc[2] = ndeg; sc[3] = maxd; }
                else { sc[0] += chi_acc; sc[1] += scale_acc; sc[2] += ndeg; sc[3] = fmax(sc[3], maxd); }
            }
        }
        lds_barrier();
    }
    STAMP(9);
    // the chunk's contribution to each pose pair of its window, one pair row each (pair-major,
    // rows of one pair contiguous: k_reduce's loads need no index word).  Row: [0, 36) the
    // landmark part of S block (p, q), row-major; diagonal pairs also [36, 69) the pose's 33 sums.
    const double* s0 = smem;
    const double* s1 = smem + Cfg::LS;
    const double* s2 = smem + (NW == 8 ? 2 : 0) * Cfg::LS;   // (8 waves only)
    const double* s3 = smem + (NW == 8 ? 3 : 0) * Cfg::LS;
    const uint32_t* wrow = reinterpret_cast<const uint32_t*>(wext + ncam * LH_EXT);
    {
        const int a = lane / 6, bb = lane - 6 * (lane / 6);
        int lp = 0;
        for (int s = 0; s < U; ++s)
            for (int t = s; t < U; ++t, ++lp) {
                if ((lp & (NW - 1)) != wave) continue;
                double* row = rows + (size_t)wrow[lp] * LH_ROW;
                if (lane < 36) {
                    int ra = 6 * s + a, rc = 6 * t + bb;
                    if ((ra >> 4) > (rc >> 4)) { const int x = ra; ra = rc; rc = x; }
                    const int R = ra >> 4, Cc = rc >> 4;
                    const int idx = (R * T - (R * (R - 1)) / 2 + (Cc - R)) * 256 + (ra & 15) * 16 + (rc & 15);
                    if constexpr (NW == 4) st_out(row + lane, s0[idx] + s1[idx]);
                    else st_out(row + lane, (s0[idx] + s2[idx]) + (s1[idx] + s3[idx]));
                }
                if (s == t && lane < LH_TASKS) {
                    const int c = Cfg::LS_TASK + s * LH_TASKS + lane;
                    if constexpr (NW == 4) st_out(row + 36 + lane, s0[c] + s1[c]);
                    else st_out(row + 36 + lane, (s0[c] + s2[c]) + (s1[c] + s3[c]));
                }
            }
    }
    double* gs = csc + (size_t)chunk * 4;
    if constexpr (NW == 4) {
        if (tid < 3) gs[tid] = s0[Cfg::LS_SC + tid] + s1[Cfg::LS_SC + tid];
        if (tid == 3) gs[3] = fmax(s0[Cfg::LS_SC + 3], s1[Cfg::LS_SC + 3]);
    } else {
        if (tid < 3) gs[tid] = (s0[Cfg::LS_SC + tid] + s2[Cfg::LS_SC + tid]) + (s1[Cfg::LS_SC + tid] + s3[Cfg::LS_SC + tid]);
        if (tid == 3) gs[3] = fmax(fmax(s0[Cfg::LS_SC + 3], s2[Cfg::LS_SC + 3]), fmax(s1[Cfg::LS_SC + 3], s3[Cfg::LS_SC + 3]));
    }
    STAMP(10);
    STAMP_FLUSH(0, 11);
}

// dynamic LDS of k_lin<T, ., ., nw>: nw wave scratches + the chunk's pose tables, step and extrinsics
template <int T>
static size_t lin_smem_bytes(int ncam, int nw) {
    using Cfg = LinCfg<T>;
    return sizeof(double) * ((size_t)nw * Cfg::SCR + 2 * (size_t)Cfg::UMAX * ncam * LH_PT_LDS + Cfg::UMAX * 6 +
                             (size_t)ncam * LH_EXT + (Cfg::UMAX * (Cfg::UMAX + 1) / 2 + 1) / 2 + 1);
}

// The one list of k_lin's instantiations, T = 1..6 x TRIAL x F32 at 4 waves and T = 1..3 x TRIAL x F32 at 8: the
// kernel of (T, trial, f32, waves) and its LDS size (a null kernel outside the list).  Every launcher below goes
// through it.
struct LinInst {
    decltype(&k_lin<1, false, false, 4>) fn;
    size_t (*smem)(int ncam, int nw);
};
template <int T, int NW>
static LinInst lin_inst_t(bool trial, bool f32) {
    return {trial ? (f32 ? k_lin<T, true, true, NW> : k_lin<T, true, false, NW>)
                  : (f32 ? k_lin<T, false, true, NW> : k_lin<T, false, false, NW>),
            lin_smem_bytes<T>};
}
static LinInst lin_inst(int T, bool trial, bool f32, int nw) {
    if (nw == 8) {
        switch (T) {
            case 1: return lin_inst_t<1, 8>(trial, f32);
            case 2: return lin_inst_t<2, 8>(trial, f32);
            case 3: return lin_inst_t<3, 8>(trial, f32);
            default: return {nullptr, nullptr};
        }
    }
    if (nw != LH_WAVES) return {nullptr, nullptr};
    switch (T) {
        case 1: return lin_inst_t<1, 4>(trial, f32);
        case 2: return lin_inst_t<2, 4>(trial, f32);
        case 3: return lin_inst_t<3, 4>(trial, f32);
        case 4: return lin_inst_t<4, 4>(trial, f32);
        case 5: return lin_inst_t<5, 4>(trial, f32);
        case 6: return lin_inst_t<6, 4>(trial, f32);
        default: return {nullptr, nullptr};
    }
}

// ============================================================================
// launchers (host side)
// ============================================================================
extern "C" {

// dynamic LDS of k_lin<T> at nw waves for ncam cameras (the host rejects windows whose chunks would not fit a CU,
// and the planner keeps 4 waves where 8 would not); (size_t)-1 for a shape that does not exist
size_t lh_lin_smem(int T, int ncam, int nw) {
    const LinInst k = lin_inst(T, false, false, nw);
    return k.fn ? k.smem(ncam, nw) : (size_t)-1;
}

// Raise the dynamic-LDS limit of every k_lin instantiation on the current device (lh_create) to the
// device's per-workgroup LDS (hipDeviceAttributeMaxSharedMemoryPerBlock, read once by the host, which
// also rejects windows whose chunks would exceed it), before any launch.
hipError_t lh_prepare_lin(int lds_limit) {
    for (int nw = LH_WAVES; nw <= LH_WAVES_WG8; nw += LH_WAVES)
        for (int T = 1; T <= 6; ++T)
            for (int v = 0; v < 4; ++v) {
                const LinInst k = lin_inst(T, v & 1, v >> 1, nw);
                if (!k.fn) continue;
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k.fn),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds_limit);
                if (e != hipSuccess) return e;
            }
    return hipSuccess;
}

// nw: the waves per workgroup the window's plan chose (lh::Plan::lin_waves)
hipError_t lh_launch_lin(int T, int nw, int trial, int nchunks, int chunk_base, hipStream_t st, const lh_chunk* chunks,
                         const lh_subbatch* sbs, const float* obs_uv, const uint32_t* obs_meta, double* rec,
                         double* ptab, const double* ext, const lh_ctrl* ctrl, const double* dxp,
                         double* edge_rho, double* rows, double* csc, const uint32_t* crow, uint8_t* wflag, long nslots,
                         lh_params prm, int nrec, const uint64_t* fixed_bits, double* pose_mat, int writer,
                         lh_reset_args rst) {
    writer = writer ? 1 : 0;   // block 0 stores the trial's candidate poses and tables (the restart, initially)
    if (nchunks + writer <= 0) return hipSuccess;
    dim3 g(nchunks + writer), b(64 * nw);
    // (diagnostic) LH_TEST_LIN_LDS_PAD bytes of extra LDS per workgroup: fewer k_lin workgroups per CU, for the
    // latency-hiding probe of scripts/occupancy_probe.py
    static const size_t lds_pad = getenv("LH_TEST_LIN_LDS_PAD") ? (size_t)atol(getenv("LH_TEST_LIN_LDS_PAD")) : 0;
    const LinInst k = lin_inst(T, trial != 0, prm.precision == 1, nw);
    if (!k.fn) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k.fn, g, b, k.smem(prm.ncam, nw) + lds_pad, st, chunks, sbs, obs_uv, obs_meta, rec, ptab, ext, ctrl,
                       dxp, edge_rho, rows, csc, crow, wflag, nslots, prm, nrec, fixed_bits, chunk_base, pose_mat, writer,
                       rst);
    return hipGetLastError();
}

}  // extern "C"
