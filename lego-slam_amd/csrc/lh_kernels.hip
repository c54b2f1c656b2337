// lh_kernels.hip — k_reduce and the controllers of the sliding-window BA solver (CDNA4, gfx950): one translation
// unit of several files (why one: the closing comment).  Here k_reduce, k_ctrl and the launchers; the LM bookkeeping
// they share is lh_lm.h, the solves in LDS lh_ldlt.h, the controllers of larger windows lh_ctrl_g.hip,
// lh_ctrl_b.hip and lh_ctrl_p.hip, the test probes lh_probe.hip.  k_lin is lh_lin.hip, k_frames lh_frames.hip, the
// small kernels around a solve lh_aux.hip.
//
// One LM trial of lego::Problem::solve (src/lego/base/problem.cpp:179-220) is k_lin (lh_lin.hip), then
//   k_reduce  fixed-order sum of the pair rows into the reduced pose system.
//   k_ctrl    one workgroup: LM accept/reject and lambda schedule
//             (isGoodStepInLM, problem.cpp:520-581), LDLT of S + lambda
//             (problem.cpp:406-420), candidate poses T' = exp(dx) T
//             (VertexPose::add, lego_types.h:61-91).
// Every reduction has a fixed order, so a solve is bitwise reproducible.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <math.h>
#include <stdint.h>

#include "lh_launch.h"

#include "lh_dev.h"
#include "lh_lm.h"
#include "lh_ldlt.h"

#pragma clang fp contract(fast)

// ============================================================================
// k_reduce: fixed-order sum of chunk slabs into the reduced pose system.
// Block b < npairs handles pose pair (pp[b], pq[b]); block npairs the scalars.
// ============================================================================
__device__ __forceinline__ int hpp_index(int a, int b) {   // packed upper 6x6, a <= b
    return a * 6 - (a * (a - 1)) / 2 + (b - a);
}

constexpr int RT = 1024;      // k_reduce's threads
constexpr int RW = RT / 64;

// With prm.dec_in_reduce (one rank, P <= LH_PMAX) the scalar block also takes the trial's LM decision
// (isGoodStepInLM on its chi2 and gain-scale sums, the controller update, the host words): k_ctrl
// then reads accept / lambda with its prefetch instead of deciding on one thread behind it.
// With prm.commit_in_reduce each pair block first copies its staged entries to the committed system
// when the previous trial was accepted (before this trial overwrites them; an evaluate-only trial
// copies and writes nothing): a controller that factors a large system then never copies it.
__global__ __launch_bounds__(RT) void k_reduce(const double* __restrict__ rows, const double* __restrict__ csc,
                                               const uint4* __restrict__ red_tab, int nred,
                                               lh_ctrl* __restrict__ ctrl, double* __restrict__ rs,
                                               double* __restrict__ rs_commit, double* __restrict__ maxd_out,
                                               lh_params prm, int n_chunks, int mode, volatile int* __restrict__ host_done,
                                               int seq, double* __restrict__ img) {
    STAMP_DECL
    __shared__ double part[3][RW][64];
    const lh_rs_layout LY = lh_rs_make(prm.P, prm.npairs);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the stop flag and this block's pair words (one 16-byte entry of the host's table: the pairs some chunk
    // reaches, then the scalar block's sentinel {npairs, 0, 0, 0}) are independent loads: one round trip
    const uint4 rt = red_tab[min((int)blockIdx.x, nred)];
    const int b = (int)blockIdx.x < nred ? (int)rt.x : LY.npairs;
    const int ib = (int)rt.y, ie = (int)rt.z;
    const int p = (int)(rt.w & 0xffffu), q = (int)(rt.w >> 16);
    const int done = __builtin_amdgcn_readfirstlane(ctrl->done);
    // k_lin wrote the chunk scalars only (this trial's word: the scalar block's decision writes the next one's)
    // this chain's evo word (evo, and above it a batch's rung count: k_lin evaluated rungs lad .. lad + nb - 1, their
    // chunk scalars at csc + r n_chunks 4)
    const int evo = mode != 0 ? __builtin_amdgcn_readfirstlane(ctrl->evo_seq[seq & 1]) : 0;
    const int nb = max(evo >> 8, 1);
    const bool copy_prev = (prm.commit_in_reduce | prm.img) && mode != 0 && b < LY.npairs && done == 0 && wave == 0;
    const int prev_acc = copy_prev ? __builtin_amdgcn_readfirstlane(ctrl->acc_hist[(seq - 1) & 1]) : 0;
    if (copy_prev) {
        if (prev_acc) {
            if (prm.img) {   // this pair's entries of k_ctrl's image (their slots below), then the rhs row's
                if (lane < 36) {
                    const int ea_ = lane / 6, eb_ = lane - 6 * (lane / 6), gi = 6 * p + ea_, gj = 6 * q + eb_;
                    const int idx = (p < q) ? gj * LH_IMG_AS + gi : ((ea_ >= eb_) ? gi * LH_IMG_AS + gj : -1);
                    if (idx >= 0) st_red(img + LH_IMG_SZ + idx, img[idx]);
                } else if (p == q && lane < 42) {
                    const int idx = LH_NPAD * LH_IMG_AS + 6 * p + (lane - 36);
                    st_red(img + LH_IMG_SZ + idx, img[idx]);
                }
            } else if (prm.bimg) {   // this pair's entries of k_ctrl_b's band image
                const int bsz = ((6 * prm.P + 15) >> 4) * LH_BIMG_TR;
                if (lane < 36) {
                    const int ea_ = lane / 6, eb_ = lane - 6 * (lane / 6), gi = 6 * p + ea_, gj = 6 * q + eb_;
                    const int r_ = (p < q) ? gj : gi, c_ = (p < q) ? gi : gj;
                    if ((p < q || ea_ >= eb_) && lh_bimg_in(r_, c_)) st_red(img + bsz + lh_bimg_idx(r_, c_), img[lh_bimg_idx(r_, c_)]);
                }
            } else if (lane < 36) {
                st_red(rs_commit + LY.off_S + b * 36 + lane, rs[LY.off_S + b * 36 + lane]);
            }
            if (p == q && lane >= 36 && lane < 54) {
                const int k = lane - 36, part_off = (k < 6) ? LY.off_bs : (k < 12) ? LY.off_bp : LY.off_hd;
                const int i = part_off + 6 * p + (k % 6);
                st_red(rs_commit + i, rs[i]);
            }
        }
    }
    // An evaluate-only trial writes no system, and if it is rejected its controller factors the committed one:
    // k_ctrl's image path loads the staged image before the decision is known, so this pair's committed
    // entries (image slots, rhs row, b_s, b_p, diag H_pp) are copied to the staged side here, and that
    // controller then needs no second load after a rejection.  After an accepted trial the copy above has
    // just made the two sides equal, and this one is skipped.
    if (prm.img && evo && !prev_acc && b < LY.npairs && done == 0 && wave == 0) {
        if (lane < 36) {
            const int ea_ = lane / 6, eb_ = lane - 6 * (lane / 6), gi = 6 * p + ea_, gj = 6 * q + eb_;
            const int idx = (p < q) ? gj * LH_IMG_AS + gi : ((ea_ >= eb_) ? gi * LH_IMG_AS + gj : -1);
            if (idx >= 0) st_red(img + idx, img[LH_IMG_SZ + idx]);
        } else if (p == q && lane < 42) {
            const int idx = LH_NPAD * LH_IMG_AS + 6 * p + (lane - 36);
            st_red(img + idx, img[LH_IMG_SZ + idx]);
        }
        if (p == q && lane >= 36 && lane < 54) {
            const int k = lane - 36, part_off = (k < 6) ? LY.off_bs : (k < 12) ? LY.off_bp : LY.off_hd;
            const int i = part_off + 6 * p + (k % 6);
            st_red(rs + i, rs_commit[i]);
        }
    }
    // (p > q and ib > ie never hold: they make the exit test need the pair words, so the compiler issues
    // them with the controller's instead of sinking them below the branch, a second round trip)
    if ((done != 0) | ((evo != 0) & (b < LY.npairs)) | (p > q) | (ib > ie)) return;   // no short-circuit: one test
    if (b == LY.npairs) {
        // the LM decision's controller words go out with the chunk scalars (one round trip, not a third
        // after the sums; only this block's thread 0 writes them in this kernel)
        CtrlWords cw0{};
        BatchWords bw0;
        __shared__ double b_sp[LH_LAD];
        __shared__ int b_its[LH_LAD], b_cnt[4];
        if (prm.dec_in_reduce && mode != 0 && tid == 0) {
            if (nb > 1) batch_load(ctrl, bw0, b_sp, b_its, b_cnt);
            else cw0 = ctrl_load(ctrl);
        }
        if (nb > 1) {
            // each rung's chi2 and gain-scale sums in the order below (thread, lane butterfly, waves in order):
            // ten rungs (a default ladder's batch) per round of loads, the butterflies in VALU (wave_sum_desc)
            constexpr int BG = 10;
            for (int g = 0; g < nb; g += BG) {
                double b[2 * BG];
#pragma unroll
                for (int j = 0; j < 2 * BG; ++j) b[j] = 0.0;
                for (int c = tid; c < n_chunks; c += RT) {
#pragma unroll
                    for (int j = 0; j < BG; ++j)
                        if (g + j < nb) {
                            const double* sc = csc + ((size_t)(g + j) * n_chunks + c) * 4;
                            b[2 * j] += sc[0]; b[2 * j + 1] += sc[1];
                        }
                }
                wave_sum_desc(b);
                if (lane == 0)
#pragma unroll
                    for (int j = 0; j < 2 * BG; ++j)
                        if (2 * g + j < 2 * nb) part[0][wave][2 * g + j] = b[j];
            }
            lds_barrier();
            // each rung's totals over the waves, in wave order, by one thread per rung: into LDS for the decisions
            // here (one rank), and behind the system (off_bsc) for the exchange and a controller that decides
            __shared__ double b_a[2 * LH_LAD];
            if (tid < nb) {
                double a0 = 0.0, a1 = 0.0;
                for (int wv = 0; wv < RW; ++wv) { a0 += part[0][wv][2 * tid]; a1 += part[0][wv][2 * tid + 1]; }
                b_a[2 * tid] = a0;
                b_a[2 * tid + 1] = a1;
                rs[LY.off_bsc + 2 * tid] = a0;
                rs[LY.off_bsc + 2 * tid + 1] = a1;
            }
            if (tid == 0) {
                rs[LY.off_sc + LH_SC_CHI2] = 0.0; rs[LY.off_sc + LH_SC_SCALE] = 0.0;
                rs[LY.off_sc + LH_SC_NDEG] = 0.0; rs[LY.off_sc + LH_SC_MAXD] = 0.0;
                *maxd_out = 0.0;
            }
            lds_barrier();
            if (prm.dec_in_reduce && tid == 0) {
                int d_o, a_o, c_o;
                double l_o;
                ctrl_batch_decide(ctrl, bw0, prm, b_a, nb, host_done, seq, false, d_o, a_o, c_o, l_o);
            }
            return;
        }
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, mx = 0.0;
        for (int c = tid; c < n_chunks; c += RT) {
            const double* sc = csc + (size_t)c * 4;
            s0 += sc[0]; s1 += sc[1]; s2 += sc[2]; mx = fmax(mx, sc[3]);
        }
        for (int off = 32; off > 0; off >>= 1) {
            s0 += __shfl_xor(s0, off); s1 += __shfl_xor(s1, off); s2 += __shfl_xor(s2, off);
            mx = fmax(mx, __shfl_xor(mx, off));
        }
        if (lane == 0) { part[0][wave][0] = s0; part[1][wave][0] = s1; part[2][wave][0] = s2; part[0][wave][1] = mx; }
        lds_barrier();
        if (tid == 0) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, m = 0.0;
            for (int w = 0; w < RW; ++w) { a0 += part[0][w][0]; a1 += part[1][w][0]; a2 += part[2][w][0]; m = fmax(m, part[0][w][1]); }
            rs[LY.off_sc + LH_SC_CHI2] = a0;
            rs[LY.off_sc + LH_SC_SCALE] = a1;
            rs[LY.off_sc + LH_SC_NDEG] = a2;
            rs[LY.off_sc + LH_SC_MAXD] = m;
            *maxd_out = m;
            if (prm.dec_in_reduce && mode != 0) {
                int d_o, a_o, c_o;
                double l_o;
                ctrl_lm_step(ctrl, cw0, prm, 1, 0.0, 0.5 * a0, a1, a2, host_done, seq, d_o, a_o, c_o, l_o, false);
            }
        }
        return;
    }
    const bool diag = p == q;
    const int a = lane / 6, bb = lane - 6 * (lane / 6);
    // lanes 0..35: S entry (a, bb) [+ H_pp entry on the diagonal]; 36..41: b_p; 42..47: bsd
    int off_h = 0;
    if (lane < 36) off_h = 36 + (diag ? hpp_index(a < bb ? a : bb, a < bb ? bb : a) : 0);
    else if (lane < 42) off_h = 36 + 21 + (lane - 36);
    else if (lane < 48) off_h = 36 + 27 + (lane - 42);
    const bool act_s = lane < 36, act_h = (lane < 36 && diag) || (lane >= 36 && lane < 48 && diag);
    // Each wave walks its rows (wave, wave + RW, ...) in order, eight at a time; the addresses
    // follow from the pair's row range alone, so every load of the pair is in flight together.
    double vs = 0.0, vh = 0.0;
    const int w_u = __builtin_amdgcn_readfirstlane(wave);
    // 24 rows per wave per round: a C3 diagonal pair's ~300 rows arrive in one round trip (8 took three:
    // 6.67 -> 6.44 us per launch; 16 took two and measured 7.2, its doubled loads per round slower)
    constexpr int LH_RED_ROWS = 24;
    for (int base = ib + w_u; base < ie; base += LH_RED_ROWS * RW) {
        double x[LH_RED_ROWS], y[LH_RED_ROWS];
#pragma unroll
        for (int u = 0; u < LH_RED_ROWS; ++u) {
            const int it = base + u * RW;
            const bool in = it < ie;
            const double* row = rows + (size_t)(in ? it : ib) * LH_ROW;
            x[u] = (in && act_s) ? row[lane] : 0.0;
            y[u] = (in && act_h) ? row[off_h] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < LH_RED_ROWS; ++u) { vs += x[u]; vh += y[u]; }
    }
    part[0][wave][lane] = vs;
    part[1][wave][lane] = vh;
    lds_barrier();
    if (wave == 0) {
        double s = 0.0, h = 0.0;
        for (int w = 0; w < RW; ++w) { s += part[0][w][lane]; h += part[1][w][lane]; }
        if (lane < 36) {
            const double v = (diag ? h : 0.0) - s;
            if (prm.img) {
                // k_ctrl's LDS layout (prm.img): entry (a, bb) of block (p, q) is S(6p + a, 6q + bb); its lower
                // slot only (the upper triangle stays zero in the image, where the factor writes L^T)
                const int gi = 6 * p + a, gj = 6 * q + bb;
                if (p < q) st_red(img + gj * LH_IMG_AS + gi, v);
                else if (a >= bb) st_red(img + gi * LH_IMG_AS + gj, v);
            } else if (prm.bimg) {
                // k_ctrl_b's band image (prm.bimg): the lower slot, (row, column) = (6q + bb, 6p + a) for p < q
                const int gi = 6 * p + a, gj = 6 * q + bb, r_ = (p < q) ? gj : gi, c_ = (p < q) ? gi : gj;
                if ((p < q || a >= bb) && lh_bimg_in(r_, c_)) st_red(img + lh_bimg_idx(r_, c_), v);
            } else {
                st_red(rs + LY.off_S + b * 36 + lane, v);
            }
            if (diag && a == bb) st_red(rs + LY.off_hd + 6 * p + a, h);
        }
        // b_p (lanes 36..41) and bs = b_p - bsd (needs lane + 6)
        const double bsd = __shfl_down(h, 6);
        if (diag && lane >= 36 && lane < 42) {
            st_red(rs + LY.off_bp + 6 * p + (lane - 36), h);
            st_red(rs + LY.off_bs + 6 * p + (lane - 36), h - bsd);
            if (prm.img) st_red(img + LH_NPAD * LH_IMG_AS + 6 * p + (lane - 36), h - bsd);   // the rhs row
        }
    }
    STAMP(20);
    STAMP_FLUSH(20, 1);
}

// ============================================================================
// k_ctrl: LM controller + reduced-system solve, one workgroup of 1024 threads (16 waves: the
// LDLT's trailing updates are latency-bound MFMA chains, four waves per SIMD overlap them).
//
//  1. one global round trip: every thread prefetches its slice of the staged reduced system and
//     the LM decision k_reduce took (one rank: prm.dec_in_reduce); otherwise thread 0 runs
//     isGoodStepInLM behind the prefetch (the initial linearisation, sharded solves);
//  2. the chosen system (the committed one on a rejection) is scattered straight from registers
//     into LDS in natural pose order, lambda on the diagonal (problem.cpp:408-418), committing it on
//     accept.  The solve is LDL^T without pivoting: S + lambda D is symmetric positive
//     (semi)definite, where Eigen's LDLT (problem.cpp:420) pivots on the largest diagonal; the two
//     agree to rounding (a zero pivot -- a fixed pose under STRATEGY1 -- is skipped as Eigen's
//     pivot_is_valid does, and its component solved as 0);
//  3. right-looking blocked LDL^T (8-column blocks, one barrier per block) over the envelope of S
//     only (lh_ctrl_units), see lds_ldlt_solve; the right-hand side rides along as row NP;
//  4. blocked back substitution in one wave; the step and the gain's pose part.
// The matrix is padded to NE = ceil16(n) with identity rows: no bounds tests in the inner loops.
// ============================================================================
// k_ctrl's prefetch of the staged reduced system (the layout, CT threads and the solves: lh_ldlt.h)
constexpr int RS_MAX = LH_PMAX * (LH_PMAX + 1) / 2 * 36 + 18 * LH_PMAX + 8;
constexpr int ER = 1008;      // reduced-system elements per prefetch round: 28 whole 6x6 S blocks
constexpr int NLD = (RS_MAX + ER - 1) / ER;

template <int SOLVER, bool IMG>
__global__ __launch_bounds__(CT) void k_ctrl(lh_ctrl* __restrict__ ctrl, double* __restrict__ rs_commit,
                                             const double* __restrict__ rs_stage, const double* __restrict__ maxd_in,
                                             const uint16_t* __restrict__ pair_pq, const uint16_t* __restrict__ units,
                                             double* __restrict__ dxp, lh_params prm, int mode /* 0 init, 1 trial */,
                                             volatile int* __restrict__ host_done, int seq, double* __restrict__ img) {
    // S + lambda D (lower); L^T above, D in place; row NP = rhs -> z / D
    __shared__ __attribute__((aligned(16))) double A[(NP + 1) * AS];
    __shared__ __attribute__((aligned(16))) double dg[NP];   // the PCG's vector (16-byte reads)
    __shared__ double bpv[NP], hdv[NP], xs[NP];
    __shared__ uint16_t s_units[16 * LH_NSTEP];
    __shared__ int s_flags[4];
    __shared__ double s_red[CT / 64], s_lam;
    __shared__ __attribute__((aligned(16))) double s_pcg[48];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = prm.P, n = 6 * P, NE = (n + 15) & ~15;
    const lh_rs_layout LY = lh_rs_make(P, prm.npairs);
    // The other controllers take the launch's decision in one call (ctrl_take_decision).  This one spells the same
    // protocol out, spread through its prefetch: the system's loads and wave 0's early block-0 factor overlap the
    // decision's reads, and at 1024 threads on 128 VGPRs small changes to this prologue have spilled twice.
    // k_reduce took this trial's LM decision; a rung workgroup > 0 reads it (or workgroup 0's) from lh_ctrl
    const int rung = (int)blockIdx.x;
    const bool dec_src = mode != 0 && prm.dec_in_reduce;
    // A batch chain of a controller that decides itself (sharded: after the exchange) is decided by the launch's
    // last workgroup (lh_launch_ctrl adds it), and every other workgroup, 0 included, waits for that decision
    // (this chain's evo word: no decision has rewritten it yet)
    const int nwg = prm.ladder > 1 ? prm.ladder : 1;
    const bool dwg = !dec_src && mode != 0;   // the decider workgroup decides this chain
    if (!prm.dec_in_reduce && rung == nwg) {
        if (dwg && threadIdx.x == 0)
            ctrl_decider(ctrl, prm, rs_stage, LY, __builtin_amdgcn_readfirstlane(ctrl->evo) >> 8, host_done, seq);
        return;
    }
    const bool decided = dec_src || rung > 0 || dwg;
    const bool nd = SOLVER == 0 && prm.nd_steps > 0;        // the two-chain LDL^T schedule
    // k_reduce wrote S and b_s in this kernel's LDS layout (img[0] staged, img[1] committed): the system
    // arrives by a straight copy, no index math per entry (the scatter below was 2.2 us of wave 0's time)
    constexpr bool imgp = IMG;   // (the host sets prm.img only for SOLVER 0 without the two-chain schedule)
    static_assert(AS == LH_IMG_AS && (NP + 1) * AS == LH_IMG_SZ && LH_IMG_SZ % 2 == 0, "k_reduce's image layout");
    // the image is copied by waves 1-15 (wave 0 factors block 0 meanwhile): copy thread ctid = tid - 64 takes the
    // double pairs ctid + CW u
    constexpr int CW = CT - 64, IMG2 = LH_IMG_SZ / 2, NIMG = (IMG2 + CW - 1) / CW;
    const int ctid = tid - 64;
    const bool cpw = tid >= 64;
    CSTAMP_START;
#ifdef LH_STAMPS
    // [160 + wave]: the wave's HW_ID word (SIMD in bits 5:4): which waves share wave 0's SIMD
    if (lane == 0) lh_stamps[160 + wave] = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4) | (1ull << 32);
#endif

    // ---------------- 1. prefetch (one round trip) ----------------
    double tchi = 0.0, sl = 0.0, ndg = 0.0;
    CtrlWords cw{};
    if (!decided && tid == 0) {
        cw = ctrl_load(ctrl);
        tchi = 0.5 * rs_stage[LY.off_sc + LH_SC_CHI2];
        sl = rs_stage[LY.off_sc + LH_SC_SCALE];
        ndg = rs_stage[LY.off_sc + LH_SC_NDEG];
    }
    // the decision's words: uniform loads in the same round trip as the system
    int done = 0, accept = 0, skip = 0;
    double lambda = 0.0;
    int dseq = -1;
    bool staged_is_commit = false;   // an evaluate-only trial: k_reduce copied the committed system to the staged side
    // workgroup `rung` > 0 of a ladder launch: the same system at the lambda of the rung-th rejection
#ifdef LH_STAMPS
    if (rung) return;   // (the diagnostic build times one controller)
#endif
    // (the initial linearisation's controller builds no ladder: its release on workgroup 0's path cost ~5 us per
    // solve, and a rejection right after it refactors and builds one)
    if (rung && mode == 0) return;
    // the decider workgroup decides and publishes (workgroup 0's thread 0 below decides the initial linearisation)
    if (dwg) ladder_wait(ctrl, seq);
    if (decided) {
        const LadderDec d = ladder_read(ctrl, prm, seq, rung);   // (the rung's lambda: block 0's early factor uses it)
        done = d.done;
        accept = d.accept;
        skip = d.skip;
        lambda = d.lambda;
        dseq = __builtin_amdgcn_readfirstlane(ctrl->done_seq);
        staged_is_commit = imgp && __builtin_amdgcn_readfirstlane(ctrl->evo_seq[seq & 1]) != 0;
    }
    // Round u covers elements [ER u, ER u + ER), thread t < ER element ER u + t (coalesced): its entry
    // (ea, eb) of a 6x6 S block is the same in every round and its block advances by 28, so the
    // element's rows need only the block's pose pair (p | q << 16, from the 840-byte pair table).
    // Only the staged system is loaded here: a trial is accepted far more often than not, and a
    // rejected one loads the committed system after the decision (one more round trip).
    const uint32_t* __restrict__ pqw = reinterpret_cast<const uint32_t*>(pair_pq);
    const int e36 = tid % 36, ea = e36 / 6, eb = e36 - 6 * ea, blk0 = tid / 36;
    const int ibase = (tid < ER) ? tid : (1 << 30);   // threads past ER hold no element
    double vs[NLD];
    uint32_t mp[NLD];
    double2 iv[NIMG];                   // imgp: this copy thread's double pairs ctid + CW u of the image
    double bpx = 0.0, hdx = 0.0;        // imgp: b_p and diag H_pp of row tid (the packed buffer)
    const double2* __restrict__ img2 = reinterpret_cast<const double2*>(img);
    // only the pairs that carry data are read (the lower triangle of the real rows and the rhs row: ~45 % of the
    // image at C3); the rest are zeros or the identity padding, written without a load (img_need, img_fill)
    auto img_need = [&](int k) {
        const int e = 2 * k, row = e / AS, col = e - AS * row;
        return k < IMG2 && ((row < n && col <= row) || (row == NP && col < n));
    };
    auto img_fill = [&](int k) {
        const int e = 2 * k, row = e / AS, col = e - AS * row;
        const bool pad = row >= n && row < NE;   // as k_img_init: identity on rows [n, NE)
        return double2{(pad && col == row) ? 1.0 : 0.0, (pad && col + 1 == row) ? 1.0 : 0.0};
    };
    if constexpr (imgp) {
        bpx = rs_stage[LY.off_bp + min(tid, n - 1)];
        hdx = rs_stage[LY.off_hd + min(tid, n - 1)];
    } else {
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = u * ER + ibase;
            vs[u] = (i < LY.total) ? rs_stage[i] : 0.0;
            mp[u] = pqw[min(blk0 + (ER / 36) * u, max(LY.npairs - 1, 0))];
        }
    }
    uint32_t unit2 = 0;   // two unit words per thread (SOLVER 0)
    if (SOLVER == 0 && tid < 8 * LH_NSTEP) unit2 = reinterpret_cast<const uint32_t*>(units)[tid];
    // The one-chain LDL^T's first block (rows 0-7: pose 0 and two rows of pose 1) is factored by wave 0
    // while the other waves scatter: its row r = lane & 7 comes straight from the packed pair blocks
    // (pairs (0, 0), (0, 1), (1, 1) at indices 0, 1, P: every pair is listed for P <= LH_PMAX), staged
    // and committed, selected once the decision is known; the scatter leaves block 0 alone.
    const bool early0 = SOLVER == 0 && !(prm.nd_steps > 0) && n >= 8;
    double b0s[8], b0c[8];
    if (imgp && early0 && wave == 0) {   // rows 0-7 of the staged image (the upper entries are zeros, unused)
        const int r = lane & 7;
#pragma unroll
        for (int q = 0; q < 8; ++q) b0s[q] = img[r * AS + q];
    } else if (!imgp && early0 && wave == 0) {
        const int r = lane & 7;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            int i;
            if (r < 6 && q < 6) i = 6 * r + q;                           // pair (0, 0)
            else if (r >= 6 && q < 6) i = 36 + 6 * q + (r - 6);           // pair (0, 1): S(6 + eb, ea)
            else if (r < 6) i = 36 + 6 * r + (q - 6);                    // (upper, unused)
            else i = 36 * P + 6 * (r - 6) + (q - 6);                     // pair (1, 1)
            b0s[q] = rs_stage[i];
            b0c[q] = rs_commit[i];
        }
    }

    // imgp: the staged image goes into LDS as it arrives, before the decision is known (a trial is accepted
    // far more often than not; a rejected one overwrites it with the committed image); block 0 is wave 0's
    // (a macro, not a lambda: a captured array would live in scratch memory)
#define LH_IMG_TO_LDS()                                                                                        \
    do {                                                                                                       \
        double2* A2_ = reinterpret_cast<double2*>(A);                                                          \
        if (cpw) _Pragma("unroll") for (int u = 0; u < NIMG; ++u) {                                            \
            const int k = ctid + CW * u, e = 2 * k, row = e / AS, col = e - AS * row; /* AS even: no straddle */\
            if (k < IMG2 && !(early0 && row < 8 && col < 8)) A2_[k] = img_need(k) ? iv[u] : img_fill(k);      \
        }                                                                                                      \
    } while (0)
    // imgp with k_reduce's decision known: wave 0 factors block 0 first, while the image is still in flight (its
    // rows come in their own loads, b0s; the image copy leaves block 0 alone), then copies its share
    bool f0_done = false;
    if constexpr (imgp) {
    if (cpw) {   // wave-uniform: the copy waves' image loads and copy, apart from wave 0's factor (registers)
#pragma unroll
        for (int u = 0; u < NIMG; ++u) iv[u] = img2[img_need(ctid + CW * u) ? ctid + CW * u : 0];
        LH_IMG_TO_LDS();
    }
#ifndef LH_NO_F0_FIRST
    else if (early0 && decided && !done && !skip) {
        if (!accept && !staged_is_commit) {   // a rejected trial factors the committed block 0
            const int r = lane & 7;
#pragma unroll
            for (int q = 0; q < 8; ++q) b0s[q] = img[LH_IMG_SZ + r * AS + q];
        }
        const int r = lane & 7;
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            double x = b0s[q];
            if (q == r) x = (prm.strategy == 0) ? x + lambda : x + lambda * x;
            v[q] = x;
        }
        LdltBlockLds& F0 = ldlt_lds();
        factor_block8_v(LdsSys{A}, v, F0.N[0], F0.ND[0], 0, lane);
        f0_done = true;
    }
#endif
    }

    if (!decided) {   // (only the initial linearisation, mode 0, on workgroup 0)
        // max |diag H_pp| for computeLambdaInitLM (problem.cpp:486-496)
        double mx = 0.0;
        if constexpr (imgp) {
            if (tid < n) mx = fabs(hdx);
        } else {
#pragma unroll
            for (int u = 0; u < NLD; ++u) {
                const int i = u * ER + ibase;
                if (i >= LY.off_hd && i < LY.off_hd + n) mx = fmax(mx, fabs(vs[u]));
            }
        }
        for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
        if (lane == 0) s_red[wave] = mx;
        lds_barrier();
        // ---------------- LM bookkeeping (thread 0) ----------------
        if (tid == 0) {
            double mdiag = 0.0;
            for (int w = 0; w < CT / 64; ++w) mdiag = fmax(mdiag, s_red[w]);
            mdiag = fmax(*maxd_in, mdiag);
            int d_o, a_o, c_o;
            double lam_n;
            // (only the initial linearisation's: a later chain's is the decider workgroup's)
            s_flags[2] = ctrl_lm_step(ctrl, cw, prm, 0, mdiag, tchi, sl, ndg, host_done, seq, d_o, a_o, c_o, lam_n);
            s_flags[0] = d_o;
            s_flags[1] = a_o;
            s_lam = lam_n;
        }
        lds_barrier();
        done = s_flags[0];
        accept = s_flags[1];
        skip = s_flags[2];
        lambda = s_lam;
    }
    // this trial's k_reduce stopped the loop: the summary goes to the host and done is raised here
    if (dec_src && done && dseq == seq && tid == 0 && host_done && rung == 0) publish_stop(ctrl, host_done);
    if (done || skip) return;
    // the ladder: a factor builds prm.ladder rungs (every factor, or with ladder_eager off only one after a
    // rejection); rung r factors at the lambda r more rejections set, by ctrl_lm_step's own updates in its order
    const bool build = mode != 0 && ladder_build(prm, accept);
    if (rung != 0 && (!build || rung >= prm.ladder)) return;
    if (rung == 0 && tid == 0) ctrl->lad_n = build ? prm.ladder : 1;
    dxp += (size_t)rung * n;
    CSTAMP_LIVE();
    CSTAMP(1);
#ifdef LH_STAMPS
    if (tid == 0) __builtin_amdgcn_s_waitcnt(0);   // (diagnostic) thread 0's staged-system loads have arrived
#endif
    CSTAMP(2);

    // ---------------- 2. commit, diag + lambda, scatter into LDS (natural order) ----------------
    if constexpr (imgp) {
        // The image: a straight copy (16-byte LDS stores at consecutive addresses, issued above), lambda
        // added on the diagonal of the real rows by the thread that stored it (the identity padding and the
        // zero upper triangle come with the image).  k_reduce commits an accepted system to img[1] before
        // the next trial overwrites img[0] (commit_in_reduce's role), so nothing here copies S.  After an
        // evaluate-only trial the staged side already holds the committed system (k_reduce), so no reload.
        if (!accept && !staged_is_commit) {
            const double2* __restrict__ imgc2 = reinterpret_cast<const double2*>(img + LH_IMG_SZ);
#pragma unroll
            for (int u = 0; u < NIMG; ++u) iv[u] = imgc2[(cpw && img_need(ctid + CW * u)) ? ctid + CW * u : 0];
            bpx = rs_commit[LY.off_bp + min(tid, n - 1)];
            hdx = rs_commit[LY.off_hd + min(tid, n - 1)];
            if (early0 && wave == 0 && !f0_done) {
                const int r = lane & 7;
#pragma unroll
                for (int q = 0; q < 8; ++q) b0s[q] = img[LH_IMG_SZ + r * AS + q];
            }
            LH_IMG_TO_LDS();
        }
#undef LH_IMG_TO_LDS
#pragma unroll
        for (int u = 0; u < NIMG; ++u) {
            const int k = ctid + CW * u, e = 2 * k, row = e / AS, col = e - AS * row;
            if (cpw && k < IMG2 && row < n && (col == row || col + 1 == row) && !(early0 && row < 8)) {
                double& d = A[row * AS + row];
                d = (prm.strategy == 0) ? d + lambda : d + lambda * d;
            }
        }
        if (tid < n) {
            bpv[tid] = bpx;
            hdv[tid] = hdx;
        }
    } else {
    if (!accept) {   // rollback: the committed system, with the new lambda
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = u * ER + ibase;
            vs[u] = (i < LY.total) ? rs_commit[i] : 0.0;
        }
    }
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
        const int i = u * ER + ibase;
        const double v = vs[u];
        if (accept && rung == 0 && i < LY.total) rs_commit[i] = v;
        if (i < LY.off_bs) {
            // S element i: pose pair (p, q), p <= q, entry (ea, eb) -> rows 6 p + ea, 6 q + eb.  The
            // upper slot of every off-diagonal entry is zeroed: the factor stores L^T there where the
            // envelope reaches, and the back substitution reads zeros elsewhere.
            int pp = (int)(mp[u] & 0xffffu), qq = (int)(mp[u] >> 16);
            if (nd) {
                pp = lh_nd_pos(pp, P, prm.nd_a, prm.nd_s, prm.nd_long_first);
                qq = lh_nd_pos(qq, P, prm.nd_a, prm.nd_s, prm.nd_long_first);
            }
            const int gi = 6 * pp + ea, gj = 6 * qq + eb;
            const int hi = max(gi, gj), lo = min(gi, gj);
            if (early0 && hi < 8) {
                // block 0: wave 0's
            } else if (gi == gj) {
                A[gi * AS + gi] = (prm.strategy == 0) ? v + lambda : v + lambda * v;
            } else if (pp != qq || gi > gj) {
                A[hi * AS + lo] = v;
                A[lo * AS + hi] = 0.0;
            }
        } else if (i < LY.off_bp) {
            int r = i - LY.off_bs;
            if (nd) r = 6 * lh_nd_pos(r / 6, P, prm.nd_a, prm.nd_s, prm.nd_long_first) + r % 6;
            A[NP * AS + r] = v;
        } else if (i < LY.off_hd) {
            bpv[i - LY.off_bp] = v;
        } else if (i < LY.off_hd + n) {
            hdv[i - LY.off_hd] = v;
        }
    }
    if (tid >= n && tid < NE) {   // identity padding rows
        A[tid * AS + tid] = 1.0;
        A[NP * AS + tid] = 0.0;
    }
    for (int x = tid; x < (NE - n) * NE; x += CT) {
        const int r = n + x / NE, c = x - NE * (x / NE);
        if (c < r) {
            A[r * AS + c] = 0.0;
            A[c * AS + r] = 0.0;
        }
    }
    }   // packed path
    if (SOLVER == 0 && tid < 8 * LH_NSTEP) reinterpret_cast<uint32_t*>(s_units)[tid] = unit2;
    CSTAMP(3);
    if (early0 && wave == 0 && !f0_done) {
        const int r = lane & 7;
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            double x = (imgp || accept) ? b0s[q] : b0c[q];
            if (q == r) x = (prm.strategy == 0) ? x + lambda : x + lambda * x;
            v[q] = x;
        }
        LdltBlockLds& F = ldlt_lds();
        factor_block8_v(LdsSys{A}, v, F.N[0], F.ND[0], 0, lane);
    }
    lds_barrier();
    CSTAMP(4);

    // ---------------- 3-4. blocked LDL^T with the forward substitution in row NP; back substitution ----------------
    if constexpr (SOLVER == 1) {
        const int its = lds_pcg_solve(A, xs, dg, s_pcg, n, tid, prm.pcg_tol, (prm.pcg_max_it > 0 ? prm.pcg_max_it : 2 * n) + 1);
        if (tid == 0) {
            ctrl->lad_its[rung] = its;
            if (rung == 0) ctrl->pcg_iters += its;   // a higher rung's count is added when a rejection uses it
        }
    } else {
        if (nd) lds_ldlt_solve_nd(A, xs, n, tid, s_units, prm);
        else lds_ldlt_solve(A, xs, n, NE, tid, nullptr, s_units, LdltTail{ctrl, dxp, bpv, hdv, lambda, prm.strategy, rung},
                            early0);
    }
    CSTAMP(8);

    // the one-chain LDL^T took the tail in its back-substitution wave
    if (SOLVER == 1 || nd) ctrl_step_tail<CT>(ctrl, prm, n, lambda, xs, bpv, hdv, s_red, dxp, rung);
    CSTAMP(12);
    CSTAMP_END();
}

#include "lh_ctrl_g.hip"
#include "lh_ctrl_b.hip"
#include "lh_ctrl_p.hip"

// ============================================================================
// launchers (host side)
// ============================================================================
extern "C" {

hipError_t lh_launch_reduce(hipStream_t st, const double* rows, const double* csc, const uint32_t* red_tab, int nred,
                            lh_ctrl* ctrl, double* rs_stage, double* rs_commit, double* maxd,
                            lh_params prm, int n_chunks, int mode, int* host_done, int seq, double* img) {
    hipLaunchKernelGGL(k_reduce, dim3(nred + 1), dim3(RT), 0, st, rows, csc, reinterpret_cast<const uint4*>(red_tab),
                       nred, ctrl, rs_stage, rs_commit, maxd, prm, n_chunks, mode, (volatile int*)host_done, seq, img);
    return hipGetLastError();
}

// k_ctrl's two LDS images (prm.img): zero (the upper triangle where the factor writes L^T, padding
// columns) with the identity on the padding rows [n, ne); k_reduce fills the lower triangle and the rhs
__global__ __launch_bounds__(256) void k_img_init(double* __restrict__ img, int n, int ne) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < 2 * LH_IMG_SZ; i += gridDim.x * 256) {
        const int e = i % LH_IMG_SZ, r = e / LH_IMG_AS, c = e - LH_IMG_AS * r;
        img[i] = (r == c && r >= n && r < ne) ? 1.0 : 0.0;
    }
}

hipError_t lh_launch_img_init(hipStream_t st, double* img, int n) {
    hipLaunchKernelGGL(k_img_init, dim3(64), dim3(256), 0, st, img, n, (n + 15) & ~15);
    return hipGetLastError();
}

// k_ctrl_g's dense S (the caller launches it exactly for LH_CTRL_DENSE windows)
hipError_t lh_launch_dense(hipStream_t st, const double* rs_stage, const uint16_t* pair_pq, const lh_ctrl* ctrl,
                           double* gS, int P) {
    const int NG = (6 * P + GNB - 1) & ~(GNB - 1);
    hipLaunchKernelGGL(k_dense, dim3(P * (P + 1) / 2), dim3(64), 0, st, rs_stage, pair_pq, ctrl, gS, P, NG);
    return hipGetLastError();
}

hipError_t lh_launch_ctrl(hipStream_t st, lh_ctrl* ctrl, double* rs_commit, const double* rs_stage, const double* maxd,
                          const uint32_t* rsmap, const uint16_t* pair_pq, double* dxp, lh_params prm, int mode,
                          int* host_done, int seq, double* gA, const double* gS, const int32_t* brow_ptr,
                          const uint32_t* brow_ent, const uint16_t* units, lh_band_args band, double* img, int kind) {
    const dim3 gl(prm.ladder > 1 ? prm.ladder : 1);   // one workgroup per lambda-ladder rung
    switch (kind) {   // lh_ctrl_kind, the window's solve configuration (lh_plan.h)
    case LH_CTRL_BAND:
        if (prm.band_lu)
            hipLaunchKernelGGL(k_ctrl_b<true>, gl, dim3(CT), 0, st, ctrl, rs_commit, rs_stage, maxd, band.bblk,
                               band.units, band.Lg, band.NDg, dxp, prm, mode, (volatile int*)host_done, seq, img);
        else
            hipLaunchKernelGGL(k_ctrl_b<false>, gl, dim3(CT), 0, st, ctrl, rs_commit, rs_stage, maxd, band.bblk,
                               band.units, band.Lg, band.NDg, dxp, prm, mode, (volatile int*)host_done, seq, img);
        break;
    case LH_CTRL_PCG:
        hipLaunchKernelGGL(k_ctrl_p, gl, dim3(CT), 0, st, ctrl, rs_commit, rs_stage, maxd, brow_ptr, brow_ent,
                           dxp, prm, mode, (volatile int*)host_done, seq, gA);   // gA: the PCG's row scratch
        break;
    case LH_CTRL_DENSE:
        hipLaunchKernelGGL(k_ctrl_g, gl, dim3(GT), 0, st, ctrl, rs_commit, rs_stage, maxd, rsmap,
                           dxp, prm, mode, (volatile int*)host_done, seq, gA, gS);
        break;
    case LH_CTRL_LDS: {
        // k_ctrl deciding itself: one more workgroup, the decider of batch chains (ctrl_batch_decider)
        const dim3 gk(gl.x + (prm.dec_in_reduce ? 0 : 1));
        if (prm.solver == 1)
            hipLaunchKernelGGL((k_ctrl<1, false>), gk, dim3(CT), 0, st, ctrl, rs_commit, rs_stage, maxd, pair_pq, units,
                               dxp, prm, mode, (volatile int*)host_done, seq, img);
        else if (prm.img)
            hipLaunchKernelGGL((k_ctrl<0, true>), gk, dim3(CT), 0, st, ctrl, rs_commit, rs_stage, maxd, pair_pq, units,
                               dxp, prm, mode, (volatile int*)host_done, seq, img);
        else
            hipLaunchKernelGGL((k_ctrl<0, false>), gk, dim3(CT), 0, st, ctrl, rs_commit, rs_stage, maxd, pair_pq,
                               units, dxp, prm, mode, (volatile int*)host_done, seq, img);
        break;
    }
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // extern "C"

// Why k_reduce, the four controllers and the test probes are one translation unit of several files and not several
// objects.  The compiler propagates constants into a shared helper (lds_ldlt_solve, lds_pcg_solve, g_ldlt_solve, the
// LM bookkeeping) from all of its callers in a unit before it inlines it, so which kernels are compiled together
// decides their code.  Compared per device function on the -S output (scripts/isa_same.py):
//  - where the helpers are written changes nothing: with lh_lm.h and lh_ldlt.h as headers, ctrl_step_tail moved up
//    beside the other LM helpers and BandSys down beside k_ctrl_b, every function of the unit is the same
//    instructions as when all of it was this one file;
//  - the probes apart: k_ldlt_probe and k_ldlt_g_probe, and with them k_ctrl<1, false> and k_ctrl_g, get other
//    register allocations (k_ctrl_g 241 VGPRs for 239); k_reduce likewise when apart from the controllers;
//  - k_ctrl_b apart, over the same helpers: both of its instantiations stay the same, but k_ctrl_p, left behind,
//    changes (two registers swap, two basic blocks differ; 239 VGPRs either way, nothing spills);
//  - k_ctrl_b and k_ctrl_p apart together: k_ctrl_g changes, and k_ctrl_p apart differs from both of the above.
// "The same instructions" is what lets a change of these files' layout go in without a performance argument, so the
// included files keep this order and no new object is cut from them.
#include "lh_probe.hip"
