// lh_lm.h — the LM bookkeeping k_reduce and the four controllers share (lh_kernels.hip and the files it includes):
// the controller words and a batch's, the LM step (isGoodStepInLM, computeLambdaInitLM), the lambda ladder's
// hand-off between workgroups, a controller launch's decision prologue and its step tail.
#pragma once
#include "lh_common.h"
#include "lh_dev.h"

#pragma clang fp contract(fast)

// ============================================================================
// LM bookkeeping shared by the controllers (isGoodStepInLM, computeLambdaInitLM)
// ============================================================================
struct CtrlWords {
    double chi, lam, ni, last, spose, chi0;
    int iter, fc, trials, nacc, done, cur, tl;
    int evo, relin;   // this trial only evaluated; this chain re-linearises (the previous trial was such an acceptance)
    int retrial;      // this chain re-runs a batch's accepted rung (lh_ctrl.retrial: 2 when that acceptance stopped the loop)
    int lad, lad_n;   // the rung this trial's step came from; the rungs built (lh_ctrl.lad)
};
__device__ __forceinline__ CtrlWords ctrl_load(const lh_ctrl* __restrict__ ctrl) {
    CtrlWords w;
    w.chi = ctrl->chi; w.lam = ctrl->lambda; w.ni = ctrl->ni; w.last = ctrl->last_chi;
    w.chi0 = ctrl->chi2_initial;
    w.iter = ctrl->iter; w.fc = ctrl->false_cnt; w.trials = ctrl->trials; w.nacc = ctrl->accepted;
    w.done = ctrl->done; w.cur = ctrl->cur; w.tl = ctrl->trace_len;
    w.evo = ctrl->evo; w.relin = ctrl->relin; w.retrial = ctrl->retrial;
    w.lad = ctrl->lad; w.lad_n = ctrl->lad_n;
    // every rung's gain part is loaded and the trial's selected (no load that waits on lad)
    double sp[LH_LAD];
#pragma unroll
    for (int i = 0; i < LH_LAD; ++i) sp[i] = ctrl->spose_l[i];
    w.spose = sp[0];
#pragma unroll
    for (int i = 1; i < LH_LAD; ++i) w.spose = (w.lad == i) ? sp[i] : w.spose;
    return w;
}
// A batch's decisions (k_reduce) run back to back on one thread: the controller words and the
// counters they update stay in registers between the rungs, the rungs' gain parts and PCG counts in LDS (reloading
// them from lh_ctrl after each decision cost two dependent round trips per rung); each decision still stores its
// words.
struct BatchWords {
    CtrlWords w;              // the words the next rung's decision starts from
    const double* sp;         // lh_ctrl.spose_l (an LDS copy)
    const int* lad_its;       // lh_ctrl.lad_its (an LDS copy)
    int* cnt;                 // (LDS) lh_ctrl's counters lskips, pcg_iters; the last decision's lskip
};
enum { BW_LSKIPS, BW_PCG, BW_LSKIP };
__device__ __forceinline__ void batch_load(const lh_ctrl* __restrict__ ctrl, BatchWords& b, double* sp, int* its, int* cnt) {
    b.w = ctrl_load(ctrl);
#pragma unroll
    for (int i = 0; i < LH_LAD; ++i) { sp[i] = ctrl->spose_l[i]; its[i] = ctrl->lad_its[i]; }
    b.sp = sp;
    b.lad_its = its;
    b.cnt = cnt;
    cnt[BW_LSKIPS] = ctrl->lskips;
    cnt[BW_PCG] = ctrl->pcg_iters;
    cnt[BW_LSKIP] = 0;
}
// a self-deciding controller's: the words it loaded, the rungs' arrays left in lh_ctrl (global: one load per rung)
__device__ __forceinline__ BatchWords batch_words(const lh_ctrl* __restrict__ ctrl, const CtrlWords& cw, int* cnt) {
    BatchWords b;
    b.w = cw;
    b.sp = ctrl->spose_l;
    b.lad_its = ctrl->lad_its;
    b.cnt = cnt;
    cnt[BW_LSKIPS] = ctrl->lskips;
    cnt[BW_PCG] = ctrl->pcg_iters;
    cnt[BW_LSKIP] = 0;
    return b;
}

// a batch's words after its last decision (what ctrl_lm_step stores after a decision, from the batch's registers)
__device__ __forceinline__ void batch_store(lh_ctrl* __restrict__ ctrl, const BatchWords& b, int seq) {
    const CtrlWords& o = b.w;
    ctrl->chi = o.chi; ctrl->lambda = o.lam; ctrl->ni = o.ni; ctrl->last_chi = o.last; ctrl->chi2_initial = o.chi0;
    ctrl->iter = o.iter; ctrl->false_cnt = o.fc; ctrl->trials = o.trials; ctrl->accepted = o.nacc;
    ctrl->done = o.done; ctrl->cur = o.cur; ctrl->trace_len = o.tl;
    ctrl->retrial = o.retrial;
    ctrl->lad = o.lad;
    ctrl->lskip = b.cnt[BW_LSKIP];
    ctrl->lskips = b.cnt[BW_LSKIPS];
    ctrl->pcg_iters = b.cnt[BW_PCG];
    ctrl->acc_hist[seq & 1] = 0;   // a batch commits nothing (a retrial does)
    ctrl->seq_last = seq;
    ctrl->relin = o.relin;
    ctrl->nofactor = o.relin | b.cnt[BW_LSKIP] | (o.retrial != 0 ? 1 : 0);
    ctrl->evo = o.evo;
    ctrl->evo_seq[(seq + 1) & 1] = o.evo;
}

// The stop trial's summary and trace to the host words, then done, by ONE thread behind its own
// system-scope fence.  A kernel boundary releases at agent scope only, and the trace entries were
// decided by earlier kernels on other CUs, so every word the host reads after done is stored here,
// from lh_ctrl (device memory, complete at this kernel's start or written by this thread).  The words
// are plain stores, issued back to back, and the one fence orders them all before done (volatile
// stores each waited for their own write to the host: the stop's controller took ~18 us).
__device__ __noinline__ void publish_stop(const lh_ctrl* __restrict__ ctrl, volatile int* __restrict__ host_done) {
    lh_host_words* hw = reinterpret_cast<lh_host_words*>(const_cast<int*>(host_done));
    const int tl = ctrl->trace_len, nt = tl < LH_TRACE ? tl : LH_TRACE;
    hw->iter = ctrl->iter; hw->trials = ctrl->trials; hw->accepted = ctrl->accepted; hw->trace_len = tl;
    hw->nonpd = ctrl->nonpd; hw->pcg_iters = ctrl->pcg_iters;
    hw->chi2_initial = ctrl->chi2_initial; hw->chi = ctrl->chi; hw->lambda = ctrl->lambda;
    // four entries' loads in flight (unconditional, in the array), then their stores: few registers, so that a
    // caller's live values need no saving around this call (sixteen at a time spilled k_ctrl<0, false>)
    for (int i0 = 0; i0 < nt; i0 += 4) {
        double c[4], l[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = min(i0 + j, LH_TRACE - 1);
            c[j] = ctrl->trace_chi[i];
            l[j] = ctrl->trace_lambda[i];
        }
        // (unconditional too: an entry past trace_len is never read by the host, and a store behind a branch
        // waited for the stores before it)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = min(i0 + j, LH_TRACE - 1);
            hw->trace_chi[i] = c[j];
            hw->trace_lambda[i] = l[j];
        }
    }
    __threadfence_system();
    host_done[0] = 1;
}

// The host's progress word after chain seq's decision (ctrl_lm_step; a batch's after its last rung, k_reduce):
// 2 seq + near, near = 1 when the next chain may be the last (one more completed iteration reaches max_iters, a
// stalled iteration's last rejection, or a pending retrial that stops the loop).
__device__ __forceinline__ void ctrl_progress(const lh_params& prm, volatile int* __restrict__ host_done, int seq, int iter,
                                              int fc, double last, double chi, int hold) {
    const int near = (prm.max_iters > 0 && iter + 1 >= prm.max_iters) ? 1 : 0;
    const int last_try = (fc + 1 >= prm.max_trials && last - chi < prm.stop_dchi2) ? 1 : 0;
    host_done[1] = 2 * seq + (near | last_try | hold);
}

// Returns 1 when the controller has nothing to factor: this trial was an evaluate-only one accepted outside the
// final iteration (the next chain re-linearises the accepted state, relin; that chain's decision commits the new
// linearisation like the initial one and leaves the LM state alone), a rejection whose step a lambda-ladder
// rung already holds (lskip), or a batch's acceptance (retrial).
// batch: the decision of one rung of a batch (k_reduce's loop over the rungs a chain evaluated):
// an acceptance commits nothing (the next chain re-runs the rung as a full trial, lh_ctrl.retrial, and its
// decision commits it; a stop it causes is raised by that chain), and the host word is the loop's to write.
__device__ __forceinline__ int ctrl_lm_step(lh_ctrl* __restrict__ ctrl, const CtrlWords& w, const lh_params& prm,
                                             int mode, double mdiag, double tchi, double sl, double ndg,
                                             volatile int* __restrict__ host_done, int seq, int& done_o, int& accept_o,
                                             int& cur_o, double& lam_o, bool raise_done = true, BatchWords* bw = nullptr,
                                             bool in_batch = true) {
    // (bw is always a valid pointer where the decision may be a batch's, and in_batch says whether it is one: a
    // pointer chosen at run time would keep the caller's words out of registers)
    const bool batch = bw != nullptr && in_batch;
    double chi = w.chi, lam = w.lam, ni = w.ni, last = w.last, spose = w.spose, chi0 = w.chi0;
    int iter = w.iter, fc = w.fc, trials = w.trials, nacc = w.nacc, tl = w.tl;
    int done = w.done, cur = w.cur;
    int accept = 0, trace = 0, relin = 0, retrial = 0;
    int lad = 0, lskip = 0;   // the next step's rung: 0 after any factor; a rejection moves up the ladder
    if (!done) {
        if (mode != 0 && (w.relin || w.retrial)) {
            // the re-linearisation of an evaluate-only acceptance: its records and pose tables were written
            // to the candidate side (k_lin), which becomes the committed one; lambda, chi2 and the counts
            // were updated by the acceptance.  A retrial (a batch's accepted rung as a full trial) likewise,
            // and it raises the stop that acceptance took.
            cur = 1 - cur;
            accept = 1;
            if (w.retrial == 2) done = 1;
        } else if (mode == 0) {
            // computeLambdaInitLM (problem.cpp:470-504)
            ni = 2.0;
            chi = tchi;
            chi0 = tchi;
            if (prm.strategy == 0) {
                if (!prm.lambda_given) {
                    double m = fmin(prm.lambda_cap, mdiag);
                    lam = prm.tau * m;
                } else {
                    lam = prm.lambda_init;
                }
            } else {
                lam = 1e-5;
            }
            last = 1e20;
            iter = 0; fc = 0; trials = 0; nacc = 0; tl = 0;
            ctrl->nonpd = (int)ndg;
            cur = 1 - cur;           // the initial linearisation becomes the committed one
            accept = 1;
            if (prm.max_iters <= 0) done = 1;
            else trace = 1;
        } else {
            // isGoodStepInLM (problem.cpp:520-581)
            double scale = 0.5 * (spose + sl);
            scale += 1e-10;
            const double rho = (chi - tchi) / scale;
            const bool ok = rho > 0 && isfinite(tchi);
            if (prm.strategy == 0) {
                if (ok) {
                    const double m = 2 * rho - 1;
                    double alpha = 1.0 - m * m * m;   // std::pow(2 rho - 1, 3), problem.cpp:541 (within an ulp)
                    alpha = fmin(alpha, 2.0 / 3.0);
                    lam *= fmax(1.0 / 3.0, alpha);
                    ni = 2;
                    chi = tchi;
                } else {
                    lam *= ni;
                    ni *= 2;
                }
            } else {
                if (ok) { lam = fmax(lam / 9.0, 1e-7); chi = tchi; }
                else lam = fmin(lam * 11.0, 1e7);
            }
            trials += 1;
            bool inner_end;
            if (ok) {
                nacc += 1;
                if (!batch) {
                    cur = 1 - cur;   // commit candidate landmarks, caches and poses
                    accept = 1;
                } else {
                    retrial = 1;     // the next chain linearises this rung's candidate (its step: rung w.lad)
                    lad = w.lad;
                }
                fc = 0;
                inner_end = true;
            } else {
                fc += 1;             // rollbackStates: the committed buffers are untouched
                inner_end = fc >= prm.max_trials;
                // the lambda just set is the next rung's (the ladder applied the same updates in the same order):
                // its step is already solved, so this chain's controller has nothing to factor
                if (w.lad + 1 < w.lad_n) {
                    lad = w.lad + 1;
                    lskip = 1;
                }
            }
            relin = (ok && w.evo && !batch) ? 1 : 0;   // (cleared below when the loop stops)
            if (inner_end) {
                iter += 1;
                if (last - chi < prm.stop_dchi2) done = 1;
                last = chi;
                if (!done && iter >= prm.max_iters) done = 1;
                if (!done) { fc = 0; trace = 1; }
            }
        }
        if (trace) {
            if (tl < LH_TRACE) { ctrl->trace_chi[tl] = chi; ctrl->trace_lambda[tl] = lam; }
            tl += 1;
        }
        if (retrial && done) retrial = 2;   // the stop is the retrial's to raise
        if (done) lskip = 0;
        if (done) relin = 0;
        // (a batch's rung stores its words once, after the batch's last decision: batch_store)
        if (!batch) {
            ctrl->chi = chi; ctrl->lambda = lam; ctrl->ni = ni; ctrl->last_chi = last; ctrl->chi2_initial = chi0;
            ctrl->iter = iter; ctrl->false_cnt = fc; ctrl->trials = trials; ctrl->accepted = nacc;
            ctrl->done = retrial ? 0 : done; ctrl->cur = cur; ctrl->trace_len = tl;
            ctrl->retrial = retrial;
            ctrl->rho_sel = 0;
            ctrl->lad = lad;
            ctrl->lskip = lskip;
            if (lskip) ctrl->lskips += 1;
            if (lskip && prm.solver == 1) ctrl->pcg_iters += ctrl->lad_its[lad];   // the rung's solve counts now
            ctrl->acc_hist[seq & 1] = accept;
            ctrl->seq_last = seq;
            ctrl->relin = relin;
            ctrl->nofactor = relin | lskip | (retrial != 0 ? 1 : 0);
        } else {   // (the same counts from the batch's registers)
            bw->cnt[BW_LSKIPS] += lskip;
            if (lskip && prm.solver == 1) bw->cnt[BW_PCG] += bw->lad_its[lad];
        }
        // The next trial is in the final iteration when one more completed iteration reaches max_iters.
        // Its decision then either stops the loop (accept, or the last rejection) or leads to another
        // such trial, so its candidate linearisation is never used: k_lin only evaluates (evo).  With
        // prm.eval_first a trial after a rejection in its iteration also only evaluates: a run of
        // rejections (every solve that stops on a stalled chi2 ends with max_trials of them) then pays
        // evaluations only, and an acceptance among them one re-linearisation chain (relin).
        const int near = (prm.max_iters > 0 && iter + 1 >= prm.max_iters) ? 1 : 0;
        // A retrial is a full trial (it linearises the accepted rung's candidate, as a re-linearisation does), or an
        // evaluate-only one when that acceptance stopped the loop (it then only writes the candidate, as the serial
        // evaluate-only trial that stopped the loop did)
        const int evo_n = retrial == 2 ? 1
                        : (done || relin || retrial || prm.no_evo) ? 0 : (near | ((prm.eval_first && fc > 0) ? 1 : 0));
        // the next chain evaluates a batch of rungs when it is an evaluate-only trial after a rejection onto a built
        // rung: the rungs from there up to the last built one, within the trials left in the iteration
        const int nbatch_n = (prm.batch > 1 && evo_n && fc > 0 && lskip) ? min(min(w.lad_n - lad, prm.max_trials - fc), prm.batch) : 1;
        // (the evo words: evo in the low byte, a batch's rung count above it)
        const int evw = evo_n | (nbatch_n > 1 ? nbatch_n << 8 : 0);
        if (!batch) {
            ctrl->evo = evw;
            ctrl->evo_seq[(seq + 1) & 1] = evw;
        }
        // host words: [0] the loop stopped; else [1] = 2 seq + near, the progress word: this live
        // trial's controller has decided (its k_lin and k_reduce are done), and near = 1 when one
        // more completed iteration reaches max_iters.  The host keeps the queue filled from it (one
        // trial ahead when near, so a stop by max_iters leaves nothing enqueued past it); it never
        // advances past the stop trial, which bounds how many trials (and all-reduces) any rank
        // can have enqueued.  One 32-bit store: the host never sees a torn pair.
        if (host_done && !batch) {
            if (done) {
                ctrl->done_seq = seq;
                if (raise_done) publish_stop(ctrl, host_done);   // reads back this thread's stores above
                // else the same trial's controller publishes the summary from lh_ctrl and raises done
                // (publish_stop): only stores of the thread that fences are ordered before done
            } else {
                // near also when the next trial's rejection would end its iteration at an unchanged chi2 (a
                // stalled solve's last trial: the stop rule then ends the loop), so no chain is left past it; and
                // likewise when the next chain is a batch whose last rung is such a trial
                const int hold = (nbatch_n > 1 && fc + nbatch_n >= prm.max_trials && last - chi < prm.stop_dchi2) ? 1 : 0;
                ctrl_progress(prm, host_done, seq, iter, fc, last, chi, hold);
            }
        }
        if (retrial == 2) done = 0;
        if (batch) {   // the words the next rung's decision starts from (as ctrl_load would read them back)
            CtrlWords& o = bw->w;
            o.chi = chi; o.lam = lam; o.ni = ni; o.last = last; o.chi0 = chi0;
            o.iter = iter; o.fc = fc; o.trials = trials; o.nacc = nacc; o.done = done; o.cur = cur; o.tl = tl;
            o.evo = evw; o.relin = relin; o.retrial = retrial; o.lad = lad;
            o.spose = bw->sp[lad];
            bw->cnt[BW_LSKIP] = lskip;
        }
    }
    done_o = done;
    accept_o = accept;
    cur_o = cur;
    lam_o = lam;
    // nothing to factor: an evaluate-only acceptance, a rejection onto a built rung, or a batch's acceptance
    return relin | lskip | (retrial != 0 ? 1 : 0);
}

// A batch's decisions, thread 0 of the deciding kernel (k_reduce with one rank, else the
// controller after the exchange): rung r's chi2 (not halved) and gain scale at sc[2 r], sc[2 r + 1] (summed over
// the chunks, and over the ranks when sharded, as a single trial's are), decided in order until an acceptance
// (retrial), the stop, or a next trial that is not the batch's next rung.  bw holds the words batch_load read.
//
// (1) The rungs before the first that will be accepted (or the last) are plain rejections: each only advances
// lambda and nu, the counts and the rung (ctrl_lm_step's rejection, which moves onto a built rung and, before the
// batch's last rung, never ends the iteration: nbatch <= max_trials - false_cnt).  Their gain ratios are
// independent (chi2 does not change across rejections), so they are found first and skipped forward with that
// arithmetic; ctrl_lm_step takes the decisive rung.  Returns that rung.
__device__ __forceinline__ int batch_skip_forward(BatchWords& bw, const lh_params& prm, const double* sc, int nb) {
    CtrlWords& w = bw.w;
    const double chi = w.chi;
    int j = nb - 1;
    for (int q = 0; q < nb - 1; ++q) {
        double scale = 0.5 * (bw.sp[w.lad + q] + sc[2 * q + 1]);
        scale += 1e-10;
        const double tchi = 0.5 * sc[2 * q];
        const double rho = (chi - tchi) / scale;
        if (rho > 0 && isfinite(tchi)) { j = q; break; }
    }
    for (int r = 0; r < j; ++r) {   // rung r rejected: the decision ctrl_lm_step takes for it, in its order
        if (prm.strategy == 0) { w.lam *= w.ni; w.ni *= 2; }
        else w.lam = fmin(w.lam * 11.0, 1e7);
        w.trials += 1;
        w.fc += 1;
        w.lad += 1;
        bw.cnt[BW_LSKIPS] += 1;
        if (prm.solver == 1) bw.cnt[BW_PCG] += bw.lad_its[w.lad];
    }
    w.spose = bw.sp[w.lad];
    if (j > 0) bw.cnt[BW_LSKIP] = 1;
    return j;
}
// (2) after the decisive rung r: the words stored once, the rung whose rho0 is "as last evaluated", and the host word
// (raise_done: publish the stop here, else the chain's controller does).  Returns nothing-to-factor, with
// ctrl_lm_step's outputs.
__device__ __forceinline__ int batch_finish(lh_ctrl* __restrict__ ctrl, BatchWords& bw, const lh_params& prm, int r,
                                            volatile int* __restrict__ host_done, int seq, bool raise_done, int& done_o,
                                            int& accept_o, int& cur_o, double& lam_o) {
    const CtrlWords& w = bw.w;
    batch_store(ctrl, bw, seq);
    ctrl->rho_sel = r;   // the per-edge rho0 of the last rung decided
    ctrl->nbatches += 1;
    if (w.retrial) ctrl->nretrials[w.retrial - 1] += 1;
    if (host_done) {
        if (w.done) {
            ctrl->done_seq = seq;
            if (raise_done) publish_stop(ctrl, host_done);   // else this chain's controller publishes it
        } else {
            ctrl_progress(prm, host_done, seq, w.iter, w.fc, w.last, w.chi, w.retrial == 2 ? 1 : 0);
        }
    }
    done_o = w.done;
    accept_o = 0;
    cur_o = w.cur;
    lam_o = w.lam;
    return w.relin | bw.cnt[BW_LSKIP] | (w.retrial != 0 ? 1 : 0);
}
__device__ __forceinline__ bool batch_more(const BatchWords& bw, int r, int nb) {
    const CtrlWords& w = bw.w;
    return !(r + 1 >= nb || w.done || w.retrial || !w.evo || !bw.cnt[BW_LSKIP]);
}
// k_reduce's (one rank)
__device__ __forceinline__ int ctrl_batch_decide(lh_ctrl* __restrict__ ctrl, BatchWords& bw, const lh_params& prm,
                                                 const double* sc, int nb, volatile int* __restrict__ host_done, int seq,
                                                 bool raise_done, int& done_o, int& accept_o, int& cur_o, double& lam_o) {
    int r = batch_skip_forward(bw, prm, sc, nb);
    for (;; ++r) {
        int d_o, a_o, c_o;
        double l_o;
        ctrl_lm_step(ctrl, bw.w, prm, 1, 0.0, 0.5 * sc[2 * r], sc[2 * r + 1], 0.0, host_done, seq, d_o, a_o, c_o, l_o,
                     false, &bw);
        if (!batch_more(bw, r, nb)) break;
    }
    return batch_finish(ctrl, bw, prm, r, host_done, seq, raise_done, done_o, accept_o, cur_o, lam_o);
}
// a self-deciding controller's decision (thread 0): a batch's (this chain's evo word above its low byte, the
// rungs' scalars behind the exchanged system, lh_rs_layout.off_bsc) or one trial's
__device__ __forceinline__ int ctrl_decide(lh_ctrl* __restrict__ ctrl, const CtrlWords& cw, const lh_params& prm, int mode,
                                           double mdiag, double tchi, double sl, double ndg, const double* rs_stage,
                                           const lh_rs_layout& LY, volatile int* __restrict__ host_done, int seq,
                                           int& done_o, int& accept_o, int& cur_o, double& lam_o, int* cnt) {
    const int nb = cw.evo >> 8;   // (cw.evo: this chain's evo word, read before its decision)
    if (mode != 0 && nb > 1) {
        BatchWords bw = batch_words(ctrl, cw, cnt);
        return ctrl_batch_decide(ctrl, bw, prm, rs_stage + LY.off_bsc, nb, host_done, seq, true, done_o, accept_o, cur_o,
                                 lam_o);
    }
    return ctrl_lm_step(ctrl, cw, prm, mode, mdiag, tchi, sl, ndg, host_done, seq, done_o, accept_o, cur_o, lam_o);
}
// ---- the lambda ladder's rung workgroups (lh_ctrl.lad) ----
// Workgroup 0 of a controller that takes the LM decision itself (the initial linearisation, sharded solves,
// k_ctrl_g, k_ctrl_p) publishes it: ctrl_lm_step's words, then dec_tag = seq + 1 (release).  Its rung workgroups
// wait for that tag (acquire) and read the decision from lh_ctrl like a controller after k_reduce's decision.
// Workgroups are dispatched in order, so workgroup 0 is resident whatever the rungs do: the wait ends.
__device__ __forceinline__ void ladder_publish(lh_ctrl* __restrict__ ctrl, int seq) {
    __hip_atomic_store(&ctrl->dec_tag, seq + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ladder_wait(const lh_ctrl* __restrict__ ctrl, int seq) {
    if (threadIdx.x == 0)
        while (__hip_atomic_load(&ctrl->dec_tag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != seq + 1)
            __builtin_amdgcn_s_sleep(2);
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // every wave's loads below see workgroup 0's words
}
// the decision as a rung reads it, and the rung's lambda: the updates `rung` more rejections apply to lambda and
// ni, in ctrl_lm_step's order (DEFAULT problem.cpp:550-551, STRATEGY1 :576), so each is bit-identical
struct LadderDec {
    int done, accept, skip;
    double lambda;
};
__device__ __forceinline__ LadderDec ladder_read(const lh_ctrl* __restrict__ ctrl, const lh_params& prm, int seq, int rung) {
    LadderDec d;
    d.done = __builtin_amdgcn_readfirstlane(ctrl->done);
    d.accept = __builtin_amdgcn_readfirstlane(ctrl->acc_hist[seq & 1]);
    // an evaluate-only acceptance (nothing to factor), or a rejection onto a built rung (its step is solved)
    d.skip = __builtin_amdgcn_readfirstlane(ctrl->nofactor);
    double lambda = ctrl->lambda, ni = ctrl->ni;
    for (int i = 0; i < rung; ++i) {
        if (prm.strategy == 0) { lambda *= ni; ni *= 2; }
        else lambda = fmin(lambda * 11.0, 1e7);
    }
    d.lambda = lambda;
    return d;
}
// k_ctrl's decider workgroup (the launch's last, when the controller decides itself: sharded solves): thread 0
// takes the chain's LM decision -- one trial's, or a batch's -- then publishes the tag the factoring workgroup and
// the rungs wait for (ladder_publish).  It holds no prefetched system: workgroup 0, deciding with that system in
// registers, spilled (k_ctrl<0, false>, once the decision learnt batches).
__device__ __forceinline__ void ctrl_decider(lh_ctrl* __restrict__ ctrl, const lh_params& prm, const double* rs_stage,
                                             const lh_rs_layout& LY, int nb, volatile int* __restrict__ host_done,
                                             int seq) {
    __shared__ int cnt[4];
    int d_o, a_o, c_o;
    double l_o;
    if (nb > 1) {
        BatchWords bw = batch_words(ctrl, ctrl_load(ctrl), cnt);
        ctrl_batch_decide(ctrl, bw, prm, rs_stage + LY.off_bsc, nb, host_done, seq, true, d_o, a_o, c_o, l_o);
    } else {
        const CtrlWords cw = ctrl_load(ctrl);
        ctrl_lm_step(ctrl, cw, prm, 1, 0.0, 0.5 * rs_stage[LY.off_sc + LH_SC_CHI2], rs_stage[LY.off_sc + LH_SC_SCALE],
                     rs_stage[LY.off_sc + LH_SC_NDEG], host_done, seq, d_o, a_o, c_o, l_o);
    }
    ladder_publish(ctrl, seq);
}

// a factoring controller's rung count: prm.ladder rungs at every factor (ladder_eager) or a factor after a rejection
__device__ __forceinline__ bool ladder_build(const lh_params& prm, int accept) {
    return prm.ladder > 1 && (prm.ladder_eager || !accept);
}

// ---- a controller launch's LM decision: k_ctrl_g, k_ctrl_b, k_ctrl_p (DESIGN.md 2.2a "Who decides") ----
// Every workgroup of the launch calls this first, all NT threads.  The decision is k_reduce's
// (prm.dec_in_reduce: read from lh_ctrl, in registers), workgroup 0's (a rung waits for its tag, then reads it
// the same way), or taken here by workgroup 0's thread 0 and broadcast through the kernel's CtrlDecLds.  Then
// the exits every controller shares, and the ladder's rung count.  run false: the kernel returns.  s_red: NT / 64
// doubles of the kernel's (its step tail reuses them).
struct CtrlDecLds {
    int flags[4];   // done, accept, cur, nothing to factor
    int cnt[4];     // a batch's counters (BatchWords::cnt)
    double lam;
};
struct CtrlDec {
    bool run;
    int accept, cur;
    double lambda;
};
template <int NT>
__device__ __forceinline__ CtrlDec ctrl_take_decision(lh_ctrl* __restrict__ ctrl, const lh_params& prm, int mode,
                                                      const double* __restrict__ rs_stage, const lh_rs_layout& LY,
                                                      const double* __restrict__ maxd_in,
                                                      volatile int* __restrict__ host_done, int seq, double* s_red,
                                                      CtrlDecLds& lds) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = 6 * prm.P;
    const int rung = (int)blockIdx.x;   // workgroup `rung` > 0: a lambda-ladder rung with its own factor storage
    const bool dec_src = mode != 0 && prm.dec_in_reduce;
    CtrlDec o{false, 0, 0, 0.0};
#ifdef LH_STAMPS
    if (rung) return o;   // (the diagnostic build times one controller)
#endif
    if (rung && mode == 0) return o;   // (the initial linearisation builds no ladder, as k_ctrl)
    if (rung && !dec_src) ladder_wait(ctrl, seq);   // workgroup 0 decides and publishes
    int done, skip;
    if (dec_src || rung) {
        const LadderDec d = ladder_read(ctrl, prm, seq, rung);
        done = d.done;
        o.accept = d.accept;
        skip = d.skip;
        o.lambda = d.lambda;
        o.cur = __builtin_amdgcn_readfirstlane(ctrl->cur);
        // this trial's k_reduce stopped the loop: the host's done is raised here (ctrl_lm_step)
        if (dec_src && done && tid == 0 && host_done && ctrl->done_seq == seq && rung == 0) publish_stop(ctrl, host_done);
    } else {
        double tchi = 0.0, sl = 0.0, ndg = 0.0;
        CtrlWords cw{};
        if (tid == 0) {
            cw = ctrl_load(ctrl);
            tchi = 0.5 * rs_stage[LY.off_sc + LH_SC_CHI2];
            sl = rs_stage[LY.off_sc + LH_SC_SCALE];
            ndg = rs_stage[LY.off_sc + LH_SC_NDEG];
        }
        if (mode == 0) {   // max |diag H_pp| for computeLambdaInitLM (problem.cpp:486-496)
            double mx = 0.0;
            for (int i = tid; i < n; i += NT) mx = fmax(mx, fabs(rs_stage[LY.off_hd + i]));
            for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
            if (lane == 0) s_red[wave] = mx;
            lds_barrier();
        }
        if (tid == 0) {
            double mdiag = 0.0;
            if (mode == 0) {
                for (int w = 0; w < NT / 64; ++w) mdiag = fmax(mdiag, s_red[w]);
                mdiag = fmax(*maxd_in, mdiag);
            }
            int d_o, a_o, c_o;
            double lam_n;
            lds.flags[3] = ctrl_decide(ctrl, cw, prm, mode, mdiag, tchi, sl, ndg, rs_stage, LY, host_done, seq, d_o, a_o,
                                       c_o, lam_n, lds.cnt);
            if (prm.ladder > 1 && mode != 0) ladder_publish(ctrl, seq);   // the rung workgroups wait for it
            lds.flags[0] = d_o;
            lds.flags[1] = a_o;
            lds.flags[2] = c_o;
            lds.lam = lam_n;
        }
        lds_barrier();
        done = lds.flags[0];
        o.accept = lds.flags[1];
        o.cur = lds.flags[2];
        skip = lds.flags[3];
        o.lambda = lds.lam;
    }
    if (done || skip) return o;   // stopped, an evaluate-only acceptance, or a rejection onto a built rung
    // the ladder: a factor builds prm.ladder rungs (every factor, or with ladder_eager off only one after a
    // rejection); rung r factors at the lambda r more rejections set (ladder_read)
    const bool build = mode != 0 && ladder_build(prm, o.accept);
    if (rung != 0 && (!build || rung >= prm.ladder)) return o;
    if (rung == 0 && tid == 0) ctrl->lad_n = build ? prm.ladder : 1;
    o.run = true;
    return o;
}

// The controllers' tail (xs: the pose step in pose order, in LDS): the pose part of the gain
// denominator (isGoodStepInLM's scale, problem.cpp:528-533), the wave partials summed in wave order
// into ctrl->spose_l[rung], and (dxp non-null) the step stored for k_lin.  The candidate poses
// (VertexPose::add) are built by the next k_lin (d_pose_candidate).  All NT threads.
template <int NT>
__device__ __forceinline__ void ctrl_step_tail(lh_ctrl* __restrict__ ctrl, const lh_params& prm, int n, double lambda,
                                               const double* xs, const double* bpv, const double* hdv, double* s_red,
                                               double* __restrict__ dxp, int rung = 0) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double sp = 0.0;
    for (int i = tid; i < n; i += NT) {
        const double d = xs[i], b = bpv[i];
        sp += (prm.strategy == 0) ? d * (lambda * d + b) : d * (lambda * hdv[i] * d + b);
        if (dxp) dxp[i] = d;
    }
    for (int off = 32; off > 0; off >>= 1) sp += __shfl_xor(sp, off);
    if (lane == 0) s_red[wave] = sp;
    lds_barrier();
    CSTAMP(9);
    if (tid == 0) {
        double s2 = 0.0;
        for (int w = 0; w < NT / 64; ++w) s2 += s_red[w];
        ctrl->spose_l[rung] = s2;
    }
}
