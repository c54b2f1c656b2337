// lh_marg_host.cpp — lh_marginalize (include/lego_ba.h): a keyframe of the window the handle last
// solved, marginalised into a prior on the poses that stay.  One stream of launches and one download:
//   k_marg_mask                        the observation words with every edge of a landmark that pose m does not
//                                      observe made invalid, in a copy of this file's (lh::MargState);
//   lh::relin_enqueue                  the snapshot of the returned state and the solver's own k_lin<T, false> and
//                                      k_reduce (mode 0), unchanged, on that copy with guard 1 (lh_cov_host.cpp);
//   k_marg_assemble, k_marg_schur      A = the packed system + the earlier prior, the 6x6 factor, H_prior and b_prior.
// The solver's state is only read; the per-edge rho0 and inlier flags of the masked linearisation go to buffers of
// this call's.
#include <cstring>

#include "lh_handle.h"
#include "lh_launch.h"

using namespace lh;

namespace {

int marginalize_impl(lh_handle* h, const lh_marg_input* in, lh_marg_result* out) {
    if (!h || !in || !out) return LH_E_BADARG;
    FrontendCall call(h);
    STAGE(call.select());
    if (!h->uploaded || !h->solved) return LH_E_STATE;
    if (h->opt.world_size > 1 || h->P > LH_PMAX_WIN) return LH_E_UNSUPPORTED;
    const int P = h->P, m = in->marg_pose, n6 = 6 * P, n_sb = h->plan.n_sb;
    if (m < 0 || m >= P || !out->H_prior || !out->b_prior || (in->prior_H != nullptr) != (in->prior_b != nullptr))
        return LH_E_BADARG;
    out->n_landmarks = 0; out->n_edges = 0; out->n_degenerate = 0; out->bad_row = -1;
    out->min_pivot = 0.0; out->max_pivot = 0.0; out->time_ms = 0.0;

    hipStream_t s = h->stream;
    MargState& mg = h->marg;
    const size_t L = (size_t)h->L, nH = (size_t)n6 * n6, nslots = (size_t)h->n_slots;
    // the download: the result block, H_prior, b_prior, then lm_marginalised's bytes
    const size_t o_H = LH_MARG_R_N, o_b = o_H + nH, o_lm = o_b + n6, n_out = o_lm + (L + 7) / 8;
    STAGE(relin_ensure(h, mg.lin));
    HIPCHK(mg.meta.ensure(nslots)); HIPCHK(mg.counts.ensure(3 * (size_t)std::max(n_sb, 1)));
    HIPCHK(mg.rho.ensure(nslots)); HIPCHK(mg.wflag.ensure(2 * nslots));
    HIPCHK(mg.A.ensure(nH)); HIPCHK(mg.b.ensure(n6)); HIPCHK(mg.Y.ensure(6 * (size_t)n6 + 6));
    HIPCHK(mg.out.ensure(n_out));
    HIPCHK(h->s_out.ensure(n_out));
    if (in->prior_H) {   // the earlier prior: through pinned staging, one copy
        HIPCHK(mg.prior.ensure(nH + n6)); HIPCHK(mg.s_prior.ensure(nH + n6));
        const ByteSeg seg[2] = {{mg.s_prior.p, in->prior_H, nH * sizeof(double)},
                                {mg.s_prior.p + nH, in->prior_b, (size_t)n6 * sizeof(double)}};
        par_copy(h, seg, 2);
        HIPCHK(hipMemcpyAsync(mg.prior.p, mg.s_prior.p, (nH + n6) * sizeof(double), hipMemcpyHostToDevice, s));
    }

    STAGE(call.start());
    uint8_t* d_lm = reinterpret_cast<uint8_t*>(mg.out.p + o_lm);
    HIPCHK(hipMemsetAsync(d_lm, 0, ((L + 7) / 8) * sizeof(double), s));   // (a landmark without a record: 0)
    const lh_marg_mask_args ma{h->d_sbs.p, h->d_meta.p, h->d_lm_perm.p, mg.meta.p, mg.counts.p, d_lm, n_sb, P, m};
    HIPCHK(lh_launch_marg_mask(s, &ma));
    lh_params prm = h->prm;   // a landmark without a valid edge, and a rank-deficient one of M, held fixed
    prm.guard = 1;
    STAGE(relin_enqueue(h, mg.lin, mg.meta.p, mg.rho.p, mg.wflag.p, prm));
    const lh_marg_args aa{mg.lin.rs.p, h->d_pair_pq.p, h->d_fixed.p, mg.counts.p,
                          in->prior_H ? mg.prior.p : nullptr, in->prior_H ? mg.prior.p + nH : nullptr,
                          P, h->LY.npairs, m, n_sb, mg.A.p, mg.b.p, mg.Y.p, mg.Y.p + 6 * (size_t)n6,
                          mg.out.p + o_H, mg.out.p + o_b, mg.out.p};
    HIPCHK(lh_launch_marg_prior(s, &aa));
    STAGE(call.stop());
    HIPCHK(hipMemcpyAsync(h->s_out.p, mg.out.p, n_out * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    STAGE(call.time(&out->time_ms));
    const double* r = h->s_out.p;
    out->n_landmarks = (int32_t)r[LH_MARG_R_NLM];
    out->n_edges = (int32_t)r[LH_MARG_R_NEDGE];
    out->n_degenerate = (int32_t)r[LH_MARG_R_NDEG];
    out->min_pivot = r[LH_MARG_R_MINP];
    out->max_pivot = r[LH_MARG_R_MAXP];
    if (r[LH_MARG_R_BAD] >= 0.0) { out->bad_row = (int32_t)r[LH_MARG_R_BAD]; return LH_E_SINGULAR; }
    // rank-deficient landmarks that the solver does not hold fixed poison its system (their factor's NaN marker)
    if (!h->opt.degenerate_guard && out->n_degenerate != 0) { out->bad_row = 0; return LH_E_SINGULAR; }
    const ByteSeg seg[3] = {{out->H_prior, r + o_H, nH * sizeof(double)},
                            {out->b_prior, r + o_b, (size_t)n6 * sizeof(double)},
                            {out->lm_marginalised, r + o_lm, L}};
    par_copy(h, seg, 3);
    return LH_OK;
}

}  // namespace

extern "C" int lh_marginalize(lh_handle* h, const lh_marg_input* in, lh_marg_result* out) {
    return no_throw(marginalize_impl, h, in, out);
}
