"""The long-double linearisation (tests/lin_ref.py) against the oracle, the planner shapes its cases claim, and its
teeth: everything tests/test_lin_system_gpu.py relies on that needs no GPU.

(a) the double-precision oracle's reduced system lies within e < 1e-11 of the reference at 1, 2 and 8 threads (the
    yardstick is not loose: measured 2e-15 .. 3.2e-13, the worst on `far`, kappa(H_ll) = 6e6);
(b) every case reaches the chunk tile counts, lane groups, landmark counts and sub-batch counts it was chosen for;
(c) corrupting the reference's handling of ONE edge moves the block metric by at least 1000 x the tolerance the GPU
    test allows on that case (a dropped edge: ~1e10 x);
(d) a plain double evaluation of the same statements keeps the a-priori summation bounds the GPU test applies to
    b_p, diag H_pp and sum rho0, and max |diag H_ll| to 16 eps: the bounds are ones a correct double implementation
    meets.  With the terms of b_p taken as the products J rho1 r (r already formed), it does not: r = uv - proj is
    a difference of hundreds of pixels leaving about one, and double NumPy exceeds (n_p + 16) eps sum |J rho1 r| by
    1.7 x on allT and 34 x on p70.  The bound therefore counts both operands of that difference (lin_ref.linearise).
"""
import numpy as np
import pytest

import lin_cases
import lin_ref
import oracle_bind as ob

EPS = 2.0 ** -52
THREADS = (1, 2, 8)
GPU_MARGIN = 8.0      # tests/test_lin_system_gpu.py: tolerance = GPU_MARGIN x the oracle's own e, floor 64 eps
MUTATION_SEEDS = (0, 1, 2)


def reference(name):
    w, _, opts, _ = lin_cases.case(name)
    return lin_ref.linearise(w, huber_delta=opts.get("huber_delta", 5.991))


def oracle_errors(w, opts, R, **state):
    """(largest block error of the oracle's S over the thread counts, largest b_s error) against reference R."""
    ws = dict(w, **state)
    es, eb = [], []
    for t in THREADS:
        S, bs, _ = ob.reduced_system(ws, n_threads=t, **opts)
        es.append(lin_ref.block_error(S, R["S"], R["fixed"])[0])
        eb.append(lin_ref.rhs_error(bs, R)[0])
    return max(es), max(eb)


@pytest.mark.parametrize("name", list(lin_cases.CASES))
def test_oracle_within_yardstick(name):
    w, _, opts, _ = lin_cases.case(name)
    R = reference(name)
    assert R["kappa"].max() < 1e8
    for t in THREADS:
        S, bs, chi2 = ob.reduced_system(w, n_threads=t, **opts)
        e, pq = lin_ref.block_error(S, R["S"], R["fixed"])
        eb, row = lin_ref.rhs_error(bs, R)
        print(f"{name} threads {t}: e(S) {e:.2e} at pair {pq}, e(b_s) {eb:.2e} at row {row}")
        assert e < 1e-11, (name, t, e, pq)
        assert eb < 1e-11, (name, t, eb, row)
        assert abs(chi2 - float(R["chi2"])) <= R["chi2_bound"]
        fx = np.repeat(R["fixed"], 6)
        assert not S[fx].any() and not S[:, fx].any() and not bs[fx].any()   # a fixed pose contributes nothing


@pytest.mark.parametrize("name", list(lin_cases.CASES))
def test_planner_shapes(name):
    w, chunk, _, claim = lin_cases.case(name)
    got = lin_cases.plan_shapes(w, chunk)
    for key, want in claim.items():
        assert got[key] == want, (name, key, got[key], want)
    P = w["n_poses"]
    if not got["sparse"]:
        assert len(got["pair_pq"]) == P * (P + 1) // 2
    assert (got["pair_pq"][:, 0] <= got["pair_pq"][:, 1]).all()


def _mutations(name):
    w = lin_cases.case(name)[0]
    kinds = ["drop_edge", "swap_poses", "wrong_camera"]
    if name == "outl":
        kinds.append("outlier_weight_one")
    return [(k, s) for k in kinds for s in MUTATION_SEEDS]


@pytest.mark.parametrize("name", list(lin_cases.CASES))
def test_mutations_move_the_metric(name):
    w, _, opts, _ = lin_cases.case(name)
    R = reference(name)
    tol = max(GPU_MARGIN * oracle_errors(w, opts, R)[0], 64 * EPS)
    for mut in _mutations(name):
        M = lin_ref.linearise(w, huber_delta=opts.get("huber_delta", 5.991), mutation=mut)
        e, pq = lin_ref.block_error(M["S"], R["S"], R["fixed"])
        eb, row = lin_ref.rhs_error(M["bs"], R)
        print(f"{name} {mut}: e(S) {e:.2e} = {e / tol:.1e} x tol at pair {pq}, e(b_s) {eb:.2e} at row {row}")
        if opts.get("huber_delta", 5.991) == 0 and mut[0] == "swap_poses":
            e = eb   # without a robust kernel S does not depend on the measurements: the swap shows in b_s alone
        assert e >= 1000 * tol, (name, mut, e, tol)


@pytest.mark.parametrize("name", list(lin_cases.CASES))
def test_double_evaluation_keeps_the_bounds(name):
    w, _, opts, _ = lin_cases.case(name)
    R = reference(name)
    D = lin_ref.linearise(w, huber_delta=opts.get("huber_delta", 5.991), dtype=np.float64)
    live = np.repeat(~R["fixed"], 6)
    d = np.abs((D["bp"].astype(lin_ref.LD) - R["bp"]).astype(np.float64))
    print(f"{name}: double b_p at {np.max(d[live] / R['bp_bound'][live]):.3f} of the bound, "
          f"{np.max(d[live] / R['bp_bound_narrow'][live]):.2f} of the one on the formed residual")
    for key in ("bp", "hd"):
        d = np.abs((D[key].astype(lin_ref.LD) - R[key]).astype(np.float64))
        assert (d <= R[key + "_bound"]).all(), (name, key, (d / np.maximum(R[key + "_bound"], 1e-300)).max())
    assert abs(float(D["chi2"] - R["chi2"])) <= R["chi2_bound"]
    assert abs(float(D["maxd"] - R["maxd"])) <= 16 * EPS * float(R["maxd"])


def test_reference_is_symmetric_and_consistent():
    """S is symmetric to long-double rounding, and H_ll Hinv = I: the adjugate inverse is the inverse."""
    R = reference("far")
    S = R["S"]
    # (tH_e Hpl_f^T and its transpose are rounded apart; the Schur complement of far landmarks cancels)
    asym = lin_ref.block_error(S.T, S, R["fixed"])[0]
    print(f"far: the reference's own asymmetry {asym:.2e}")
    assert asym < 1e-15   # the oracle's distance on this case is 3e-13
    I = np.einsum("lij,ljk->lik", R["Hll"], R["Hinv"])
    assert float(np.abs(I - np.eye(3)).max()) < R["kappa"].max() * 2.0 ** -60


def test_mutation_needs_a_target():
    w = lin_cases.case("nohuber")[0]
    with pytest.raises(ValueError):
        lin_ref.linearise(w, huber_delta=0.0, mutation=("outlier_weight_one", 0))   # no robust kernel: no outlier
