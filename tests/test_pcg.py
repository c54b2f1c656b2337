"""PCG reduced-pose solve (BASELINE config 3 "Schur + PCG").

The reference's Problem::PCGSolver (problem.cpp:584-614) is dead code (its call
site :422 is commented out) and buggy (the first step alpha*p never reaches x,
:595-596).  The build offers it fixed, as lh_options.linear_solver = PCG, with
the reference's stop rule ||r|| <= 1e-6 ||b|| (:597) and cap 2*rows (:422).
The oracle restates the same fixed algorithm (oracle/lego_oracle.c pcg_solve).

Tolerances: a PCG solve stops at a residual threshold, so a rounding difference
can move the stop by one step; single systems are compared at the stop rule's
own scale (x within 1e-5 relative), full solves at the north-star bar (final
chi2 within 1e-6 of the oracle's PCG solve and of the reference LDLT solve).
"""
import numpy as np
import pytest

import lego_ba
import oracle_bind as ob
from windows import stable_window, window


def spd_system(n, seed):
    """S + lambda I shaped like the reduced pose system: block-banded, wide diagonal spread."""
    rng = np.random.default_rng(seed)
    P = n // 6
    S = np.zeros((n, n))
    for p in range(P):
        for q in range(p, min(P, p + 8)):
            S[6 * p:6 * p + 6, 6 * q:6 * q + 6] += rng.standard_normal((6, 6)) * (10.0 ** rng.uniform(0, 2))
    S = S @ S.T + np.diag(10.0 ** rng.uniform(1, 4, n))
    return S, rng.standard_normal(n) * 1e2


# ------------------------------------------------------------------ CPU: the oracle's PCG
@pytest.mark.parametrize("n", [6, 30, 60, 120])
def test_oracle_pcg_meets_stop_rule(n):
    S, b = spd_system(n, n)
    x, steps = ob.pcg_solve(S, b)
    assert 1 <= steps <= 2 * n + 1
    assert np.linalg.norm(S @ x - b) <= 1e-6 * np.linalg.norm(b) * (1 + 1e-9)
    xr = np.linalg.solve(S, b)
    assert np.linalg.norm(x - xr) <= 1e-3 * np.linalg.norm(xr)


def test_oracle_pcg_first_step_applied():
    """The reference's bug (problem.cpp:595-596): on a diagonal system Jacobi-PCG is exact after one
    step, which the reference would drop (returning x = 0); the fixed solver returns the solution."""
    S = np.diag([2.0, 5.0, 7.0])
    b = np.array([1.0, -2.0, 3.0])
    x, steps = ob.pcg_solve(S, b)
    assert steps == 1
    assert np.allclose(x, b / np.diag(S), rtol=1e-15)


def test_oracle_pcg_cap_and_zero_rhs():
    S, b = spd_system(60, 3)
    x, steps = ob.pcg_solve(S, b, tol=0.0, max_iters=5)
    assert steps == 6                          # first step + maxIter loop iterations (problem.cpp:598)
    x0, s0 = ob.pcg_solve(S, np.zeros(60))
    assert s0 == 0 and not x0.any()


@pytest.mark.parametrize("cfg,seed,family", [("C1", 0, "stable_noout"), ("mini", 0, "stable_noout"),
                                              ("C1", 1, "stable")])
def test_oracle_pcg_solve_matches_ldlt_solve(cfg, seed, family):
    w = window(cfg, seed=seed, family=family)
    a = ob.solve(w)
    c = ob.solve(w, linear_solver=1)
    assert c["pcg_iterations"] > 0 and a["pcg_iterations"] == 0
    assert c["iterations"] == a["iterations"]
    assert abs(c["chi2_final"] - a["chi2_final"]) / a["chi2_final"] < 1e-6


# ------------------------------------------------------------------ GPU: k_ctrl's PCG
@pytest.mark.gpu
@pytest.mark.parametrize("n", [6, 12, 60, 96, 120, 126])
def test_gpu_pcg_probe_matches_oracle(n):
    import ctypes as C
    import torch
    S, b = spd_system(n, 100 + n)
    lib = lego_ba.ba_lib()
    lib.lh_debug_pcg_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p,
                                       C.POINTER(C.c_int)]
    St = torch.tensor(S, dtype=torch.float64, device="cuda").contiguous()
    bt = torch.tensor(b, dtype=torch.float64, device="cuda")
    xt = torch.zeros(n, dtype=torch.float64, device="cuda")
    it = C.c_int(0)
    assert lib.lh_debug_pcg_probe(St.data_ptr(), bt.data_ptr(), n, 1e-6, 0, xt.data_ptr(), C.byref(it)) == 0
    x = xt.cpu().numpy()
    xo, so = ob.pcg_solve(S, b)
    # these random systems take more steps than rows (n = 96: ~155), so rounding shapes the tail of the
    # convergence and the step count moves with the order of the sums (the oracle's are sequential)
    assert abs(it.value - so) <= max(2, 0.03 * so)
    assert np.linalg.norm(S @ x - b) <= 1.01e-6 * np.linalg.norm(b)
    assert np.linalg.norm(x - xo) <= 1e-5 * np.linalg.norm(xo)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,seed", [("C1", 0), ("mini", 0), ("C2", 1), ("C2", 2)])
def test_gpu_pcg_full_solve_parity(cfg, seed):
    w = window(cfg, seed=seed, family="stable_noout")
    g = lego_ba.Solver(linear_solver=lego_ba.LH_SOLVER_PCG).solve(w)
    o = ob.solve(w, linear_solver=1)
    r = ob.solve(w)                            # the reference's LDLT path
    assert g["pcg_iterations"] > 0
    assert g["iterations"] == o["iterations"]
    assert abs(g["chi2_final"] - o["chi2_final"]) / o["chi2_final"] < 1e-6
    assert abs(g["chi2_final"] - r["chi2_final"]) / r["chi2_final"] < 1e-6
    assert np.allclose(g["pose_Tcw"], o["pose_Tcw"], atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("family,tol", [("stable_noout", 1e-8), ("default", 1e-2)])
def test_gpu_pcg_single_trial(family, tol):
    """One trial.  On a gauge-free window (survey default: no fixed pose) S + lambda I is
    ill-conditioned along the gauge, and a 1e-6 residual stop leaves an error there that rounding
    differences in the iterates move: the step (and chi2 after it) only agrees to ~1e-3."""
    w = window("C2", seed=0, family=family)
    g = lego_ba.Solver(linear_solver=lego_ba.LH_SOLVER_PCG, max_iters=1, max_trials=1).solve(w)
    o = ob.solve(w, linear_solver=1, max_iters=1, max_trials=1)
    assert abs(g["pcg_iterations"] - o["pcg_iterations"]) <= 2
    assert abs(g["chi2_final"] - o["chi2_final"]) / o["chi2_final"] < tol


@pytest.mark.gpu
def test_gpu_pcg_c3_window():
    """The bench window (C3) through PCG: converges to the LDLT solve's chi2 (north-star bar)."""
    w = window("C3", seed=0, family="stable_noout")
    s = lego_ba.Solver(linear_solver=lego_ba.LH_SOLVER_PCG)
    g = s.solve(w)
    d = lego_ba.Solver().solve(w)
    assert abs(g["chi2_final"] - d["chi2_final"]) / d["chi2_final"] < 1e-6
    assert g["iterations"] == d["iterations"]


# ------------------------------------------------------------------ GPU: many-keyframe windows (k_ctrl_p)
@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("P,L,seed,kw", [(22, 2000, 1, {}), (40, 3000, 2, {}), (64, 4000, 2, {}), (96, 5000, 3, {}),
                                         (128, 6000, 3, {}), (128, 6000, 1, {}), (256, 12000, 1, {})])
def test_gpu_pcg_many_keyframes(P, L, seed, kw):
    """Windows past 21 keyframes through PCG, past 64 with the block-sparse
    reduced system (k_ctrl_p: S p over the packed pose-pair blocks, never densified): one trial at the
    single-trial bar, then the full solve against the oracle's PCG (same iterations, final chi2 1e-6,
    poses and landmarks 1e-6) and against the reference LDLT solve (chi2 1e-6).  The windows are
    reproducible: the oracle's PCG and LDLT solves agree on iterations and trials across thread counts
    (128 keyframes seed 1 rejects 12 of its 20 trials).  Windows of random keyframe subsets stall at
    different trials under reordering even in the oracle, so they are not used here."""
    w = stable_window(P, L, seed, **kw)
    g1 = lego_ba.Solver(linear_solver=lego_ba.LH_SOLVER_PCG, max_iters=1, max_trials=1).solve(w)
    o1 = ob.solve(w, linear_solver=1, max_iters=1, max_trials=1)
    # the residual stop is crossed within a few steps of the oracle's (rounding in S and the dots)
    assert abs(g1["pcg_iterations"] - o1["pcg_iterations"]) <= max(2, 0.03 * o1["pcg_iterations"])
    assert abs(g1["chi2_initial"] - o1["chi2_initial"]) / o1["chi2_initial"] < 1e-12
    assert abs(g1["chi2_final"] - o1["chi2_final"]) / o1["chi2_final"] < 1e-8
    g = lego_ba.Solver(linear_solver=lego_ba.LH_SOLVER_PCG).solve(w)
    o = ob.solve(w, linear_solver=1)
    r = ob.solve(w)
    assert g["pcg_iterations"] > 0
    assert g["iterations"] == o["iterations"] and g["trials"] == o["trials"]
    assert abs(g["chi2_final"] - o["chi2_final"]) / o["chi2_final"] < 1e-6
    assert abs(g["chi2_final"] - r["chi2_final"]) / r["chi2_final"] < 1e-6
    assert np.allclose(g["pose_Tcw"], o["pose_Tcw"], atol=1e-6)
    assert np.allclose(g["lm_xyz"], o["lm_xyz"], atol=1e-6)
    # bitwise repeatable (fixed-order reductions)
    g2 = lego_ba.Solver(linear_solver=lego_ba.LH_SOLVER_PCG).solve(w)
    assert g2["chi2_final"] == g["chi2_final"] and np.array_equal(g2["pose_Tcw"], g["pose_Tcw"])


@pytest.mark.gpu
def test_many_keyframes_envelope():
    """Past 64 keyframes a banded window runs LDLT (k_ctrl_b) as well as PCG (k_ctrl_p, up to 256)."""
    w = stable_window(80, 2000, 5)
    s = lego_ba.Solver(max_iters=2)
    a = s.solve(w)
    assert s.controller() == "k_ctrl_b" and a["chi2_final"] < a["chi2_initial"]
    sp = lego_ba.Solver(linear_solver=lego_ba.LH_SOLVER_PCG, max_iters=2)
    g = sp.solve(w)
    assert sp.controller() == "k_ctrl_p" and g["chi2_final"] < g["chi2_initial"]
    assert abs(g["chi2_final"] - a["chi2_final"]) / a["chi2_final"] < 1e-6
