"""Every controller's pose step against a long-double solve of the system it read (tests/step_ref.py).

The controllers claim that the pending pose step solves (S + lambda D) dx = b_s.  Here the claim is checked on the
production solves themselves -- the host's unit tables, the fused tails, the lambda insertion, the image / band image /
packed sources, the ladder's rung workgroups with their own storage -- for the cases of tests/step_cases.py (their
planner paths and first decisions are asserted on the CPU, tests/test_step_ref_cpu.py).  The steps are read through
lh_debug_ladder_steps (Solver.ladder_steps), the systems through lh_debug_reduced_system.

Routes (deterministic runs of one trajectory):
  S0          max_iters = 0: the staged system of the initial linearisation, S from the layout the controller reads
              (k_ctrl's LDS image, k_ctrl_b's band image, else the packed blocks), as Test A of test_lin_system_gpu.py.
  first step  max_iters = max_trials = 1: the mode-0 controller (it decides itself, the initial lambda, no ladder).  Its
              step must solve S0 at trace_lambda[0]; lad_n = 1; the trial's decision is the case's.
  ladder, R   max_iters = 1, max_trials = m: the first trial is rejected, the factor after it builds m rungs from the
              COMMITTED system (the committed half of the image or band image; k_ctrl_g's committed dense copy), and
              nothing factors after it (every later trial evaluates a built rung; an acceptance stops the loop).  Rung r
              must solve S0 at rung_lambdas(lambda_1, 4, ...)[r], lambda_1 one rejection update of trace_lambda[0].
  ladder, A   max_iters = 2, max_trials = m: the factor after the acceptance builds m eager rungs from the STAGED system
              S1; iteration 2 only evaluates built rungs and stops.  Rung r must solve S1 at
              rung_lambdas(trace_lambda[1], 2, ...)[r].
S1, the accepted linearisation as the controller read it, comes from the same run: b_s, b_p, diag H_pp from the
committed packed buffer, S from the committed packed blocks where the controller reads those (k_ctrl_p; k_ctrl_b under
LH_NO_BIMG, which k_reduce commits block by block).  Where the controller reads an image the packed BLOCKS are not
S1 -- k_reduce then writes and commits the image alone (lh_kernels.hip: `if (prm.img) ... else if (prm.bimg) ... else`
the packed block) and the hook has no view of the image's committed half -- so S is the staged half of the image,
which the accepting controller read and which the evaluate-only trials after it leave as it is or refill from the
committed half.  Either way the system is asserted equal, bit for bit, to the staged system of Test B's route on that
window (LH_NO_EVO, LH_NO_LADDER, LH_NO_BATCH, max_iters = max_trials = 1).  (k_ctrl_g keeps no committed packed S either -- its dense copy is double-buffered -- and both its cases are
R-cases, judged against S0.)

Per step, LDL^T controllers: rows of fixed poses exact zeros; forward error e and backward error eta (step_ref) at most
max(MARGIN x yardstick, 64 eps), the yardstick the worse of the oracle's LDL^T and a Cholesky solve of the same A, b.
PCG controllers (the bars of tests/test_pcg.py): ||b - A x|| <= 1.01e-6 ||b|| in long double, lad_its[r] within max(2,
3 %) of ob.pcg_solve on the same system, x within 1e-5 relative of it.  spose_l[r], all controllers: against
sum_i dx_i (lambda D_ii dx_i + b_p,i) in long double from the GPU's own dx, within (n + 16) eps sum |terms|.
b_wide_packed (LH_NO_BIMG: the packed-block loaders of every sharded solve) must equal b_wide's steps bit for bit.

MARGIN (step_ref.MARGIN) is measured: the smallest power of two that is at least twice the worst e_gpu / e_yard below.
Measured e_gpu / e_yard | eta_gpu / eta_yard (MI355X; every step's figures are printed as RATIO lines; also DESIGN.md
4.6):

    case            first step      ladder: worst e (rung) | worst eta (rung)    e_yard, first step
    lds_band        0.15 | 1.01     1.65 (rung  4) | 1.47 (rung  0)    1.7e-12
    lds_dense       1.43 | 0.50     0.92 (rung  4) | 1.12 (rung  5)    9.4e-14
    lds_p21         1.59 | 0.82     0.83 (rung  9) | 1.39 (rung  7)    3.0e-13
    lds_tiny        0.29 | 0.29     3.02 (rung  4) | 1.91 (rung  8)    7.4e-15
    lds_s1          0.21 | 0.99     1.15 (rung  0) | 1.54 (rung  0)    9.5e-14
    g_p24           5.18 | 1.31     7.88 (rung  3) | 1.31 (rung  3)    8.9e-14
    g_p64           0.48 | 1.03     3.46 (rung  3) | 1.35 (rung  5)    2.2e-12
    b_p22           0.67 | 0.54     1.23 (rung  0) | 0.99 (rung  2)    8.0e-14
    b_p70           0.06 | 0.59     1.04 (rung  2) | 0.83 (rung  0)    2.3e-12
    b_wide          1.54 | 0.59     1.41 (rung  3) | 1.87 (rung  3)    5.2e-11
    b_lu            2.30 | 0.60     3.46 (rung  4) | 1.30 (rung  4)    3.3e-13
    b_p256          0.45 | 1.26     0.31 (rung  9) | 0.80 (rung  0)    1.2e-09
    b_s1            0.48 | 0.44     0.94 (rung  0) | 0.77 (rung  9)    6.6e-13
    lds_nd          0.12 | 1.34     1.17 (rung  4) | 1.25 (rung  3)    1.7e-12
    lds_lad16       0.15 | 1.01     1.65 (rung  4) | 1.47 (rung  0)    1.7e-12
    b_wide_packed   1.54 | 0.59     1.41 (rung  3) | 1.87 (rung  3)    5.2e-11

Worst e ratio 7.88, so MARGIN = 16; no backward-error ratio is above 1.91.  k_ctrl_g's three largest forward ratios
(g_p24: 4.54, 5.18, 7.88; its other steps and g_p64's are at most 3.46) come with backward ratios of 1.31 or less: the
step is as backward stable as the yardstick's two solves, and what differs is where in kappa(A) eta each solve's
forward error happens to fall (k_ctrl_g eliminates in Eigen's diagonal-pivot order, over a dense envelope; at g_p24's
rung 3 the yardstick's own e is 3.1e-14, its smallest of that ladder's first five rungs).  Not a fault; no margin was
widened for it.  spose_l: at most 2.3 % of its bound.  PCG (p_p30, p_p72, lds_pcg): steps within 3 of the
oracle's (of 417, where the bar is 12), x within 8.2e-6.  The whole file runs in 8 s.
"""
import numpy as np
import pytest

import lego_ba
import lin_cases
import oracle_bind as ob
import step_cases as sc
import step_ref as sr
import test_lin_system_gpu as tli

pytestmark = pytest.mark.gpu

EPS = sr.EPS
TEST_B_ENV = ("LH_NO_EVO", "LH_NO_LADDER", "LH_NO_BATCH")

_traj = {}


def read_system(s, w, packed=0):
    """(S, bs, bp, hd) of solver `s`: the packed buffer `packed` (0 staged, 1 committed), S from the staged image where
    the controller reads one."""
    P = w["n_poses"]
    pair_pq = lego_ba.plan_window(w)["pair_pq"].astype(np.int64)
    v, npairs = s.reduced_system(packed)
    assert npairs == len(pair_pq), (npairs, len(pair_pq))
    S, bs, bp, hd, _ = lin_cases.decode_packed(v, P, pair_pq)
    img, _ = s.reduced_system(3)
    src = "packed"
    if len(img):
        # with an image k_reduce writes no packed block of S.  An entry outside k_ctrl_b's band has no slot and is
        # taken as the zero the planner promised (held to the long-double linearisation in test_lin_system_gpu.py)
        S, bs_img = tli.decode_image(img, P, np.zeros((6 * P, 6 * P)))
        src = "image"
        if bs_img is not None:
            assert np.array_equal(bs_img, bs), "the image's rhs row differs from the packed b_s"
    return dict(S=S, bs=bs.copy(), bp=bp.copy(), hd=hd.copy(), src=src)


def solve(name, monkeypatch, max_iters, max_trials, env=()):
    """One run of the case: (result, solver); the caller closes the solver."""
    sc.set_env(monkeypatch, name)
    for v in env:
        monkeypatch.setenv(v, "1")
    s = lego_ba.Solver(max_iters=max_iters, max_trials=max_trials, **sc.solver_opts(name))
    try:
        g = s.solve(sc.window(name))
        assert g["degenerate"] == 0
    except Exception:
        s.close()
        raise
    return g, s


def trajectory(name, monkeypatch):
    """The case's runs, once: the systems S0 (and S1), the first step, the ladder's steps with their lambdas."""
    if name in _traj:
        return _traj[name]
    c, w = sc.CASES[name], sc.window(name)
    strategy = c["opts"].get("strategy", 0)
    m = c["max_trials"]
    T = dict(strategy=strategy)
    # S0
    g, s = solve(name, monkeypatch, 0, m)
    try:
        assert g["trials"] == 0
        T["ctrl"] = s.controller()
        assert T["ctrl"] == c["controller"]
        T["S0"] = read_system(s, w)
        assert s.ladder_steps()["lad_n"] == 0   # no controller has factored
    finally:
        s.close()
    # the first step
    g, s = solve(name, monkeypatch, 1, 1)
    try:
        L = s.ladder_steps()
        assert L["lad_n"] == 1 and L["lad"] == 0, (L["lad_n"], L["lad"])
        assert np.array_equal(L["dxp"][0], s.reduced_system(2)[0])
        assert g["trials"] == 1 and ("A" if g["accepted"] else "R") == c["first"], (name, g["accepted"], c["first"])
        T["first"] = dict(lam=[float(g["trace_lambda"][0])], dxp=L["dxp"], spose=L["spose"], its=L["its"], sys="S0")
    finally:
        s.close()
    # the ladder
    g, s = solve(name, monkeypatch, 1 if c["first"] == "R" else 2, m)
    try:
        L = s.ladder_steps()
        assert L["lad_n"] == m, (L["lad_n"], m)
        assert np.array_equal(L["dxp"][L["lad"]], s.reduced_system(2)[0]), "which = 2 is row lad of the ladder's steps"
        lam0 = float(g["trace_lambda"][0])
        assert lam0 == T["first"]["lam"][0]
        if c["first"] == "R":
            assert g["iterations"] == 1
            lam1, ni1 = sr.reject_update(lam0, 2.0, strategy)
            lams, sysn = sr.rung_lambdas(lam1, ni1, strategy, m), "S0"
        else:
            assert len(g["trace_lambda"]) >= 2 and g["accepted"] >= 1
            lams, sysn = sr.rung_lambdas(float(g["trace_lambda"][1]), 2.0, strategy, m), "S1"
            T["S1"] = read_system(s, w, packed=1)
        T["ladder"] = dict(lam=lams, dxp=L["dxp"], spose=L["spose"], its=L["its"], sys=sysn)
    finally:
        s.close()
    if c["first"] == "A":
        # S1 by Test B's route: the staged system of one accepted full trial
        g, s = solve(name, monkeypatch, 1, 1, env=TEST_B_ENV)
        try:
            assert g["accepted"] == 1 and g["trials"] == 1
            B = read_system(s, w)
        finally:
            s.close()
        S1 = T["S1"]
        assert B["src"] == S1["src"]
        for k in ("bs", "bp", "hd"):
            assert np.array_equal(S1[k], B[k]), f"{name}: committed {k} differs from Test B's staged one"
        assert np.array_equal(S1["S"], B["S"]), f"{name}: S1 ({S1['src']}) differs from Test B's staged system"
    _traj[name] = T
    return T


def rungs_of(name, n):
    r = sc.CASES[name]["rungs"]
    return list(range(n)) if r is None else [x for x in r if x < n]


def check_spose(tag, name, T, step, r):
    sysd = T[step["sys"]]
    ref, tol = sr.spose_ref(step["dxp"][r], step["lam"][r], T["strategy"], sysd["bp"], sysd["hd"])
    d = abs(float(step["spose"][r]) - ref)
    print(f"SPOSE {tag} {name} rung {r}: {d / tol if tol else 0.0:.3f} of its bound")
    assert d <= tol, (f"{name} ({T['ctrl']}) {tag} rung {r} lambda {step['lam'][r]:.6e}: spose_l = {step['spose'][r]!r}, "
                      f"long double {ref!r}, off by {d:.3e} > {tol:.3e}")


def check_ldlt(tag, name, T, step, rungs):
    """The LDL^T assertions of the steps `rungs`; returns the worst (e ratio, eta ratio)."""
    sysd = T[step["sys"]]
    fixed = np.repeat(np.asarray(sc.window(name)["pose_fixed"], bool), 6)
    worst = [0.0, 0.0]
    for r in rungs:
        lam, x = step["lam"][r], step["dxp"][r]
        where = f"{name} ({T['ctrl']}) {tag} rung {r} lambda {lam:.6e}"
        assert not x[fixed].any(), f"{where}: a fixed pose has a step"
        A = sr.assemble(sysd["S"], lam, T["strategy"])
        free = sr.free_rows(A, sysd["bs"])
        assert np.array_equal(free, ~fixed), f"{where}: the system's zero rows are not the fixed poses'"
        x_ref, corr = sr.solve_ld(A, sysd["bs"], free)
        e_y, eta_y = sr.yardstick(A, sysd["bs"], x_ref, free)
        e, eta = sr.forward_error(x, x_ref, free), sr.backward_error(A, sysd["bs"], x, free)
        p, dp = sr.worst_pose(x, x_ref)
        print(f"RATIO {tag} {name} rung {r} lambda {lam:.3e}: e_gpu {e:.2e} e_yard {e_y:.2e} ratio {e / e_y:.2f} | "
              f"eta_gpu {eta:.2e} eta_yard {eta_y:.2e} ratio {eta / eta_y:.2f} | reference correction {corr:.1e}, "
              f"worst pose {p}")
        worst = [max(worst[0], e / e_y), max(worst[1], eta / eta_y)]
        assert corr <= 2.0 ** -10 * e_y, f"{where}: the reference has not converged ({corr:.2e} against {e_y:.2e})"
        assert e <= sr.bound(e_y), (f"{where}: e = {e:.3e} > {sr.bound(e_y):.3e} ({e / e_y:.1f} x the yardstick's "
                                    f"{e_y:.2e}); worst pose {p}, off by {dp:.3e}")
        assert eta <= sr.bound(eta_y), (f"{where}: eta = {eta:.3e} > {sr.bound(eta_y):.3e} ({eta / eta_y:.1f} x the "
                                        f"yardstick's {eta_y:.2e}); worst pose {p}")
        check_spose(tag, name, T, step, r)
    return worst


def check_pcg(tag, name, T, step, rungs):
    sysd = T[step["sys"]]
    fixed = np.repeat(np.asarray(sc.window(name)["pose_fixed"], bool), 6)
    LD = sr.LD
    for r in rungs:
        lam, x = step["lam"][r], step["dxp"][r]
        where = f"{name} ({T['ctrl']}) {tag} rung {r} lambda {lam:.6e}"
        assert not x[fixed].any(), f"{where}: a fixed pose has a step"
        A = sr.assemble(sysd["S"], lam, T["strategy"])
        b = sysd["bs"]
        res = b.astype(LD) - A.astype(LD) @ x.astype(LD)
        rn, bn = float(np.sqrt((res * res).sum())), float(np.linalg.norm(b))
        xo, so = ob.pcg_solve(A, b)
        its = int(step["its"][r])
        dx = float(np.linalg.norm(x - xo) / np.linalg.norm(xo))
        p, dp = sr.worst_pose(x, xo)
        print(f"PCG {tag} {name} rung {r} lambda {lam:.3e}: residual {rn / bn:.3e}, steps {its} (oracle {so}), "
              f"|x - x_oracle| / |x_oracle| {dx:.2e}")
        assert rn <= 1.01e-6 * bn, f"{where}: ||b - A x|| = {rn / bn:.3e} ||b||"
        assert abs(its - so) <= max(2, 0.03 * so), f"{where}: {its} PCG steps, the oracle {so}"
        assert dx <= 1e-5, f"{where}: x is {dx:.2e} from the oracle's PCG; worst pose {p}, off by {dp:.3e}"
        check_spose(tag, name, T, step, r)


def check(tag, name, T, step):
    rungs = rungs_of(name, len(step["dxp"]))
    if name in sc.PCGS:
        return check_pcg(tag, name, T, step, rungs)
    return check_ldlt(tag, name, T, step, rungs)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_first_step(name, monkeypatch):
    T = trajectory(name, monkeypatch)
    check("first", name, T, T["first"])


@pytest.mark.parametrize("name", list(sc.CASES))
def test_ladder_steps(name, monkeypatch):
    T = trajectory(name, monkeypatch)
    check("ladder", name, T, T["ladder"])


def test_packed_loaders_equal_the_band_image(monkeypatch):
    """k_ctrl_b from the packed blocks (LH_NO_BIMG) and from the band image: the same steps bit for bit."""
    a, b = trajectory("b_wide", monkeypatch), trajectory("b_wide_packed", monkeypatch)
    assert a["S0"]["src"] == "image" and b["S0"]["src"] == "packed"
    assert np.array_equal(a["S0"]["S"], b["S0"]["S"]) and np.array_equal(a["S1"]["S"], b["S1"]["S"])
    for k in ("first", "ladder"):
        assert a[k]["lam"] == b[k]["lam"]
        for r in range(len(a[k]["dxp"])):
            assert np.array_equal(a[k]["dxp"][r], b[k]["dxp"][r]), f"{k} rung {r}: the packed loaders' step differs"
        assert np.array_equal(a[k]["spose"], b[k]["spose"])


def test_ladder_hook(monkeypatch):
    """lh_debug_ladder_steps: its errors (test_hook_arguments' pattern), and that it only reads -- a solve after it
    returns what a solve without it does."""
    import ctypes as C
    name = "lds_band"
    sc.set_env(monkeypatch, name)
    w = sc.window(name)
    f = lego_ba.ba_lib().lh_debug_ladder_steps
    n, lad_n, lad = C.c_int64(-1), C.c_int32(-1), C.c_int32(-1)
    sp, its = np.full(16, -7.0), np.full(16, -7, np.int32)
    s = lego_ba.Solver(max_iters=1, max_trials=10, **sc.solver_opts(name))
    try:
        with pytest.raises(lego_ba.LhError) as ei:
            s.ladder_steps()                      # no upload
        assert ei.value.status == lego_ba.LH_E_BADARG
        g1 = s.solve(w)
        L = s.ladder_steps()
        assert L["lad_n"] == 10 and L["dxp"].shape == (10, 6 * w["n_poses"])
        small = np.full(L["dxp"].size, -7.0)
        st = f(s.h, small.ctypes.data, small.size - 1, C.byref(n), C.byref(lad_n), C.byref(lad), sp.ctypes.data,
               its.ctypes.data)
        assert st == lego_ba.LH_E_BADARG and n.value == small.size and lad_n.value == 10
        assert (small == -7.0).all() and (sp == -7.0).all() and (its == -7).all() and lad.value == -1   # nothing written
        assert f(s.h, None, small.size, C.byref(n), C.byref(lad_n), C.byref(lad), sp.ctypes.data,
                 its.ctypes.data) == lego_ba.LH_E_BADARG
        assert not L["its"].any()                 # LDL^T: no PCG steps
        g2 = s.solve(w)                           # the same handle after the reads
        L2 = s.ladder_steps()
    finally:
        s.close()
    s = lego_ba.Solver(max_iters=1, max_trials=10, **sc.solver_opts(name))
    try:
        g3 = s.solve(w)                           # a handle the hook never touched
        g4 = s.solve(w)
    finally:
        s.close()
    for a, b in ((g1, g3), (g2, g4)):
        for k in ("pose_Tcw", "lm_xyz", "trace_chi2", "trace_lambda", "edge_robust_chi2"):
            assert np.array_equal(a[k], b[k]), k
        assert (a["chi2_final"], a["trials"], a["accepted"]) == (b["chi2_final"], b["trials"], b["accepted"])
    assert np.array_equal(L["dxp"], L2["dxp"]) and np.array_equal(L["spose"], L2["spose"])
