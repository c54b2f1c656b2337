"""CPU side of the controller step tests: what tests/test_ctrl_step_gpu.py relies on, checked without a GPU.

  - every case of tests/step_cases.py reaches the controller path it is listed for (lego_ba.solve_config), and its
    first trial's decision is the listed one in the oracle at 1 and 8 threads;
  - the reference may judge: on the oracle's own S, b_s of each window, at lambdas spanning the ladder, solve_ld's last
    correction is at most 2^-10 of the yardstick's forward error (measured: at most 2e-15 where the yardstick is
    1e-10, at most 1e-16 where it is 1e-13);
  - rung_lambdas is the oracle's rejection sequence, strategy 0 and 1;
  - the criterion has teeth: tests/test_ctrl_units.replay with the planner's full unit table meets it; with one valid
    unit word cleared, or one tile row of one step read a step stale, it misses it by more than 1e3.
"""
import numpy as np
import pytest

import lego_ba
import oracle_bind as ob
import step_cases as sc
import step_ref as sr
import test_ctrl_units as tcu
import windows

# the windows the margin is measured on: one case per distinct (window, strategy)
MARGIN_CASES = [n for n in sc.LDLT if n not in ("lds_nd", "b_wide_packed")]

_sys = {}


def oracle_system(name):
    """The oracle's S (its lower triangle, mirrored), b_s of the case's window at its input state, once per window."""
    key = repr(sorted(sc.CASES[name]["gen"].items())) + repr(sc.CASES[name]["fixed"])
    if key not in _sys:
        S, bs, _ = ob.reduced_system(sc.window(name), n_threads=1, huber_delta=0.0, gate_mode=1)
        _sys[key] = (sr.lower_symmetric(S), bs)
    return _sys[key]


def ladder_span(name):
    """The initial lambda and rungs 0, middle and last of the ladder a first rejection builds."""
    c = sc.CASES[name]
    s = c["opts"].get("strategy", 0)
    lam0 = c["opts"].get("lambda_init", 1e-5)
    lam1, ni1 = sr.reject_update(lam0, 2.0, s)
    lad = sr.rung_lambdas(lam1, ni1, s, c["max_trials"])
    picks = [lam0, lad[0], lad[len(lad) // 2], lad[-1]]
    return s, (picks[::3] if name == "b_p256" else picks)   # (1536 rows: the two ends)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_planner_claims(name, monkeypatch):
    sc.set_env(monkeypatch, name)
    cfg = sc.config(name)
    assert sc.check_claims(name, cfg) == [], cfg
    if name == "lds_nd":
        assert cfg["nd_steps"] > 0
    if name == "b_p256":
        assert 6 * sc.window(name)["n_poses"] == 1536   # BNMAX
    if name == "b_p70":
        n = 6 * sc.window(name)["n_poses"]
        assert n == 420 and ((n + 15) & ~15) != n
    if name == "lds_p21":
        assert 6 * sc.window(name)["n_poses"] == 126


@pytest.mark.parametrize("name", list(sc.CASES))
def test_first_decision(name):
    w = sc.window(name)
    for t in (1, 8):
        o = ob.solve(w, max_iters=1, max_trials=1, n_threads=t, **sc.oracle_opts(name))
        assert o["trials"] == 1
        assert ("A" if o["accepted"] else "R") == sc.CASES[name]["first"], (name, t)


def test_strategy1_diagonal_is_the_oracles():
    """assemble's strategy-1 form against the oracle's own solve (the source says S[i][i] += lambda S[i][i]; this runs
    it).  An accepted strategy-1 trial of the oracle returns exp(dx) T for the step of (S + lambda diag S) dx = b_s at
    lambda = 1e-5: solve_ld's step of that system reproduces the poses, the step of S + lambda I does not."""
    import lin_ref
    w = sc.window("b_p22")   # (its first strategy-1 trial is accepted; the listed strategy-1 cases reject theirs)
    o = ob.solve(w, max_iters=1, max_trials=1, n_threads=1, huber_delta=0.0, strategy=1, gate_mode=1)
    assert o["accepted"] == 1, "the comparison needs an accepted trial"
    S, bs = oracle_system("b_p22")
    P = w["n_poses"]
    err = {}
    for s in (0, 1):
        x, _ = sr.solve_ld(sr.assemble(S, 1e-5, s), bs)
        T = np.asarray(lin_ref.left_update(x.reshape(P, 6), w["pose_Tcw"]), np.float64).reshape(P, 12)
        err[s] = float(np.abs(T - o["pose_Tcw"]).max())
    print(f"STRATEGY1 pose distance from the oracle's trial: diag(S) form {err[1]:.2e}, identity form {err[0]:.2e}")
    assert err[1] <= 1e-9 and err[0] >= 1e3 * err[1], err


@pytest.mark.parametrize("name", MARGIN_CASES)
def test_reference_converges_past_the_yardstick(name):
    S, bs = oracle_system(name)
    s, lams = ladder_span(name)
    for lam in lams:
        A = sr.assemble(S, lam, s)
        free = sr.free_rows(A, bs)
        fixed = np.repeat(np.asarray(sc.window(name)["pose_fixed"], bool), 6)
        assert np.array_equal(free, ~fixed), "the zero rows are the fixed poses'"
        x, corr = sr.solve_ld(A, bs, free)
        assert not x[~free].any()
        e_y, eta_y = sr.yardstick(A, bs, x, free)
        eta = sr.backward_error(A, bs, x, free)
        print(f"REF {name} lambda {lam:.3e}: last correction {corr:.2e}, yardstick e {e_y:.2e} eta {eta_y:.2e}, "
              f"eta(ref) {eta:.2e}")
        assert corr <= 2.0 ** -10 * e_y, (name, lam, corr, e_y)
        assert eta <= 2.0 ** -10 * eta_y, (name, lam, eta, eta_y)


@pytest.mark.parametrize("name", sc.PCGS)
def test_pcg_reference_stop_is_stable(name):
    """The PCG steps are held to ob.pcg_solve's step count (max(2, 3 %)), which only means something where that count
    is not an accident of the stop threshold: PCG's residual is not monotone, and near the rounding regime (steps of
    the order of the rows) it can dip to just above 1e-6 ||b|| and take dozens of steps to come back, while a run with
    another order of summation dips just below and stops.  Two such runs' residuals differ by tens of percent there,
    so: with the threshold 1.5 x higher or lower, the oracle's count moves by no more than max(4, 3 %) -- on the
    oracle's own systems, at the initial lambda and at every rung of the ladder.  (4: where PCG still converges at a
    steady rate, that threshold change is worth its few steps -- log 1.5 / log(1 / rate), 4 at a rate of 0.9 -- which
    is no knife edge; the dips this guards against cost 18 to 33 steps on the windows that were turned down.)"""
    c, w = sc.CASES[name], sc.window(name)
    s = c["opts"].get("strategy", 0)
    S, bs = oracle_system(name)
    lam0 = c["opts"].get("lambda_init", 1e-5)
    systems = [(S, bs, lam0)]
    if c["first"] == "R":
        lam1, ni1 = sr.reject_update(lam0, 2.0, s)
        systems += [(S, bs, l) for l in sr.rung_lambdas(lam1, ni1, s, c["max_trials"])]
    else:
        o = ob.solve(w, max_iters=1, max_trials=1, n_threads=1, **sc.oracle_opts(name))
        S1, b1, _ = ob.reduced_system(dict(w, pose_Tcw=o["pose_Tcw"], lm_xyz=o["lm_xyz"]), n_threads=1, huber_delta=0.0,
                                      gate_mode=1)
        systems += [(sr.lower_symmetric(S1), b1, l) for l in sr.rung_lambdas(o["lambda_final"], 2.0, s, c["max_trials"])]
    for Sx, bx, lam in systems:
        A = sr.assemble(Sx, lam, s)
        lo, mid, hi = (ob.pcg_solve(A, bx, tol=t)[1] for t in (1.5e-6, 1e-6, 1e-6 / 1.5))
        print(f"PCGREF {name} lambda {lam:.3e}: steps {lo} / {mid} / {hi}")
        assert max(mid - lo, hi - mid) <= max(4, 0.03 * mid), (name, lam, lo, mid, hi)


@pytest.mark.parametrize("label", ["k_ctrl LDLT", "k_ctrl_b strategy 1"])
def test_rung_lambdas_are_the_oracles_rejections(label):
    kind, gen, opts, dec, _ = next(r for r in windows.RELIN_WINDOWS if r[0] == label)
    k = len(dec) - len(dec.lstrip("R"))
    assert k >= 3
    w = windows.relin_window(gen)
    s = opts.get("strategy", 0)
    lam0 = opts.get("lambda_init", 1e-5)
    seq = sr.rung_lambdas(lam0, 2.0, s, k + 1)
    for j in range(1, k + 1):
        o = ob.solve(w, max_iters=1, max_trials=j, n_threads=1, **opts)
        assert o["trials"] == j and o["accepted"] == 0
        assert o["lambda_final"] == seq[j], (j, o["lambda_final"], seq[j])
    # a ladder built after the first rejection: rung r is rejection r + 1
    lam1, ni1 = sr.reject_update(lam0, 2.0, s)
    assert sr.rung_lambdas(lam1, ni1, s, k) == seq[1:]


def _units_system(name):
    """S + lambda I of a case, its unit table from the planner's envelope, and the reference step."""
    S, bs = oracle_system(name)
    cfg = lego_ba.solve_config(sc.window(name))
    n = len(bs)
    band = cfg["controller"] == "k_ctrl_b"
    e = tcu.envelope_fcb(n, cfg["pf"])
    if band:
        fcb = e
    else:
        fcb = np.zeros(8, np.int32)
        fcb[:len(e)] = e
    units, _ = lego_ba.ctrl_units(n, fcb, band=band)
    A = sr.assemble(S, 2e-3, 0)
    free = sr.free_rows(A, bs)
    x_ref, _ = sr.solve_ld(A, bs, free)
    e_y, _ = sr.yardstick(A, bs, x_ref, free)
    return A, bs, units, band, free, x_ref, e_y


@pytest.mark.parametrize("name", ["lds_band", "b_p22"])
def test_criterion_has_teeth(name, monkeypatch):
    sc.set_env(monkeypatch, name)
    A, bs, units, band, free, x_ref, e_y = _units_system(name)
    steps = units.shape[1]
    tol = sr.bound(e_y)
    e_full = sr.forward_error(tcu.replay(A, bs, units, steps, band=band), x_ref, free)
    print(f"TEETH {name}: full table e {e_full:.2e} (yardstick {e_y:.2e}, bound {tol:.2e})")
    assert e_full <= tol
    # one valid unit word cleared: a unit wave of a middle step (never wave 0's, the diagonal tile)
    t = steps // 3 if not band else 5
    ws = [w for w in range(1, 16) if units[w, t] & tcu.VALID]
    assert ws, "the step has unit waves"
    cut = units.copy()
    cut[ws[len(ws) // 2], t] = 0
    e_cut = sr.forward_error(tcu.replay(A, bs, cut, steps, band=band), x_ref, free)
    # one tile row of that step replayed from the previous step's operands
    e_stale = sr.forward_error(tcu.replay(A, bs, units, steps, band=band, stale=(t, 1)), x_ref, free)
    print(f"TEETH {name}: unit cleared e {e_cut:.2e}, stale tile row e {e_stale:.2e}")
    assert e_cut > 1e3 * tol and e_stale > 1e3 * tol
