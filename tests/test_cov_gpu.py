"""lh_covariance on the device against tests/cov_ref.py's long-double covariances (include/lego_ba.h).

Test 1  values at the input state (max_iters = 0) on the cases below: pose_cov_full and lm_cov within
        max(8 x e(double, ref), 64 eps kappa_scaled) of the reference in the scaled error e(A, B) = max_ij |A_ij - B_ij|
        / sqrt(B_ii B_jj); e(double, ref) is the double evaluation's own distance on that case, computed at run time
        (the margin and the floor are tests/test_lin_system_gpu.py's, for the same reason: another valid order of
        operations; kappa_scaled on the floor is the forward-error shape of an inverse).  Exact: pose_cov[p] is block
        (p, p) of the full matrix by bits, the full matrix is its transpose by bits, held rows and columns are +0.0,
        n_free, bad_row == -1, 0 < min_pivot <= max_pivot.  A failing entry is named by its pose pair or landmark.
Test 2  at the returned state: allT and outl with max_iters = 2 stop on an accepted evaluate-only trial (iterations ==
        2, accepted == 2: the oracle's counts too), which commits the state and writes no system.  The reference is
        evaluated at the returned poses and landmarks; the reference at the previous accepted state (the max_iters = 1
        result) is asserted to lie more than 100 x the bound away, so a stale linearisation cannot pass.
Test 3  two calls return equal bits; asking for lm_cov does not change pose_cov's bits; solve_resident before and
        after a covariance call returns equal bits (poses, landmarks, rho0, trace).
Test 4  the statuses; after LH_E_SINGULAR the output arrays are untouched and the handle still solves.
Test 5  degenerate_guard = 1 with one landmark of `tiny` cut to a single observation: its nine values are NaN and
        every other value is within the bound of the reference with that landmark's edge dropped; guard 0 on the same
        window is LH_E_SINGULAR.

Measured e_GPU / e_double, Sigma_pp | Sigma_l (MI355X; also DESIGN.md 2.12).  Worst 2.19 (far: the landmark factor at
kappa(H_ll) = 6e6 against the reference's adjugate inverse), so the margin stays 8:

    case            n_free  kappa_scaled  test 1          test 2 (allT, outl), 5 (tiny)
    tiny            12      3.0e2         0.48 | 1.16     0.67 | 0.61
    allT            90      1.6e3         0.20 | 1.43     0.20 | 1.53
    fixedmid        84      4.3e2         0.14 | 0.45
    outl            54      8.0e2         0.10 | 0.53     0.00 | 1.50
    far             54      3.8e2         0.03 | 2.19
    cams4           42      4.7e2         0.44 | 0.14
    allT_anchor5    90      1.0e3         0.14 | 0.63
    p30             174     9.7e3         0.12 | 0.26
    p64             378     6.7e4         0.01 | 1.00

The free gauge (allT, no fixed pose, no anchor) fails at row 90 of 96 with pivots 5.9e2 .. 2.9e6 before it.
"""
import numpy as np
import pytest

import cov_ref
import lego_ba
import lin_cases

pytestmark = pytest.mark.gpu

def _free_gauge():
    w, chunk, opts, _ = lin_cases.case("allT")
    return dict(w, pose_fixed=None), chunk, opts


def _gen_case(**kw):
    return lambda: (lin_cases._gen(**kw), 16, dict(gate_mode=1))


# id: (window, chunk_landmarks, solver options), the anchor, n_free
CASES = {
    "tiny": (lambda: lin_cases.case("tiny")[:3], -1, 12),
    "allT": (lambda: lin_cases.case("allT")[:3], -1, 90),
    "fixedmid": (lambda: lin_cases.case("fixedmid")[:3], -1, 84),
    "outl": (lambda: lin_cases.case("outl")[:3], -1, 54),
    "far": (lambda: lin_cases.case("far")[:3], -1, 54),
    "cams4": (lambda: lin_cases.case("cams4")[:3], -1, 42),
    "allT_anchor5": (_free_gauge, 5, 90),
    "p30": (_gen_case(P=30, L=240, k=2, k_max=16, pose_mode=1, seed=4), -1, 174),   # n > 128: the planner chooses k_ctrl_g
    "p64": (_gen_case(P=64, L=400, k=2, k_max=8, pose_mode=0, seed=5), -1, 378),    # the envelope's edge
}

_win, _refs, _runs = {}, {}, {}


def window(name):
    if name not in _win:
        _win[name] = CASES[name][0]()
    return _win[name]


def huber(opts):
    return opts.get("huber_delta", 5.991)


def references(key, w, opts, anchor, pose=None, lm=None):
    """(long-double reference, double evaluation's distances (pose, landmarks)) once per key."""
    if key not in _refs:
        ref = cov_ref.covariance(w, pose=pose, lm=lm, huber_delta=huber(opts), anchor=anchor)
        dbl = cov_ref.covariance(w, pose=pose, lm=lm, huber_delta=huber(opts), anchor=anchor, dtype=np.float64)
        e_p = cov_ref.pose_error(dbl["pose_full"], ref["pose_full"], ref["free"])[0]
        e_l = cov_ref.lm_error(dbl["lm"], ref["lm"])[0]
        _refs[key] = (ref, (e_p, e_l))
    return _refs[key]


def run(name):
    """The case solved with max_iters = 0 and three covariance calls (all arrays, all arrays again, no landmarks):
    once per case, shared by tests 1 and 3."""
    if name not in _runs:
        w, chunk, opts = window(name)
        s = lego_ba.Solver(max_iters=0, chunk_landmarks=chunk, **opts)
        try:
            g = s.solve(w)
            assert g["degenerate"] == 0
            a = CASES[name][1]
            _runs[name] = (s.controller(), s.covariance(anchor=a, full=True, landmarks=True),
                           s.covariance(anchor=a, full=True, landmarks=True), s.covariance(anchor=a, full=True))
        finally:
            s.close()
    return _runs[name]


def check_exact(name, c, held, n_free):
    P = len(held)
    full = c["pose_cov_full"]
    assert c["n_free"] == n_free and c["bad_row"] == -1, (c["n_free"], c["bad_row"])
    assert 0 < c["min_pivot"] <= c["max_pivot"], (c["min_pivot"], c["max_pivot"])
    assert np.array_equal(full.view(np.uint64), full.T.copy().view(np.uint64)), f"{name}: Sigma_pp is not its transpose by bits"
    for p in range(P):
        blk = full[6 * p:6 * p + 6, 6 * p:6 * p + 6]
        assert np.array_equal(c["pose_cov"][p].view(np.uint64), np.ascontiguousarray(blk).view(np.uint64)), \
            f"{name}: pose_cov[{p}] is not block ({p}, {p}) of the full matrix"
    hr = np.repeat(held, 6)
    z = np.concatenate([full[hr].ravel(), full[:, hr].ravel()])
    assert not z.view(np.uint64).any(), f"{name}: a held pose's row or column is not +0.0"
    if c.get("lm_cov") is not None:
        lc = c["lm_cov"]
        assert np.array_equal(lc.view(np.uint64), lc.transpose(0, 2, 1).copy().view(np.uint64)), f"{name}: a Sigma_l is not symmetric by bits"


def check_values(tag, name, c, ref, e_dbl):
    """pose_cov_full and lm_cov of result c against reference `ref`; e_dbl: the double evaluation's distances."""
    e_p, pq = cov_ref.pose_error(c["pose_cov_full"], ref["pose_full"], ref["free"])
    tol_p = cov_ref.tolerance(e_dbl[0], ref["kappa"])
    e_l, l = cov_ref.lm_error(c["lm_cov"], ref["lm"])
    tol_l = cov_ref.tolerance(e_dbl[1], ref["kappa"])
    print(f"RATIO {tag} {name}: n_free {len(ref['free'])} kappa_scaled {ref['kappa']:.1e} | Sigma_pp e_gpu {e_p:.2e} "
          f"e_double {e_dbl[0]:.2e} ratio {e_p / e_dbl[0]:.2f} bound {tol_p:.2e} (poses {pq}) | Sigma_l e_gpu {e_l:.2e} "
          f"e_double {e_dbl[1]:.2e} ratio {e_l / e_dbl[1]:.2f} bound {tol_l:.2e} (landmark {l}) | pivots "
          f"{c['min_pivot']:.2e} .. {c['max_pivot']:.2e} | device {c['time_ms']:.3f} ms")
    assert e_p <= tol_p, f"{name}: Sigma_pp entry of pose pair {pq}: e = {e_p:.3e} > {tol_p:.3e} ({e_p / e_dbl[0]:.1f} x the double evaluation's)"
    assert e_l <= tol_l, f"{name}: Sigma_l of landmark {l}: e = {e_l:.3e} > {tol_l:.3e} ({e_l / e_dbl[1]:.1f} x the double evaluation's)"


@pytest.mark.parametrize("name", list(CASES))
def test_values_at_the_input_state(name):
    """Test 1."""
    w, _, opts = window(name)
    anchor, n_free = CASES[name][1:]
    ref, e_dbl = references(name, w, opts, anchor)
    assert len(ref["free"]) == n_free
    kind, c, _, _ = run(name)
    if name == "p30":
        assert kind == "k_ctrl_g", "the planner no longer chooses k_ctrl_g for this window"
    check_exact(name, c, ref["held"], n_free)
    check_values("1", name, c, ref, e_dbl)


@pytest.mark.parametrize("name", ["allT", "outl"])
def test_values_at_the_returned_state(name):
    """Test 2."""
    w, chunk, opts = window(name)
    states = {}
    for mi in (1, 2):
        s = lego_ba.Solver(max_iters=mi, chunk_landmarks=chunk, **opts)
        try:
            g = s.solve(w)
            assert g["iterations"] == mi and g["accepted"] == mi, (mi, g["iterations"], g["accepted"])
            states[mi] = (g["pose_Tcw"], g["lm_xyz"], s.covariance(full=True, landmarks=True) if mi == 2 else None)
        finally:
            s.close()
    pose, lm, c = states[2]
    ref, e_dbl = references(name + "@2", w, opts, -1, pose=pose, lm=lm)
    check_exact(name, c, ref["held"], len(ref["free"]))
    check_values("2", name, c, ref, e_dbl)
    # teeth: the covariance at the previous accepted state is far outside the bound
    stale = cov_ref.covariance(w, pose=states[1][0], lm=states[1][1], huber_delta=huber(opts), dtype=np.float64)
    d_p = cov_ref.pose_error(stale["pose_full"], ref["pose_full"], ref["free"])[0]
    d_l = cov_ref.lm_error(stale["lm"], ref["lm"])[0]
    print(f"TEETH {name}: the previous state's covariances lie {d_p:.2e} | {d_l:.2e} away")
    assert d_p > 100 * cov_ref.tolerance(e_dbl[0], ref["kappa"]) and d_l > 100 * cov_ref.tolerance(e_dbl[1], ref["kappa"])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("name", ["tiny", "outl", "p30"])
def test_two_calls_and_the_landmark_request_change_no_bits(name):
    """Test 3, the calls among themselves."""
    _, c1, c2, c3 = run(name)
    for k in ("pose_cov", "pose_cov_full", "lm_cov"):
        assert np.array_equal(_bits(c1[k]), _bits(c2[k])), f"{name}: {k} differs between two calls"
    for k in ("pose_cov", "pose_cov_full"):
        assert np.array_equal(_bits(c1[k]), _bits(c3[k])), f"{name}: {k} changes when lm_cov is asked for"
    assert c3["lm_cov"] is None and (c1["min_pivot"], c1["max_pivot"]) == (c3["min_pivot"], c3["max_pivot"])


@pytest.mark.parametrize("name,guard", [("allT", 0), ("outl", 1), ("p30", 0)])
def test_a_covariance_call_changes_no_later_solve(name, guard):
    """Test 3, solve_resident around a call (the default max_iters: ladder, batches and evaluate-only trials all run).
    outl runs with degenerate_guard = 1: its fifth accepted state has a landmark whose H_ll is not positive definite,
    so with guard 0 every later trial is rejected, as in the reference, and lh_covariance answers LH_E_SINGULAR
    there, as defined; with guard 1 that landmark is held fixed and its covariance is NaN."""
    w, chunk, opts = window(name)
    s = lego_ba.Solver(chunk_landmarks=chunk, degenerate_guard=guard, **opts)
    try:
        s.upload(w)
        r1 = s.solve_resident(want_states=True, want_edges=True)
        sys1, _ = s.reduced_system(1)
        c = s.covariance(full=True, landmarks=True)
        sys2, _ = s.reduced_system(1)
        r2 = s.solve_resident(want_states=True, want_edges=True)
    finally:
        s.close()
    assert c["bad_row"] == -1
    assert np.array_equal(_bits(sys1), _bits(sys2)), "the committed reduced system changed under lh_covariance"
    for k in ("pose_Tcw", "lm_xyz", "edge_robust_chi2", "trace_chi2", "trace_lambda"):
        assert np.array_equal(_bits(r1[k]), _bits(r2[k])), f"{name}: {k} differs after a covariance call"
    assert (r1["iterations"], r1["trials"], r1["accepted"]) == (r2["iterations"], r2["trials"], r2["accepted"])


def _status(s, **kw):
    with pytest.raises(lego_ba.LhError) as ei:
        s.covariance(**kw)
    return ei.value


def test_statuses():
    """Test 4."""
    w, chunk, opts = window("tiny")
    s = lego_ba.Solver(max_iters=0, chunk_landmarks=chunk, **opts)
    try:
        assert _status(s).status == lego_ba.LH_E_STATE          # before any solve
        s.upload(w)
        assert _status(s).status == lego_ba.LH_E_STATE          # a window, no solve of it
        s.solve(w)
        assert _status(s, anchor=w["n_poses"]).status == lego_ba.LH_E_BADARG
        assert _status(s, anchor=-2).status == lego_ba.LH_E_BADARG
        assert s.covariance(anchor=1)["n_free"] == 6             # (fixed pose 0 and the anchor held)
        s.solve(dict(w, pose_fixed=np.ones(w["n_poses"], np.uint8)))
        e = _status(s)
        assert e.status == lego_ba.LH_E_SINGULAR and e.result["n_free"] == 0
    finally:
        s.close()
    w70, chunk70, opts70, _ = lin_cases.case("p70")
    s = lego_ba.Solver(max_iters=0, chunk_landmarks=chunk70, **opts70)
    try:
        s.solve(w70)
        assert _status(s).status == lego_ba.LH_E_UNSUPPORTED
    finally:
        s.close()


def test_free_gauge_is_reported_singular():
    """Test 4: allT without a fixed pose and without an anchor; the arrays keep their sentinel; the handle still solves."""
    w, chunk, opts = window("allT_anchor5")
    P, L = w["n_poses"], len(w["lm_xyz"])
    s = lego_ba.Solver(max_iters=0, chunk_landmarks=chunk, **opts)
    try:
        s.solve(w)
        out = dict(pose_cov=np.full((P, 6, 6), -7.0), pose_cov_full=np.full((6 * P, 6 * P), -7.0), lm_cov=np.full((L, 3, 3), -7.0))
        with pytest.raises(lego_ba.LhError) as ei:
            s.covariance(full=True, landmarks=True, out=out)
        assert ei.value.status == lego_ba.LH_E_SINGULAR
        r = ei.value.result
        print(f"free gauge: bad_row {r['bad_row']} of {6 * P}, pivots {r['min_pivot']:.2e} .. {r['max_pivot']:.2e}")
        assert 0 <= r["bad_row"] < 6 * P and r["n_free"] == 6 * P
        assert all((a == -7.0).all() for a in out.values()), "an output array was written on LH_E_SINGULAR"
        g = s.solve(w)
        assert g["degenerate"] == 0
        assert s.covariance(anchor=5)["bad_row"] == -1
    finally:
        s.close()


def test_degenerate_landmark():
    """Test 5."""
    w, chunk, opts = window("tiny")
    ol = np.asarray(w["obs_lm"])
    l = int(np.flatnonzero(np.bincount(ol) >= 3)[0])
    mine = np.flatnonzero(ol == l)

    def without(drop):
        keep = np.ones(len(ol), bool)
        keep[drop] = False
        return dict(w, **{k: np.asarray(w[k])[keep] for k in ("obs_pose", "obs_lm", "obs_cam", "obs_uv")})

    w1, w0 = without(mine[1:]), without(mine)   # one observation left; none (the reference: no vertex)
    s = lego_ba.Solver(max_iters=0, chunk_landmarks=chunk, degenerate_guard=1, **opts)
    try:
        g = s.solve(w1)
        assert g["degenerate"] == 1
        c = s.covariance(full=True, landmarks=True)
    finally:
        s.close()
    assert np.isnan(c["lm_cov"][l]).all(), c["lm_cov"][l]
    ref, e_dbl = references("tiny-deg", w0, opts, -1)
    assert np.isnan(ref["lm"][l].astype(np.float64)).all()
    check_exact("tiny-deg", c, ref["held"], 12)
    check_values("5", "tiny-deg", c, ref, e_dbl)
    s = lego_ba.Solver(max_iters=0, chunk_landmarks=chunk, degenerate_guard=0, **opts)
    try:
        s.solve(w1)
        assert _status(s, landmarks=True).status == lego_ba.LH_E_SINGULAR
    finally:
        s.close()
