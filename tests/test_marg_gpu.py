"""lh_marginalize on the device against tests/marg_ref.py's long-double priors (include/lego_ba.h).

Windows come from tests/lin_cases.py with its chunk sizes and gate_mode = 1 (p30 and p64: tests/test_cov_gpu.py's
generators), max_iters = 0 unless stated.  H_prior is compared in e(A, B) = max_ij |A_ij - B_ij| / sqrt(B_ii B_jj) over
the rows whose reference diagonal is not zero, b_prior in max_i |b_i - B_i| / sqrt(H_ii) over max_i |B_i| / sqrt(H_ii)
(marg_ref.rhs_error).  The bound of both is cov_ref.tolerance's: max(8 x the double evaluation's own distance on that
case, computed at run time, 64 eps kappa), kappa the scaled condition number of the eliminated 6x6 block (1 for a fixed
m, where nothing is eliminated).

Test 1  values on the cases below.  Exact: H_prior is its transpose by bits; the rows and columns of m, of the fixed
        poses and of the poses that share no landmark with m are +0.0 (H_prior and b_prior); lm_marginalised,
        n_landmarks, n_edges, n_degenerate equal the reference's; bad_row == -1; 0 < min_pivot <= max_pivot (both 0 for
        a fixed m).  A failing entry is named by its pose pair.
Test 2  teeth.  On allT m = 1 the reference formed from all landmarks, and from the edges to m alone (the reference
        routine's choice), each lie more than 100 x the bound away.  At the returned state (allT m = 1, outl m = 9,
        max_iters = 2) the values are within the bound and the reference at the previous accepted state lies more than
        100 x the bound away.
Test 3  an earlier prior (allT m = 1, a random SPD prior_H of the size of A's diagonal and a random prior_b): within
        the same bound; garbage in prior_H's strict upper triangle changes no bit.
Test 4  two calls return equal bits; solve_resident (default iterations), reduced_system(1) and
        covariance(full, landmarks) before and after a call are equal by bits (allT, outl with guard 1, p30).
Test 5  the statuses; a window in which m's landmarks are seen by m alone: guard 1 LH_OK with an all-zero prior and
        n_degenerate == n_landmarks, guard 0 LH_E_SINGULAR with the output arrays untouched and a handle that still
        solves.
Test 6  one landmark of tiny that m observes cut to its single edge to m: guard 1, n_degenerate == 1, the values
        within the bound of the reference with that landmark held fixed (its H_pp and b_p stay, its Schur terms go).

Measured e_GPU / e_double, H_prior | b_prior (MI355X; also DESIGN.md 2.13; printed by `pytest -s`, lines RATIO).  Worst
5.72, where m is fixed and nothing is eliminated (k_lin + k_reduce's own sums against the plain double evaluation);
1.81 where a pose is eliminated (far), so the margin stays 8:

    case            m    landmarks (edges)  rows  kappa    test 1          tests 2, 3, 6
    tiny            1    9 (25)             6     5.6e1    0.63 | 1.32     0.30 | 0.41  (6: one landmark cut to one edge)
    tiny            2    9 (25)             6     6.1e1    0.42 | 0.35
    allT            1    51 (558)           84    8.4e1    0.35 | 0.87     0.78 | 0.82  (2);  0.45 | 1.07  (3, kappa 3.3)
    allT            15   55 (578)           84    1.2e1    0.75 | 1.07
    fixedmid        1    51 (558)           78    8.4e1    0.35 | 0.87
    fixedmid        7    51 (571)           84    1        5.72 | 0.83
    outl            9    73 (516)           48    2.0e1    0.36 | 0.73     0.72 | 1.12  (2)
    far             1    66 (488)           48    8.3      1.81 | 1.12
    cams4           1    64 (512)           36    4.2e1    1.23 | 0.41
    nohuber         1    51 (558)           84    8.4e1    0.28 | 0.87
    p30             15   68 (736)           168   1.1e2    1.19 | 0.62
    p64             32   35 (190)           84    5.1e1    0.75 | 0.66

The prior from all landmarks lies 0.96 | 0.78 from the reference, the one from the edges to m alone 1.0 | 1.0, the one
at the previous accepted state 3.9e-3 | 0.11 (allT) and 5.5e-2 | 0.61 (outl).
"""
import ctypes as C

import numpy as np
import pytest

import lego_ba
import lin_cases
import marg_ref
from test_cov_gpu import CASES as COV_CASES

pytestmark = pytest.mark.gpu


def _lin(name):
    return lambda: lin_cases.case(name)[:3]


# id: (window, chunk_landmarks, solver options), m
CASES = {
    "tiny-m1": (_lin("tiny"), 1), "tiny-m2": (_lin("tiny"), 2),
    "allT-m1": (_lin("allT"), 1), "allT-m15": (_lin("allT"), 15),
    "fixedmid-m1": (_lin("fixedmid"), 1), "fixedmid-m7": (_lin("fixedmid"), 7),   # (7 is fixed: conditioning)
    "outl-m9": (_lin("outl"), 9), "far-m1": (_lin("far"), 1), "cams4-m1": (_lin("cams4"), 1),
    "nohuber-m1": (_lin("nohuber"), 1),
    "p30-m15": (COV_CASES["p30"][0], 15), "p64-m32": (COV_CASES["p64"][0], 32),
}

_win, _refs, _runs = {}, {}, {}


def window(name):
    if name not in _win:
        _win[name] = CASES[name][0]()
    return _win[name]


def huber(opts):
    return opts.get("huber_delta", 5.991)


def references(key, w, opts, m, **kw):
    """(long-double reference, the double evaluation's distances (H, b)) once per key."""
    if key not in _refs:
        ref = marg_ref.marginalize(w, m, huber_delta=huber(opts), **kw)
        dbl = marg_ref.marginalize(w, m, huber_delta=huber(opts), dtype=np.float64, **kw)
        e_H = marg_ref.pose_error(dbl["H"], ref["H"], ref["rows"])[0] if len(ref["rows"]) else 0.0
        e_b = marg_ref.rhs_error(dbl["b"], ref)[0] if len(ref["rows"]) else 0.0
        _refs[key] = (ref, (e_H, e_b))
    return _refs[key]


def run(name):
    """The case solved with max_iters = 0 and two marginalize calls: once per case, shared by tests 1, 2 and 4."""
    if name not in _runs:
        w, chunk, opts = window(name)
        s = lego_ba.Solver(max_iters=0, chunk_landmarks=chunk, **opts)
        try:
            g = s.solve(w)
            assert g["degenerate"] == 0
            m = CASES[name][1]
            _runs[name] = (s.marginalize(m), s.marginalize(m))
        finally:
            s.close()
    return _runs[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check_exact(name, c, ref, m, prior=False):
    H, b = c["H_prior"], c["b_prior"]
    n = H.shape[0]
    assert c["bad_row"] == -1, c["bad_row"]
    if ref["fixed"][m]:
        assert c["min_pivot"] == 0.0 and c["max_pivot"] == 0.0, (c["min_pivot"], c["max_pivot"])
    else:
        assert 0 < c["min_pivot"] <= c["max_pivot"], (c["min_pivot"], c["max_pivot"])
    assert np.array_equal(_bits(H), _bits(H.T.copy())), f"{name}: H_prior is not its transpose by bits"
    zero = np.ones(n, bool)
    zero[ref["rows"]] = False
    assert zero[6 * m:6 * m + 6].all() and np.repeat(ref["fixed"], 6)[~zero].sum() == 0
    if not prior:   # (with an earlier prior its entries pass through on the poses M does not reach)
        z = np.concatenate([H[zero].ravel(), H[:, zero].ravel(), b[zero]])
        assert not _bits(z).any(), f"{name}: a row or column of m, a fixed pose or an uninvolved pose is not +0.0"
    assert np.array_equal(c["lm_marginalised"], ref["in_M"]), f"{name}: lm_marginalised"
    got = (c["n_landmarks"], c["n_edges"], c["n_degenerate"])
    assert got == (ref["n_landmarks"], ref["n_edges"], ref["n_degenerate"]), (name, got)


def check_values(tag, name, c, ref, e_dbl):
    rows = ref["rows"]
    e_H, pq = marg_ref.pose_error(c["H_prior"], ref["H"], rows)
    e_b, pb = marg_ref.rhs_error(c["b_prior"], ref)
    tol_H, tol_b = marg_ref.tolerance(e_dbl[0], ref["kappa"]), marg_ref.tolerance(e_dbl[1], ref["kappa"])
    print(f"RATIO {tag} {name}: landmarks {ref['n_landmarks']} edges {ref['n_edges']} rows {len(rows)} kappa {ref['kappa']:.1e} | "
          f"H_prior e_gpu {e_H:.2e} e_double {e_dbl[0]:.2e} ratio {e_H / max(e_dbl[0], 1e-300):.2f} bound {tol_H:.2e} (poses {pq}) | "
          f"b_prior e_gpu {e_b:.2e} e_double {e_dbl[1]:.2e} ratio {e_b / max(e_dbl[1], 1e-300):.2f} bound {tol_b:.2e} (pose {pb}) | "
          f"pivots {c['min_pivot']:.2e} .. {c['max_pivot']:.2e} | device {c['time_ms']:.3f} ms")
    assert e_H <= tol_H, f"{name}: H_prior entry of pose pair {pq}: e = {e_H:.3e} > {tol_H:.3e} ({e_H / max(e_dbl[0], 1e-300):.1f} x the double evaluation's)"
    assert e_b <= tol_b, f"{name}: b_prior row of pose {pb}: e = {e_b:.3e} > {tol_b:.3e} ({e_b / max(e_dbl[1], 1e-300):.1f} x the double evaluation's)"


@pytest.mark.parametrize("name", list(CASES))
def test_values_at_the_input_state(name):
    """Test 1."""
    w, _, opts = window(name)
    m = CASES[name][1]
    ref, e_dbl = references(name, w, opts, m)
    c, _ = run(name)
    check_exact(name, c, ref, m)
    check_values("1", name, c, ref, e_dbl)


def test_other_landmark_sets_are_far_away():
    """Test 2, the landmark set."""
    name, m = "allT-m1", 1
    w, _, opts = window(name)
    ref, e_dbl = references(name, w, opts, m)
    tol_H, tol_b = marg_ref.tolerance(e_dbl[0], ref["kappa"]), marg_ref.tolerance(e_dbl[1], ref["kappa"])
    for edges in ("all", "to_m"):
        other = marg_ref.marginalize(w, m, huber_delta=huber(opts), dtype=np.float64, edges=edges)
        d_H = marg_ref.pose_error(other["H"], ref["H"], ref["rows"])[0]
        d_b = marg_ref.rhs_error(other["b"], ref)[0]
        print(f"TEETH {name}: the prior from edges '{edges}' lies {d_H:.2e} | {d_b:.2e} from the reference")
        assert d_H > 100 * tol_H and d_b > 100 * tol_b, (edges, d_H, d_b)


@pytest.mark.parametrize("name", ["allT-m1", "outl-m9"])
def test_values_at_the_returned_state(name):
    """Test 2, the state."""
    w, chunk, opts = window(name)
    m = CASES[name][1]
    states = {}
    for mi in (1, 2):
        s = lego_ba.Solver(max_iters=mi, chunk_landmarks=chunk, **opts)
        try:
            g = s.solve(w)
            assert g["iterations"] == mi and g["accepted"] == mi, (mi, g["iterations"], g["accepted"])
            states[mi] = (g["pose_Tcw"], g["lm_xyz"], s.marginalize(m) if mi == 2 else None)
        finally:
            s.close()
    pose, lm, c = states[2]
    ref, e_dbl = references(name + "@2", w, opts, m, pose=pose, lm=lm)
    check_exact(name, c, ref, m)
    check_values("2", name, c, ref, e_dbl)
    stale = marg_ref.marginalize(w, m, pose=states[1][0], lm=states[1][1], huber_delta=huber(opts), dtype=np.float64)
    d_H = marg_ref.pose_error(stale["H"], ref["H"], ref["rows"])[0]
    d_b = marg_ref.rhs_error(stale["b"], ref)[0]
    print(f"TEETH {name}: the previous state's prior lies {d_H:.2e} | {d_b:.2e} away")
    assert d_H > 100 * marg_ref.tolerance(e_dbl[0], ref["kappa"]) and d_b > 100 * marg_ref.tolerance(e_dbl[1], ref["kappa"])


def test_earlier_prior():
    """Test 3."""
    name, m = "allT-m1", 1
    w, chunk, opts = window(name)
    P = w["n_poses"]
    A0, b0, _ = marg_ref.system(w, m, huber_delta=huber(opts), dtype=np.float64)
    H0, g0 = marg_ref.random_prior(P, A0, b0, seed=11)
    ref, e_dbl = references(name + "+prior", w, opts, m, prior=(H0, g0))
    garbage = np.tril(H0) + np.triu(np.random.default_rng(5).standard_normal(H0.shape) * 1e9, 1)
    s = lego_ba.Solver(max_iters=0, chunk_landmarks=chunk, **opts)
    try:
        s.solve(w)
        c = s.marginalize(m, prior=(H0, g0))
        c2 = s.marginalize(m, prior=(garbage, g0))
    finally:
        s.close()
    check_exact(name, c, ref, m, prior=True)
    check_values("3", name + "+prior", c, ref, e_dbl)
    for k in ("H_prior", "b_prior"):
        assert np.array_equal(_bits(c[k]), _bits(c2[k])), f"{k} depends on prior_H's strict upper triangle"
    fixed = np.repeat(ref["fixed"], 6)
    assert not _bits(c["H_prior"][fixed]).any() and not _bits(c["b_prior"][fixed]).any()


@pytest.mark.parametrize("name", ["tiny-m1", "outl-m9", "p30-m15"])
def test_two_calls_return_equal_bits(name):
    """Test 4, the calls among themselves."""
    c1, c2 = run(name)
    for k in ("H_prior", "b_prior"):
        assert np.array_equal(_bits(c1[k]), _bits(c2[k])), f"{name}: {k} differs between two calls"
    assert np.array_equal(c1["lm_marginalised"], c2["lm_marginalised"])
    for k in ("n_landmarks", "n_edges", "n_degenerate", "min_pivot", "max_pivot"):
        assert c1[k] == c2[k], k


@pytest.mark.parametrize("name,guard", [("allT-m1", 0), ("outl-m9", 1), ("p30-m15", 0)])
def test_a_call_changes_nothing_later(name, guard):
    """Test 4, solve_resident, the committed reduced system and lh_covariance around two calls (the default max_iters:
    ladder, batches and evaluate-only trials all run; outl with guard 1 as in tests/test_cov_gpu.py)."""
    w, chunk, opts = window(name)
    m = CASES[name][1]
    s = lego_ba.Solver(chunk_landmarks=chunk, degenerate_guard=guard, **opts)
    try:
        s.upload(w)
        r1 = s.solve_resident(want_states=True, want_edges=True)
        sys1, _ = s.reduced_system(1)
        v1 = s.covariance(full=True, landmarks=True)
        c1 = s.marginalize(m)
        c2 = s.marginalize(m)
        sys2, _ = s.reduced_system(1)
        v2 = s.covariance(full=True, landmarks=True)
        r2 = s.solve_resident(want_states=True, want_edges=True)
        c3 = s.marginalize(m)
    finally:
        s.close()
    assert c1["bad_row"] == -1
    for k in ("H_prior", "b_prior"):
        assert np.array_equal(_bits(c1[k]), _bits(c2[k])) and np.array_equal(_bits(c1[k]), _bits(c3[k])), f"{name}: {k}"
    assert np.array_equal(_bits(sys1), _bits(sys2)), "the committed reduced system changed under lh_marginalize"
    for k in ("pose_cov", "pose_cov_full", "lm_cov"):
        assert np.array_equal(_bits(v1[k]), _bits(v2[k])), f"{name}: lh_covariance's {k} differs after a marginalize call"
    for k in ("pose_Tcw", "lm_xyz", "edge_robust_chi2", "trace_chi2", "trace_lambda"):
        assert np.array_equal(_bits(r1[k]), _bits(r2[k])), f"{name}: {k} differs after a marginalize call"
    assert (r1["iterations"], r1["trials"], r1["accepted"]) == (r2["iterations"], r2["trials"], r2["accepted"])


def _status(s, *a, **kw):
    with pytest.raises(lego_ba.LhError) as ei:
        s.marginalize(*a, **kw)
    return ei.value


def test_statuses():
    """Test 5."""
    w, chunk, opts = lin_cases.case("tiny")[:3]
    P = w["n_poses"]
    s = lego_ba.Solver(max_iters=0, chunk_landmarks=chunk, **opts)
    try:
        assert _status(s, 1).status == lego_ba.LH_E_STATE          # before any solve
        s.upload(w)
        assert _status(s, 1).status == lego_ba.LH_E_STATE          # a window, no solve of it
        s.solve(w)
        assert _status(s, -1).status == lego_ba.LH_E_BADARG
        assert _status(s, P).status == lego_ba.LH_E_BADARG
        H, b = np.zeros((6 * P, 6 * P)), np.zeros(6 * P)
        for pH, pb in ((H, None), (None, b)):   # one prior pointer without the other
            i, r = lego_ba.LhMargInput(1), lego_ba.LhMargResult()
            i.prior_H, i.prior_b = lego_ba._ptr(pH), lego_ba._ptr(pb)
            oH, ob = np.zeros((6 * P, 6 * P)), np.zeros(6 * P)
            r.H_prior, r.b_prior = lego_ba._ptr(oH), lego_ba._ptr(ob)
            assert lego_ba.ba_lib().lh_marginalize(s.h, C.byref(i), C.byref(r)) == lego_ba.LH_E_BADARG
        assert s.marginalize(1)["bad_row"] == -1
    finally:
        s.close()
    w70, chunk70, opts70, _ = lin_cases.case("p70")
    s = lego_ba.Solver(max_iters=0, chunk_landmarks=chunk70, **opts70)
    try:
        s.solve(w70)
        assert _status(s, 1).status == lego_ba.LH_E_UNSUPPORTED
    finally:
        s.close()


def _cut(w, drop):
    keep = np.ones(len(w["obs_pose"]), bool)
    keep[drop] = False
    return marg_ref.restrict(w, keep)


def test_landmarks_seen_by_m_alone():
    """Test 5: tiny with every edge from another pose to a landmark that pose 2 observes removed."""
    w, chunk, opts = lin_cases.case("tiny")[:3]
    m, P, L = 2, w["n_poses"], len(w["lm_xyz"])
    op, ol = np.asarray(w["obs_pose"], np.int64), np.asarray(w["obs_lm"], np.int64)
    wa = _cut(w, np.flatnonzero(marg_ref.landmark_set(w, m)[ol] & (op != m)))
    n_m = int(marg_ref.landmark_set(wa, m).sum())
    assert n_m > 0
    s = lego_ba.Solver(max_iters=0, chunk_landmarks=chunk, degenerate_guard=1, **opts)
    try:
        s.solve(wa)
        c = s.marginalize(m)
    finally:
        s.close()
    assert c["bad_row"] == -1 and c["n_landmarks"] == n_m and c["n_degenerate"] == n_m and c["n_edges"] == n_m
    assert not _bits(c["H_prior"]).any() and not _bits(c["b_prior"]).any(), "the prior is not all +0.0"
    assert 0 < c["min_pivot"] <= c["max_pivot"]
    s = lego_ba.Solver(max_iters=0, chunk_landmarks=chunk, degenerate_guard=0, **opts)
    try:
        s.solve(wa)
        out = dict(H_prior=np.full((6 * P, 6 * P), -7.0), b_prior=np.full(6 * P, -7.0), lm_marginalised=np.full(L, 9, np.uint8))
        with pytest.raises(lego_ba.LhError) as ei:
            s.marginalize(m, out=out)
        assert ei.value.status == lego_ba.LH_E_SINGULAR and ei.value.result["n_degenerate"] == n_m
        assert (out["H_prior"] == -7.0).all() and (out["b_prior"] == -7.0).all() and (out["lm_marginalised"] == 9).all(), \
            "an output array was written on LH_E_SINGULAR"
        g = s.solve(w)
        assert g["degenerate"] == 0 and s.marginalize(m)["bad_row"] == -1
    finally:
        s.close()


def test_degenerate_landmark_in_M():
    """Test 6."""
    w, chunk, opts = lin_cases.case("tiny")[:3]
    m = 1
    op, ol = np.asarray(w["obs_pose"], np.int64), np.asarray(w["obs_lm"], np.int64)
    cand = np.flatnonzero(marg_ref.landmark_set(w, m) & (np.bincount(ol, minlength=len(w["lm_xyz"])) >= 2))
    l = int(cand[0])
    w1 = _cut(w, np.flatnonzero((ol == l) & (op != m)))
    s = lego_ba.Solver(max_iters=0, chunk_landmarks=chunk, degenerate_guard=1, **opts)
    try:
        g = s.solve(w1)
        assert g["degenerate"] == 1
        c = s.marginalize(m)
    finally:
        s.close()
    ref, e_dbl = references("tiny-deg", w1, opts, m)
    assert ref["n_degenerate"] == 1 and ref["in_M"][l]
    check_exact("tiny-deg", c, ref, m)
    check_values("6", "tiny-deg", c, ref, e_dbl)
    # the landmark's H_pp stays: the reference without its edge lies outside the bound
    w0 = _cut(w, np.flatnonzero(ol == l))
    gone = marg_ref.marginalize(w0, m, huber_delta=huber(opts), dtype=np.float64)
    d_H = marg_ref.pose_error(gone["H"], ref["H"], ref["rows"])[0]
    print(f"TEETH tiny-deg: the prior without the landmark's edge lies {d_H:.2e} away")
    assert d_H > 100 * marg_ref.tolerance(e_dbl[0], ref["kappa"])
