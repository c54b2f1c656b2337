"""marg_ref -- a keyframe of one window marginalised into a pose prior, in np.longdouble (TEST INFRASTRUCTURE).

What lh_marginalize (include/lego_ba.h) computes, from tests/lin_ref.py's linearisation.  With m the
pose to marginalise and M the landmarks with an edge to m:

    A, b        lin_ref.linearise's S and bs of the window restricted to the edges of M's landmarks (to every pose they
                reach), plus the earlier prior with the fixed poses' rows and columns zeroed;
    H_prior     A[r, r] - A[r, m] A[m, m]^-1 A[m, r], b_prior = b[r] - A[r, m] A[m, m]^-1 b[m], r the other poses' rows,
                laid out over all 6P rows with m's zero; a fixed m: A[r, r] and b[r] (nothing is eliminated).

A landmark of M with fewer than two edges has a rank-deficient H_ll.  It is treated as the solver's linearisation
treats it under degenerate_guard = 1 (k_lin: the landmark is held fixed): its Schur terms H_pl H_ll^-1 H_lp and
H_pl H_ll^-1 b_l are dropped, its edges' H_pp and b_p stay.  lin_ref.linearise inverts every H_ll, so it is called
here with its 3x3 inverse replaced, for the duration of the call, by one that answers zero for those landmarks: a zero
H_ll^-1 drops exactly the two Schur terms.

The reference (dtype np.longdouble) inverts A[m, m] with cov_ref.invert; the double evaluation (dtype np.float64) is
the same statements in double, the unit of the GPU's tolerance.  lin_ref models gate_mode = 1 only.
"""
import numpy as np

import cov_ref
import lin_ref

LD = lin_ref.LD
EPS = lin_ref.EPS
EDGE_KEYS = ("obs_pose", "obs_lm", "obs_cam", "obs_uv")


def landmark_set(w, m):
    """in_M [L]: the landmarks with an edge to pose m."""
    L = len(w["lm_xyz"])
    op, ol = np.asarray(w["obs_pose"], np.int64), np.asarray(w["obs_lm"], np.int64)
    in_M = np.zeros(L, bool)
    in_M[ol[op == m]] = True
    return in_M


def restrict(w, keep):
    """Window w with the edges keep [O] alone."""
    return dict(w, **{k: np.asarray(w[k])[keep] for k in EDGE_KEYS if w.get(k) is not None})


def edge_mask(w, m, edges):
    """The edges the system is formed from.  "M": those of the landmarks m observes (the definition); "all": every
    edge, "to_m": the edges to m alone (the two wrong choices the tests hold the GPU away from)."""
    op, ol = np.asarray(w["obs_pose"], np.int64), np.asarray(w["obs_lm"], np.int64)
    if edges == "M":
        return landmark_set(w, m)[ol]
    if edges == "all":
        return np.ones(len(op), bool)
    if edges == "to_m":
        return op == m
    raise ValueError(edges)


def _linearise_guarded(w, deg, **kw):
    """lin_ref.linearise(w) with H_ll^-1 = 0 for the landmarks deg [L] (the module's docstring)."""
    orig = lin_ref._inv3

    def inv3(H):
        Hs = H.copy()
        Hs[deg] = np.eye(3, dtype=H.dtype)
        X = orig(Hs)
        X[deg] = 0
        return X

    lin_ref._inv3 = inv3
    try:
        return lin_ref.linearise(w, **kw)
    finally:
        lin_ref._inv3 = orig


def system(w, m, pose=None, lm=None, huber_delta=5.991, prior=None, dtype=LD, edges="M"):
    """(A [6P, 6P], b [6P], info): the system before the elimination.  prior: (H [6P, 6P], b [6P]) or None."""
    P, L = int(w["n_poses"]), len(w["lm_xyz"])
    keep = edge_mask(w, m, edges)
    wm = restrict(w, keep)
    n_obs = np.bincount(np.asarray(wm["obs_lm"], np.int64), minlength=L)
    deg = n_obs == 1
    R = _linearise_guarded(wm, deg, pose=pose, lm=lm, huber_delta=huber_delta, dtype=dtype)
    fixed = np.asarray(R["fixed"], bool)
    A, b = R["S"].astype(dtype).copy(), R["bs"].astype(dtype).copy()
    if prior is not None:
        live = np.repeat(~fixed, 6)
        A += np.where(live[:, None] & live[None, :], np.asarray(prior[0], dtype), 0)
        b += np.where(live, np.asarray(prior[1], dtype), 0)
    info = dict(in_M=n_obs > 0, n_landmarks=int((n_obs > 0).sum()), n_edges=int(keep.sum()), n_degenerate=int(deg.sum()),
                fixed=fixed)
    return A, b, info


def marginalize(w, m, pose=None, lm=None, huber_delta=5.991, prior=None, dtype=LD, edges="M"):
    """The prior of window `w` with pose m marginalised, at the input state or at pose [P, 12] / lm [L, 3].  Returns a
    dict: H [6P, 6P], b [6P], A and b_A (the system before the elimination), in_M [L], n_landmarks, n_edges,
    n_degenerate, fixed [P], rows (the rows whose diagonal of H is not zero), kappa (the scaled condition number of the
    eliminated block A[m, m]; 1 for a fixed m)."""
    P = int(w["n_poses"])
    A, b, info = system(w, m, pose=pose, lm=lm, huber_delta=huber_delta, prior=prior, dtype=dtype, edges=edges)
    mm = np.arange(6 * m, 6 * m + 6)
    r = np.setdiff1d(np.arange(6 * P), mm)
    H, g = np.zeros((6 * P, 6 * P), dtype), np.zeros(6 * P, dtype)
    if info["fixed"][m]:
        H[np.ix_(r, r)], g[r] = A[np.ix_(r, r)], b[r]
        kappa = 1.0
    else:
        Amm = A[np.ix_(mm, mm)]
        Ai = cov_ref.invert(Amm, dtype)
        Arm = A[np.ix_(r, mm)]
        H[np.ix_(r, r)] = A[np.ix_(r, r)] - Arm @ Ai @ Arm.T
        g[r] = b[r] - Arm @ (Ai @ b[mm])
        kappa = cov_ref.scaled_kappa(Amm)[0]
    rows = np.flatnonzero(np.diag(H).astype(np.float64) != 0.0)
    return dict(info, H=H, b=g, A=A, b_A=b, rows=rows, kappa=kappa)


def pose_error(A, B, rows):
    """e(A, B) = max_ij |A_ij - B_ij| / sqrt(B_ii B_jj) over `rows` (those with a non-zero reference diagonal), and the
    worst entry's pose pair: cov_ref.pose_error."""
    return cov_ref.pose_error(A, B, rows)


def rhs_scale(ref):
    """The scale of b_prior's error: max_i |b_i| / sqrt(H_ii) of the reference over its rows (lin_ref.rhs_error's)."""
    rows = ref["rows"]
    d = np.sqrt(np.diag(ref["H"]).astype(np.float64)[rows])
    return float((np.abs(ref["b"].astype(np.float64)[rows]) / d).max())


def rhs_error(b, ref):
    """max_i |b_i - ref_i| / sqrt(H_ii) over the reference's rows, over rhs_scale(ref); and the worst row's pose."""
    rows = ref["rows"]
    d = np.sqrt(np.diag(ref["H"]).astype(np.float64)[rows])
    num = np.abs((np.asarray(b, LD) - ref["b"]).astype(np.float64)[rows]) / d
    if not np.isfinite(num).all():
        return float("inf"), int(rows[np.argmax(~np.isfinite(num))]) // 6
    i = int(np.argmax(num))
    return float(num[i] / rhs_scale(ref)), int(rows[i]) // 6


def tolerance(e_double, kappa):
    """cov_ref.tolerance: max(8 x the double evaluation's own distance, 64 eps kappa), kappa the eliminated block's."""
    return cov_ref.tolerance(e_double, kappa)


def random_prior(P, A, b, seed):
    """A random SPD prior_H of the size of A's diagonal and a random prior_b of the size of b (the earlier prior of the tests)."""
    rng = np.random.default_rng(seed)
    n = 6 * P
    G = rng.standard_normal((n, n))
    dA = np.diag(np.asarray(A, np.float64))
    s = np.sqrt(np.where(dA > 0, dA, np.median(dA[dA > 0])))
    H = (G @ G.T / n + np.eye(n)) * s[:, None] * s[None, :] * 0.5
    H = np.tril(H) + np.tril(H, -1).T
    g = rng.standard_normal(n) * np.abs(np.asarray(b, np.float64)).max()
    return H, g
