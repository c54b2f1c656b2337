"""cov_ref -- the marginal covariances of one window at a given state, in np.longdouble (TEST INFRASTRUCTURE).

What lh_covariance (include/lego_ba.h) computes, from tests/lin_ref.py's linearisation: with
S = H_pp - H_pl H_ll^-1 H_lp (no lambda), the held poses (the window's fixed ones and `anchor`) and f the rows of
the others,

    Sigma_pp[f, f] = (S[f, f])^-1, zero elsewhere
    Sigma_l = H_ll^-1 + H_ll^-1 (sum_{e, e' in l} H_lp,e Sigma_pp[p(e), p(e')] H_pl,e') H_ll^-1

The reference (dtype np.longdouble) inverts S[f, f] from np.linalg.inv in double by three Newton-Schulz steps
X <- X (2 I - S X) in long double and asserts max |S X - I| < 1e-13.  The double evaluation (dtype np.float64) is
the same statements in double with np.linalg.inv alone: what a careful double implementation gets, and so the unit of
the GPU's tolerance.  lin_ref models gate_mode = 1 only (tests/lin_cases.py's cases pass it).
"""
import numpy as np

import lin_ref

LD = lin_ref.LD
EPS = lin_ref.EPS


def held_poses(w, anchor=-1):
    P = int(w["n_poses"])
    held = np.zeros(P, bool) if w.get("pose_fixed") is None else np.asarray(w["pose_fixed"]).astype(bool).copy()
    if anchor >= 0:
        held[anchor] = True
    return held


def invert(S, dtype=LD):
    """S^-1 of a symmetric positive definite S [n, n] in `dtype` (the module's docstring)."""
    X = np.linalg.inv(np.asarray(S, np.float64))
    if dtype is np.float64:
        return X
    S, X = np.asarray(S, LD), X.astype(LD)
    I2 = 2 * np.eye(len(S), dtype=LD)
    for _ in range(3):
        X = X @ (I2 - S @ X)
    res = float(np.abs(S @ X - np.eye(len(S), dtype=LD)).max())
    assert res < 1e-13, f"cov_ref: max |S X - I| = {res:.2e}"
    return X


def scaled_kappa(S):
    """kappa_2 of the unit-diagonal scaling of S, and its extreme eigenvalues."""
    S = np.asarray(S, np.float64)
    d = 1.0 / np.sqrt(np.diag(S))
    ev = np.linalg.eigvalsh(S * d[:, None] * d[None, :])
    return float(ev[-1] / ev[0]), float(ev[0]), float(ev[-1])


def covariance(w, pose=None, lm=None, huber_delta=5.991, anchor=-1, dtype=LD):
    """The covariances of window `w` at its input state or at pose [P, 12] / lm [L, 3].  Returns a dict: pose_full
    [6P, 6P], pose_blocks [P, 6, 6], lm [L, 3, 3] (NaN for a landmark no edge observes), held [P], free (the free rows),
    S_ff, kappa (the scaled S[f, f]'s), and R, the linearisation."""
    R = lin_ref.linearise(w, pose=pose, lm=lm, huber_delta=huber_delta, dtype=dtype)
    P = int(w["n_poses"])
    held = held_poses(w, anchor)
    free = np.flatnonzero(np.repeat(~held, 6))
    S_ff = R["S"][np.ix_(free, free)]
    full = np.zeros((6 * P, 6 * P), dtype)
    full[np.ix_(free, free)] = invert(S_ff, dtype)
    blocks = np.stack([full[6 * p:6 * p + 6, 6 * p:6 * p + 6] for p in range(P)])
    op, ol, Hpl, Hinv = R["op"], R["ol"], R["Hpl"], R["Hinv"]
    L = Hinv.shape[0]
    F4 = full.reshape(P, 6, P, 6)
    out = np.full((L, 3, 3), np.nan, dtype)
    order = np.argsort(ol, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(ol, minlength=L))])
    for l in range(L):
        idx = order[ptr[l]:ptr[l + 1]]
        idx = idx[R["keep"][idx]]
        if len(idx) == 0:
            continue
        G = Hpl[idx]                                  # [k, 6, 3] H_pl,e (zero for an edge to a fixed pose)
        Sg = F4[op[idx]][:, :, op[idx], :]            # [k, 6, k, 6]
        M = np.einsum("eac,eafb,fbd->cd", G, Sg, G)
        out[l] = Hinv[l] + Hinv[l] @ M @ Hinv[l]
    return dict(pose_full=full, pose_blocks=blocks, lm=out, held=held, free=free, S_ff=S_ff,
                kappa=scaled_kappa(S_ff)[0], R=R)


def pose_error(A, B, free):
    """e(A, B) = max_ij |A_ij - B_ij| / sqrt(B_ii B_jj) over the free rows, and the worst entry's pose pair."""
    A = np.asarray(A, LD)[np.ix_(free, free)]
    Bf = np.asarray(B, LD)[np.ix_(free, free)]
    d = np.sqrt(np.diag(Bf).astype(np.float64))
    E = np.abs((A - Bf).astype(np.float64)) / d[:, None] / d[None, :]
    if not np.isfinite(E).all():
        i, j = np.argwhere(~np.isfinite(E))[0]
        return float("inf"), (int(free[i]) // 6, int(free[j]) // 6)
    i, j = np.unravel_index(np.argmax(E), E.shape)
    return float(E[i, j]), (int(free[i]) // 6, int(free[j]) // 6)


def lm_error(A, B):
    """The same per landmark on the 3x3, over the landmarks whose reference is finite: (e, the worst landmark).  Where
    the reference is NaN (no edge) A must be NaN too: else the error is inf at that landmark."""
    A, B = np.asarray(A, LD), np.asarray(B, LD)
    ok = np.isfinite(B.astype(np.float64)).all((1, 2))
    wrong = np.flatnonzero(~ok & ~np.isnan(A.astype(np.float64)).all((1, 2)))
    if len(wrong):
        return float("inf"), int(wrong[0])
    if not ok.any():
        return 0.0, -1
    d = np.sqrt(np.einsum("lii->li", B[ok]).astype(np.float64))
    E = np.abs((A[ok] - B[ok]).astype(np.float64)) / d[:, :, None] / d[:, None, :]
    E = np.where(np.isfinite(E), E, np.inf).max((1, 2))
    k = int(np.argmax(E))
    return float(E[k]), int(np.flatnonzero(ok)[k])


def tolerance(e_double, kappa, margin=8.0):
    """The GPU's bound on a case: margin x the double evaluation's own distance from the reference, floor 64 eps kappa
    (the forward error of an inverse grows with the scaled condition number)."""
    return max(margin * e_double, 64 * EPS * kappa)
