"""step_ref -- the pose step of one LM trial in np.longdouble, and the yardsticks it is judged by (TEST INFRASTRUCTURE).

Every controller claims that its pose step solves (S + lambda D) dx = b_s.  This module states that claim in plain
NumPy: the damped system as the controllers insert it (`assemble`), the ladder's lambdas (`rung_lambdas`), the step
to long-double accuracy (`solve_ld`), and what two careful double-precision direct solvers make of the same system
(`yardstick`), which is the scale a controller's error is measured in.  Used by tests/test_step_ref_cpu.py and
tests/test_ctrl_step_gpu.py.
"""
import numpy as np

import oracle_bind as ob

LD = np.longdouble
if np.finfo(LD).eps > 2.0 ** -63:
    raise RuntimeError("step_ref needs an 80-bit (or wider) np.longdouble: eps = %g" % np.finfo(LD).eps)

EPS = 2.0 ** -52
# a controller's step may be this many times further from the truth than the worse of the two direct solves: the
# smallest power of two that is at least twice the worst ratio measured on the device (7.88; the table is in
# tests/test_ctrl_step_gpu.py's docstring and DESIGN.md 4.6)
MARGIN = 16.0


def bound(yard):
    """The criterion of a step's forward or backward error: MARGIN x the yardstick's, floor 64 eps (the floor of
    tests/test_lin_system_gpu.py)."""
    return max(MARGIN * yard, 64 * EPS)


def assemble(S, lam, strategy):
    """S + lambda I (strategy 0, problem.cpp's DEFAULT) or S + lambda diag(S) (strategy 1), as every controller inserts
    it (band_value, lh_ctrl_b.hip: v + lambda, v + lambda v on the rows of real poses) and as the oracle does
    (oracle/lego_oracle.c: S[i][i] += lambda, S[i][i] += lambda S[i][i]): the same two double operations, so the
    diagonal is bit-identical to the one the controller factors."""
    A = np.array(S, np.float64, copy=True)
    d = np.diagonal(A).copy()
    lam = float(lam)
    np.fill_diagonal(A, d + lam if strategy == 0 else d + lam * d)
    return A


def rung_lambdas(lam, ni, strategy, m):
    """The lambdas of ladder rungs 0..m-1 (ladder_read, lh_lm.h): rung r applies r rejection updates to (lambda, ni) in
    ctrl_lm_step's order -- lambda *= ni, ni *= 2 (problem.cpp:550-551), or min(11 lambda, 1e7) (:576).  Python
    floats are IEEE doubles and each update is one rounded product, so the sequence is exact."""
    lam, ni = float(lam), float(ni)
    out = []
    for _ in range(m):
        out.append(lam)
        if strategy == 0:
            lam *= ni
            ni *= 2.0
        else:
            lam = min(lam * 11.0, 1e7)
    return out


def reject_update(lam, ni, strategy):
    """(lambda, ni) after one rejection."""
    return (lam * ni, ni * 2.0) if strategy == 0 else (min(lam * 11.0, 1e7), ni)


def free_rows(A, b):
    """The rows that carry an unknown: a fixed pose's rows and columns of S and its b_s are exact zeros (k_lin adds
    nothing for it), so its rows of A hold at most lambda on the diagonal and its step is exactly 0."""
    A = np.asarray(A)
    off = A - np.diag(np.diagonal(A))
    return off.any(axis=1) | (np.asarray(b) != 0)


def lower_symmetric(S):
    """The symmetric matrix of S's lower triangle: what every LDL^T here reads (the oracle's S is not symmetric to
    the last bit and further where a landmark's H_ll is ill-conditioned: its LU inverse of H_ll is not)."""
    S = np.asarray(S, np.float64)
    return np.tril(S) + np.tril(S, -1).T


def cholesky(A):
    """A = C C^T, or a ValueError that names the trouble: the damped systems of these tests are positive definite."""
    try:
        return np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        raise ValueError("the system is not positive definite (smallest eigenvalue %.3e): not a case these tests can "
                         "judge" % np.linalg.eigvalsh(A)[0]) from None


def cho_solve(C, b):
    """x = (C C^T)^-1 b by forward and back substitution, row by row (no inverse is formed: a product with C^-1 is
    not backward stable)."""
    n = len(b)
    y = np.zeros(n)
    for i in range(n):
        y[i] = (b[i] - C[i, :i] @ y[:i]) / C[i, i]
    U = np.ascontiguousarray(C.T)
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - U[i, i + 1:] @ x[i + 1:]) / U[i, i]
    return x


def _two_product(a, b):
    """a b = p + e exactly, elementwise in double (Dekker's product with Veltkamp's split: no fused multiply-add)."""
    p = a * b
    c = 134217729.0 * a
    ah = c - (c - a)
    al = a - ah
    c = 134217729.0 * b
    bh = c - (c - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def residual(A, b, x):
    """b - A x for a double A, b and a long-double x, every entry rounded once: x = xh + xl in two doubles (exact: an
    80-bit x has 64 significant bits), each product A_ij xh_j and A_ij xl_j as an exact sum of two doubles, and a row's
    terms added by math.fsum.  A residual accumulated in long double carries eps_ld |A| |x|, which leaves the refined
    x at kappa(A) 2^-64: only 2^-11 below a double solve's kappa(A) 2^-53, no margin against a yardstick that is a
    little lucky.  This one leaves x at the rounding of its own long-double entries."""
    import math
    x = np.asarray(x, LD)
    xh = x.astype(np.float64)
    xl = (x - xh.astype(LD)).astype(np.float64)
    ph, eh = _two_product(A, xh[None, :])
    pl, el = _two_product(A, xl[None, :])
    T = np.stack([ph, eh, pl, el], 1)          # [row][4][column]
    nz = A != 0
    r = np.zeros(len(b))
    for i in range(len(b)):
        r[i] = math.fsum([b[i]] + (-T[i][:, nz[i]]).ravel().tolist())
    return r


def solve_ld(A, b, free=None, max_rounds=30):
    """x = A^-1 b in long double by iterative refinement: x is kept in long double, each residual b - A x is evaluated
    to the last bit (`residual`), the correction comes from a double Cholesky factor of A, until the correction stops
    shrinking.  Returns (x, the last relative correction applied: ||d|| / ||x||).  The refinement contracts by about
    kappa(A) eps per round, so what is left of the error is far below that last correction.  Rows outside `free`
    (default free_rows) are removed first; their x is exactly 0."""
    A = np.asarray(A, np.float64)
    b = np.asarray(b, np.float64)
    if free is None:
        free = free_rows(A, b)
    idx = np.flatnonzero(free)
    x = np.zeros(len(b), LD)
    if len(idx) == 0:
        return x, 0.0
    Af, bf = np.ascontiguousarray(A[np.ix_(idx, idx)]), b[idx]
    C = cholesky(Af)
    xf = cho_solve(C, bf).astype(LD)
    last, prev = np.inf, np.inf
    for _ in range(max_rounds):
        d = cho_solve(C, residual(Af, bf, xf))
        nx = float(np.sqrt((xf * xf).sum()))
        rel = float(np.linalg.norm(d)) / nx if nx > 0 else 0.0
        if not rel < prev:
            break
        xf = xf + d.astype(LD)
        last, prev = rel, rel
        if rel == 0.0:
            break
    x[idx] = xf
    return x, last


def _norm(v):
    v = np.asarray(v, LD)
    return float(np.sqrt((v * v).sum()))


def forward_error(x, x_ref, free):
    """e = ||x - x_ref||_2 / ||x_ref||_2 over the free rows."""
    x, x_ref = np.asarray(x, LD), np.asarray(x_ref, LD)
    return _norm((x - x_ref)[free]) / _norm(x_ref[free])


def backward_error(A, b, x, free):
    """eta = ||b - A x||_2 / (||A||_F ||x||_2 + ||b||_2) over the free rows, the residual in long double."""
    idx = np.flatnonzero(free)
    Af = np.asarray(A, np.float64)[np.ix_(idx, idx)]
    bf, xf = np.asarray(b, LD)[idx], np.asarray(x, LD)[idx]
    r = bf - Af.astype(LD) @ xf
    return _norm(r) / (float(np.linalg.norm(Af)) * _norm(xf) + _norm(bf))


def worst_pose(x, x_ref):
    """(pose, ||x - x_ref||_inf over its six rows) of the pose that is furthest off."""
    d = np.abs((np.asarray(x, LD) - np.asarray(x_ref, LD)).astype(np.float64)).reshape(-1, 6).max(1)
    p = int(np.argmax(d))
    return p, float(d[p])


def direct_solves(A, b, free):
    """Two double-precision direct solves of the free rows' system: the reference's own LDL^T as the oracle restates it
    (Eigen LDLT with diagonal pivoting, ob.ldlt_solve) and an unpivoted Cholesky solve (np.linalg.cholesky, two
    triangular solves).  np.linalg.solve (LU with row pivoting) is left out: it ignores the symmetry, is about 30 x
    further from the truth than the oracle's LDL^T on these systems and would only loosen the test."""
    idx = np.flatnonzero(free)
    Af = np.ascontiguousarray(np.asarray(A, np.float64)[np.ix_(idx, idx)])
    bf = np.ascontiguousarray(np.asarray(b, np.float64)[idx])
    out = []
    xs = np.zeros(len(b))
    xs[idx] = ob.ldlt_solve(Af, bf)
    out.append(xs)
    xs = np.zeros(len(b))
    xs[idx] = cho_solve(cholesky(Af), bf)
    out.append(xs)
    return out


def yardstick(A, b, x_ref, free=None):
    """(e_yard, eta_yard): the larger forward and the larger backward error of direct_solves' two solutions."""
    if free is None:
        free = free_rows(A, b)
    xs = direct_solves(A, b, free)
    return (max(forward_error(x, x_ref, free) for x in xs), max(backward_error(A, b, x, free) for x in xs))


def spose_ref(dx, lam, strategy, bp, hd):
    """The pose half of the gain denominator (ctrl_step_tail, isGoodStepInLM's scale): sum_i dx_i (lambda D_ii dx_i +
    b_p,i) in long double, D = I (strategy 0) or diag H_pp (strategy 1), with the a-priori bound of a double
    evaluation in any order: (n + 16) eps sum |terms| (both products of a term counted, as lin_ref does)."""
    d, bpl = np.asarray(dx, LD), np.asarray(bp, LD)
    D = LD(1) if strategy == 0 else np.asarray(hd, LD)
    t1, t2 = LD(lam) * D * d * d, d * bpl
    n = len(d)
    return float((t1 + t2).sum()), float((n + 16) * EPS * (np.abs(t1) + np.abs(t2)).sum())
