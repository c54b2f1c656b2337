"""lin_ref -- the linearisation of one window and its reduced pose system, in np.longdouble (TEST INFRASTRUCTURE).

A plain, vectorised restatement of what k_lin + k_reduce (and oracle/lego_oracle.c's build_sparse /
solve_sparse) compute, evaluated in 80-bit arithmetic from the window's double inputs: the yardstick of
tests/test_lin_ref_cpu.py and tests/test_lin_system_gpu.py.  Every step follows the reference's order of
operations (the Sophus quaternion round trip of each pose and extrinsic, the `+1e-18` denominators), so that
what is left between this and a double evaluation is rounding alone.

Outlier edges take the Huber gate's residue as zero (gate_mode=1 of the oracle and the solver): W = rho1 I.
Gate mode 0 tests the sign of a rounding residue of double arithmetic, which no higher precision reproduces.
"""
import numpy as np

LD = np.longdouble
if np.finfo(LD).eps > 2.0 ** -63:
    raise RuntimeError("lin_ref needs an 80-bit (or wider) np.longdouble: eps = %g" % np.finfo(LD).eps)

EPS = 2.0 ** -52   # the double arithmetic under test
MUTATIONS = ("drop_edge", "outlier_weight_one", "swap_poses", "wrong_camera")


def q_from_R(R):
    """Eigen's quaternion (w, x, y, z) of rotation matrices R [n, 3, 3]."""
    R = np.asarray(R, LD)
    q = np.zeros((R.shape[0], 4), LD)
    for n, M in enumerate(R):
        t = M[0, 0] + M[1, 1] + M[2, 2]
        if t > 0:
            t = np.sqrt(t + LD(1))
            h = LD(0.5) / t
            q[n] = (LD(0.5) * t, (M[2, 1] - M[1, 2]) * h, (M[0, 2] - M[2, 0]) * h, (M[1, 0] - M[0, 1]) * h)
        else:
            i = 1 if M[1, 1] > M[0, 0] else 0
            i = 2 if M[2, 2] > M[i, i] else i
            j, k = (i + 1) % 3, (i + 2) % 3
            t = np.sqrt(M[i, i] - M[j, j] - M[k, k] + LD(1))
            h = LD(0.5) / t
            q[n, 0] = (M[k, j] - M[j, k]) * h
            q[n, 1 + i], q[n, 1 + j], q[n, 1 + k] = LD(0.5) * t, (M[j, i] + M[i, j]) * h, (M[k, i] + M[i, k]) * h
    return q


def R_from_q(q):
    """Eigen's toRotationMatrix of quaternions q [..., 4] (not normalised first, as Eigen)."""
    w, x, y, z = (q[..., i] for i in range(4))
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    R = np.empty(q.shape[:-1] + (3, 3), LD)
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - (ty * y + tz * z), ty * x - tz * w, tz * x + ty * w
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = ty * x + tz * w, 1 - (tx * x + tz * z), tz * y - tx * w
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = tz * x - ty * w, tz * y + tx * w, 1 - (tx * x + ty * y)
    return R


def q_mul(a, b):
    """Eigen's quaternion product with Sophus' first-order renormalisation (SO3 *= SO3)."""
    w = a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2] - a[..., 3] * b[..., 3]
    x = a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0] + a[..., 2] * b[..., 3] - a[..., 3] * b[..., 2]
    y = a[..., 0] * b[..., 2] + a[..., 2] * b[..., 0] + a[..., 3] * b[..., 1] - a[..., 1] * b[..., 3]
    z = a[..., 0] * b[..., 3] + a[..., 3] * b[..., 0] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
    o = np.stack([w, x, y, z], -1)
    return o * (2 / (1 + (o * o).sum(-1)))[..., None]


def se3_exp(a):
    """Sophus SE3::exp of twists a [n, 6] (translation part first): (q [n, 4], t [n, 3])."""
    a = np.asarray(a, LD)
    w = a[:, 3:]
    th2 = (w * w).sum(1)
    th = np.sqrt(th2)
    small = th < 1e-10
    ths = np.where(small, LD(1), th)
    imag = np.where(small, LD(0.5) - th2 / 48 + th2 * th2 / 3840, np.sin(ths / 2) / ths)
    real = np.where(small, 1 - th2 / 8 + th2 * th2 / 384, np.cos(ths / 2))
    q = np.concatenate([real[:, None], imag[:, None] * w], 1)
    Om = np.zeros((len(a), 3, 3), LD)
    Om[:, 0, 1], Om[:, 0, 2], Om[:, 1, 0] = -w[:, 2], w[:, 1], w[:, 2]
    Om[:, 1, 2], Om[:, 2, 0], Om[:, 2, 1] = -w[:, 0], -w[:, 1], w[:, 0]
    c1 = (1 - np.cos(ths)) / (ths * ths)
    c2 = (ths - np.sin(ths)) / (ths * ths * ths)
    V = np.eye(3, dtype=LD) + c1[:, None, None] * Om + c2[:, None, None] * np.einsum("nij,njk->nik", Om, Om)
    V = np.where(small[:, None, None], R_from_q(q), V)
    return q, np.einsum("nij,nj->ni", V, a[:, :3])


def left_update(dx, pose12):
    """exp(dx) * T for poses [P, 12] (row-major [R | t]) and steps dx [P, 6]: the new [P, 12], VertexPose::add."""
    T = np.asarray(pose12, LD).reshape(-1, 3, 4)
    qe, te = se3_exp(np.asarray(dx, LD).reshape(-1, 6))
    q = q_mul(qe, q_from_R(T[:, :, :3]))
    t = te + np.einsum("nij,nj->ni", R_from_q(qe), T[:, :, 3])
    return np.concatenate([R_from_q(q), t[:, :, None]], 2).reshape(-1, 12)


def _inv3(H):
    """Exact adjugate inverse of 3x3 matrices [n, 3, 3]."""
    a, b, c, d, e, f, g, h, i = (H[:, r, s] for r in range(3) for s in range(3))
    A = np.empty_like(H)
    A[:, 0, 0], A[:, 0, 1], A[:, 0, 2] = e * i - f * h, c * h - b * i, b * f - c * e
    A[:, 1, 0], A[:, 1, 1], A[:, 1, 2] = f * g - d * i, a * i - c * g, c * d - a * f
    A[:, 2, 0], A[:, 2, 1], A[:, 2, 2] = d * h - e * g, b * g - a * h, a * e - b * d
    det = a * A[:, 0, 0] + b * A[:, 1, 0] + c * A[:, 2, 0]
    return A / det[:, None, None]


def _mutate(mutation, op, ol, oc, ncam, outlier):
    """One seeded corruption of a single edge's handling: (keep mask, obs_pose, obs_cam, edge forced to weight 1)."""
    kind, seed = mutation
    rng = np.random.default_rng(seed)
    O = len(op)
    keep, op, oc, force = np.ones(O, bool), op.copy(), oc.copy(), -1
    if kind == "drop_edge":   # (of a landmark that keeps two edges at least: its H_ll stays regular)
        keep[rng.choice(np.flatnonzero(np.bincount(ol)[ol] >= 3))] = False
    elif kind == "outlier_weight_one":
        cand = np.flatnonzero(outlier)
        if len(cand) == 0:
            raise ValueError("outlier_weight_one: the window has no outlier edge")
        force = int(rng.choice(cand))
    elif kind == "swap_poses":   # two edges of one landmark from different poses exchange their poses
        while True:
            e = rng.integers(O)
            other = np.flatnonzero((ol == ol[e]) & (op != op[e]))
            if len(other):
                f = int(rng.choice(other))
                op[e], op[f] = op[f], op[e]
                break
    elif kind == "wrong_camera":
        if ncam < 2:
            raise ValueError("wrong_camera: the window has one camera")
        e = rng.integers(O)
        oc[e] = (oc[e] + 1 + rng.integers(ncam - 1)) % ncam
    else:
        raise ValueError(kind)
    return keep, op, oc, force


def linearise(w, pose=None, lm=None, huber_delta=5.991, mutation=None, dtype=LD):
    """The linearisation of window `w` (lego_ba.generate_window's layout) at its input state, or at `pose`
    [P, 12] / `lm` [L, 3], and its reduced pose system.  mutation: (one of MUTATIONS, seed) corrupts the handling
    of one edge (the self-test that the comparison has teeth).  dtype: np.float64 evaluates the same statements in
    double (a plain double implementation, to check the a-priori bounds against).

    Returns a dict: S [6P, 6P], bs, bp, hd (diag H_pp), chi2 (sum rho0), maxd (max |diag H_ll|), ndeg, per landmark
    Hll, Hinv, bl, kappa (kappa_2(H_ll)) and hinv_norm; per edge Hpl [O, 6, 3] and the index arrays it used (op, ol);
    the a-priori summation bounds bp_bound, hd_bound [6P] and chi2_bound ((n + 16) eps sum |terms|; bp_bound_narrow:
    with the formed residual as one operand, which double arithmetic does not keep); fixed [P]."""
    F = dtype
    pose = np.asarray(w["pose_Tcw"] if pose is None else pose, np.float64).reshape(-1, 3, 4).astype(F)
    X_all = np.asarray(w["lm_xyz"] if lm is None else lm, np.float64).astype(F)
    P, L = pose.shape[0], X_all.shape[0]
    op, ol = np.asarray(w["obs_pose"], np.int64), np.asarray(w["obs_lm"], np.int64)
    O = len(op)
    oc = np.zeros(O, np.int64) if w.get("obs_cam") is None else np.asarray(w["obs_cam"], np.int64)
    uv = np.asarray(w["obs_uv"], np.float64).astype(F)
    ext = w.get("cam_ext")
    ext = (np.tile(np.eye(3, 4), (1, 1, 1)) if ext is None else np.asarray(ext, np.float64).reshape(-1, 3, 4)).astype(F)
    fixed = np.zeros(P, bool) if w.get("pose_fixed") is None else np.asarray(w["pose_fixed"]).astype(bool)
    fx, fy, cx, cy = (F(v) for v in np.asarray(w["K"], np.float64))
    tiny = F(1e-18)

    # the Sophus round trip: SE3(estimate_) keeps a quaternion, rotationMatrix() rebuilds the matrix from it
    qT, tT = q_from_R(pose[:, :, :3]).astype(F), pose[:, :, 3]
    qe, te = q_from_R(ext[:, :, :3]).astype(F), ext[:, :, 3]
    RT, Re = R_from_q(qT).astype(F), R_from_q(qe).astype(F)
    # ext * T per (camera, pose): the Jacobian's point goes through the product, the residual's through both in turn
    q_et = q_mul(qe[:, None, :], qT[None, :, :]).astype(F)
    R_et = R_from_q(q_et).astype(F)
    t_et = te[:, None, :] + np.einsum("cij,pj->cpi", Re, tT)

    def edges(op, oc, force=-1):
        X = X_all[ol]
        Pb = np.einsum("oij,oj->oi", RT[op], X) + tT[op]
        Pc = np.einsum("oij,oj->oi", Re[oc], Pb) + te[oc]
        den = Pc[:, 2] + tiny
        proj = np.stack([(fx * Pc[:, 0] + cx * Pc[:, 2]) / den, (fy * Pc[:, 1] + cy * Pc[:, 2]) / den], 1)
        r = uv - proj
        Pj = np.einsum("oij,oj->oi", R_et[oc, op], X) + t_et[oc, op]
        x, y, zi = Pj[:, 0], Pj[:, 1], 1 / (Pj[:, 2] + tiny)
        zi2 = zi * zi
        Jp = np.zeros((len(op), 2, 6), F)
        Jp[:, 0, 0], Jp[:, 0, 2], Jp[:, 0, 3] = -fx * zi, fx * x * zi2, fx * x * y * zi2
        Jp[:, 0, 4], Jp[:, 0, 5] = -fx - fx * x * x * zi2, fx * y * zi
        Jp[:, 1, 1], Jp[:, 1, 2], Jp[:, 1, 3] = -fy * zi, fy * y * zi2, fy + fy * y * y * zi2
        Jp[:, 1, 4], Jp[:, 1, 5] = -fy * x * y * zi2, -fy * x * zi
        Jl = np.einsum("oik,okj->oij", np.einsum("oik,okj->oij", Jp[:, :, :3], Re[oc]), RT[op])
        e2 = (r * r).sum(1)
        if huber_delta > 0:
            d, d2 = F(huber_delta), F(huber_delta) * F(huber_delta)
            out = e2 > d2
            s = np.sqrt(np.where(out, e2, F(1)))
            rho0 = np.where(out, 2 * s * d - d2, e2)
            rho1 = np.where(out, d / s, F(1))
        else:
            out, rho0, rho1 = np.zeros(len(op), bool), e2, np.ones(len(op), F)
        if force >= 0:
            rho1 = rho1.copy()
            rho1[force] = 1
        return r, proj, Jp, Jl, rho0, rho1, out

    keep = np.ones(O, bool)
    force = -1
    if mutation is not None:
        outlier = edges(op, oc)[6]
        keep, op, oc, force = _mutate(mutation, op, ol, oc, ext.shape[0], outlier)
    r, proj, Jp, Jl, rho0, rho1, _ = edges(op, oc, force)
    live = (keep & ~fixed[op]).astype(F)   # a fixed pose's edge contributes to the landmark alone
    kf = keep.astype(F)
    wJp = Jp * (rho1 * live)[:, None, None]   # W = rho1 I (the gate's residue taken as zero)
    Hpp_e = np.einsum("oka,okb->oab", wJp, Jp)
    Hpl_e = np.einsum("oka,okb->oab", wJp, Jl)
    Hll_e = np.einsum("oka,okb->oab", Jl * (rho1 * kf)[:, None, None], Jl)
    bp_e = -np.einsum("oka,ok->oa", wJp, r)
    bl_e = -np.einsum("oka,ok->oa", Jl * (rho1 * kf)[:, None, None], r)

    Hpp = np.zeros((P, 6, 6), F)
    bp = np.zeros((P, 6), F)
    Hll = np.zeros((L, 3, 3), F)
    bl = np.zeros((L, 3), F)
    np.add.at(Hpp, op, Hpp_e)
    np.add.at(bp, op, bp_e)
    np.add.at(Hll, ol, Hll_e)
    np.add.at(bl, ol, bl_e)
    seen = np.bincount(ol[keep], minlength=L) > 0
    Hs = np.where(seen[:, None, None], Hll, np.eye(3, dtype=F))   # a landmark without an edge is no vertex
    Hinv = np.where(seen[:, None, None], _inv3(Hs), F(0))

    S4 = np.zeros((P, P, 6, 6), F)
    S4[np.arange(P), np.arange(P)] = Hpp
    bs = bp.copy()
    tH = np.einsum("oak,okc->oac", Hpl_e, Hinv[ol])
    np.add.at(bs, op, -np.einsum("oak,ok->oa", tH, bl[ol]))
    order = np.argsort(ol, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(ol, minlength=L))])
    for l in range(L):
        idx = order[ptr[l]:ptr[l + 1]]
        if len(idx):
            np.add.at(S4, (op[idx][:, None], op[idx][None, :]), -np.einsum("iak,jck->ijac", tH[idx], Hpl_e[idx]))
    S = S4.transpose(0, 2, 1, 3).reshape(6 * P, 6 * P)

    H64 = Hs.astype(np.float64)
    ev = np.linalg.eigvalsh(H64)
    kappa = np.where(seen, ev[:, 2] / ev[:, 0], 1.0)
    hinv_norm = np.where(seen, 1.0 / ev[:, 0], 0.0)

    # the a-priori bounds of a recursive sum of n products: (n + 16) eps sum |terms|.  The terms are the products as
    # the arithmetic forms them: r = uv - proj cancels (a residual of a pixel from operands of hundreds), so each
    # operand of that difference counts by itself
    n_p = np.bincount(op, weights=live.astype(np.float64), minlength=P)
    aJ = np.abs(wJp).astype(np.float64)
    ar = (np.abs(uv) + np.abs(proj)).astype(np.float64)
    bp_abs = np.zeros((P, 6))
    np.add.at(bp_abs, op, np.einsum("oka,ok->oa", aJ, ar))
    hd = np.einsum("paa->pa", Hpp).reshape(6 * P)
    nn = np.repeat(n_p, 6)
    # rho0's terms likewise: d rho0 = rho1 d(r . r), and r . r moves by 2 |r_k| per unit of either operand of r_k
    chi_abs = float(((rho0 + 2 * rho1 * (np.abs(r) * (np.abs(uv) + np.abs(proj))).sum(1)) * kf).sum())
    return dict(S=S, bs=bs.reshape(6 * P), bp=bp.reshape(6 * P), hd=hd, chi2=(rho0 * kf).sum(),
                maxd=np.abs(np.einsum("laa->la", Hll)).max(), ndeg=0, Hll=Hll, Hinv=Hinv, bl=bl, kappa=kappa,
                hinv_norm=hinv_norm, Hpl=Hpl_e, op=op, ol=ol, keep=keep, fixed=fixed,
                bp_bound=(nn + 16) * EPS * bp_abs.reshape(6 * P),
                bp_bound_narrow=(nn + 16) * EPS * _scatter_abs(op, np.abs(bp_e).astype(np.float64), P),
                hd_bound=(nn + 16) * EPS * np.abs(hd).astype(np.float64),
                chi2_bound=(O + 16) * EPS * chi_abs)


def _scatter_abs(op, a, P):
    out = np.zeros((P, 6))
    np.add.at(out, op, a)
    return out.reshape(6 * P)


def block_error(X, R, fixed):
    """e(X) = max over live pose pairs (p, q) of ||X_pq - R_pq||_F / sqrt(||R_pp||_F ||R_qq||_F), and the worst pair."""
    P = len(fixed)
    D = (np.asarray(X, LD) - R).reshape(P, 6, P, 6)
    nD = np.sqrt((D * D).sum((1, 3)).astype(np.float64))
    Rb = R.reshape(P, 6, P, 6)
    d = np.sqrt(np.array([float((Rb[p, :, p, :] ** 2).sum()) for p in range(P)]))
    d = np.sqrt(d)   # sqrt(||R_pp||_F)
    livep = ~np.asarray(fixed, bool)
    e = np.where(livep[:, None] & livep[None, :], nD / np.where(livep, d, 1.0)[:, None] / np.where(livep, d, 1.0)[None, :], 0.0)
    p, q = np.unravel_index(np.argmax(e), e.shape)
    return float(e[p, q]), (int(p), int(q))


def rhs_error(b, R):
    """b_s's metric: max_i |b_i - bs_i| / sqrt(S_ii) over max_i |bs_i| / sqrt(S_ii), live rows; and the worst row."""
    d = np.sqrt(np.diag(R["S"]).astype(np.float64))
    livep = np.repeat(~R["fixed"], 6)
    s = np.where(livep, 1.0 / np.where(livep, d, 1.0), 0.0)
    num = np.abs((np.asarray(b, LD) - R["bs"]).astype(np.float64)) * s
    den = (np.abs(R["bs"].astype(np.float64)) * s).max()
    i = int(np.argmax(num))
    return float(num[i] / den), i
