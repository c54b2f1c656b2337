"""Synthetic frames for the frontend pose-only path (Frontend::EstimateCurrentPose,
src/frontend_lego.cpp:157-250).  Test data only.

A frame: the true pose T_cw (camera moving along +z with small yaw, as the
backend windows), map points in front of the camera (depth 8-60 m, the
windows' ranges), their projections with N(0, 1 px) noise rounded to float32
(cv::KeyPoint, toVec2), a fraction of gross outliers uniform in the image, and
the frame's initial pose: the truth perturbed (the constant-velocity guess the
frontend starts from).  Counter-based: frame f of seed s is the same whatever
batch it is generated in.
"""
import numpy as np

K = np.array([517.3, 516.5, 325.1, 249.7])   # config/kitti_00.yaml:10-13


def _rot(axis_angle):
    th = np.linalg.norm(axis_angle)
    if th < 1e-15:
        return np.eye(3)
    k = axis_angle / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def frame(seed, f, n_obs=150, outlier_frac=0.05, rot_sigma=0.01, trans_sigma=0.05):
    rng = np.random.default_rng([seed, f])
    R_true = _rot(np.array([0.0, rng.normal(0, 0.02), 0.0]))
    c = np.array([rng.normal(0, 0.5), 0.0, float(f)])          # camera centre (world)
    t_true = -R_true @ c
    # points in the camera frame, then to the world
    z = rng.uniform(8.0, 60.0, n_obs)
    u = rng.uniform(0, 640, n_obs)
    v = rng.uniform(0, 480, n_obs)
    Xc = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
    Xw = (Xc - t_true) @ R_true                                  # R^T (Xc - t)
    proj = np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], axis=1)
    uv = proj + rng.normal(0, 1.0, proj.shape)
    out = rng.random(n_obs) < outlier_frac
    ang = rng.uniform(0, 2 * np.pi, out.sum())
    mag = rng.uniform(10.0, 40.0, out.sum())
    uv[out] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)
    uv = uv.astype(np.float32).astype(np.float64)
    dR = _rot(rng.normal(0, rot_sigma, 3))
    R0 = dR @ R_true
    t0 = t_true + rng.normal(0, trans_sigma, 3)
    pose_true = np.hstack([R_true, t_true[:, None]]).reshape(12)
    pose0 = np.hstack([R0, t0[:, None]]).reshape(12)
    return dict(pose_true=pose_true, pose_Tcw=pose0, pts=Xw, obs_uv=uv, outlier=out)


def batch(seed, n_frames, n_obs=150, **kw):
    """n_frames frames as one CSR batch (obs_ptr), the lh_frames layout."""
    fs = [frame(seed, f, n_obs=n_obs if np.isscalar(n_obs) else n_obs[f], **kw) for f in range(n_frames)]
    ptr = np.zeros(n_frames + 1, np.int64)
    ptr[1:] = np.cumsum([len(x["pts"]) for x in fs])
    cat = lambda k, shape: (np.concatenate([x[k] for x in fs]) if fs else np.zeros(shape))
    return dict(n_frames=n_frames, obs_ptr=ptr,
                pose_Tcw=np.stack([x["pose_Tcw"] for x in fs]) if fs else np.zeros((0, 12)),
                pose_true=np.stack([x["pose_true"] for x in fs]) if fs else np.zeros((0, 12)),
                pts=np.ascontiguousarray(cat("pts", (0, 3)), np.float64),
                obs_uv=np.ascontiguousarray(cat("obs_uv", (0, 2)), np.float64),
                gross=cat("outlier", (0,)).astype(bool), K=K.copy())


# ------------------------------------------------------------------ derived batches
_EDGE_KEYS = ("pts", "obs_uv", "gross")


def take(fb, idx):
    """The frames `idx` of `fb`, in that order, as a batch of their own."""
    idx = [int(f) for f in idx]
    ptr = np.asarray(fb["obs_ptr"], np.int64)
    rows = (np.concatenate([np.arange(ptr[f], ptr[f + 1]) for f in idx]) if idx else np.zeros(0, np.int64)).astype(np.int64)
    out = dict(fb)
    out["n_frames"] = len(idx)
    out["obs_ptr"] = np.concatenate([[0], np.cumsum([ptr[f + 1] - ptr[f] for f in idx])]).astype(np.int64)
    out["pose_Tcw"], out["pose_true"] = fb["pose_Tcw"][idx].copy(), fb["pose_true"][idx].copy()
    for k in _EDGE_KEYS:
        out[k] = np.ascontiguousarray(fb[k][rows])
    return out


def concat(a, b):
    """The frames of `a` followed by those of `b` (same K)."""
    out = dict(a)
    out["n_frames"] = int(a["n_frames"]) + int(b["n_frames"])
    out["obs_ptr"] = np.concatenate([a["obs_ptr"], a["obs_ptr"][-1] + np.asarray(b["obs_ptr"][1:])]).astype(np.int64)
    for k in ("pose_Tcw", "pose_true") + _EDGE_KEYS:
        out[k] = np.ascontiguousarray(np.concatenate([a[k], b[k]]))
    return out


def permute_edges(fb, seed):
    """(`fb` with each frame's edges in another order, perm): edge j of the result is edge perm[j] of `fb`, so
    a per-edge output x of the result goes back to `fb`'s order as y[perm] = x.  The problem is the same one;
    only the order of the per-edge sums changes."""
    ptr = np.asarray(fb["obs_ptr"], np.int64)
    perm = np.arange(int(ptr[-1]), dtype=np.int64)
    for f in range(int(fb["n_frames"])):
        rng = np.random.default_rng([seed, f, 0x5EED])
        perm[ptr[f]:ptr[f + 1]] = ptr[f] + rng.permutation(int(ptr[f + 1] - ptr[f]))
    out = dict(fb)
    for k in _EDGE_KEYS:
        out[k] = np.ascontiguousarray(fb[k][perm])
    return out, perm


def scale_scene(fb, s):
    """The scene shrunk or grown by `s` about the world origin: points and the translation column of both
    poses times s.  Every projection is unchanged; the depths become s x (8-60 m), so the translation
    entries of H grow by 1/s^2 against the rotation ones."""
    out = dict(fb)
    out["pts"] = np.ascontiguousarray(fb["pts"] * s)
    for k in ("pose_Tcw", "pose_true"):
        p = np.array(fb[k], np.float64, copy=True).reshape(-1, 12)
        p[:, [3, 7, 11]] *= s
        out[k] = p
    return out


def ulp_nudge(fb, frame_idx, seed):
    """`fb` with every point and observation coordinate of the frames `frame_idx` moved to the next double up or
    down (a counter-based coin per coordinate)."""
    if len(frame_idx) == 0:
        return fb
    ptr = np.asarray(fb["obs_ptr"], np.int64)
    out = dict(fb, pts=fb["pts"].copy(), obs_uv=fb["obs_uv"].copy())
    for f in frame_idx:
        rng = np.random.default_rng([seed, int(f), 0x01B])
        for k in ("pts", "obs_uv"):
            a = out[k][ptr[f]:ptr[f + 1]]
            a[...] = np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))
    return out


def _hessian_diag(fb, f, huber_delta):
    """diag(H) of frame f at its start pose: J as the kernel's po_edge, W as the oracle's po_build."""
    ptr = np.asarray(fb["obs_ptr"], np.int64)
    T = np.asarray(fb["pose_Tcw"], np.float64).reshape(-1, 3, 4)[f]
    X, uv = fb["pts"][ptr[f]:ptr[f + 1]], fb["obs_uv"][ptr[f]:ptr[f + 1]]
    fx, fy, cx, cy = (float(v) for v in fb["K"])
    Pc = X @ T[:, :3].T + T[:, 3]
    x, y, z = Pc[:, 0], Pc[:, 1], Pc[:, 2]
    den = z + 1e-18
    r = np.stack([uv[:, 0] - (fx * x + cx * z) / den, uv[:, 1] - (fy * y + cy * z) / den], axis=1)
    zi = 1.0 / den
    zi2 = zi * zi
    o = np.zeros_like(x)
    J = np.stack([np.stack([-fx * zi, o, fx * x * zi2, fx * x * y * zi2, -fx - fx * x * x * zi2, fx * y * zi], 1),
                  np.stack([o, -fy * zi, fy * y * zi2, fy + fy * y * y * zi2, -fy * x * y * zi2, -fy * x * zi], 1)], 1)
    n = len(x)
    W = np.tile(np.eye(2), (n, 1, 1))
    if huber_delta > 0:
        e2 = (r * r).sum(1)
        far = e2 > huber_delta * huber_delta
        rho1 = np.where(far, huber_delta / np.sqrt(np.where(far, e2, 1.0)), 1.0)
        rho2 = np.where(far, -0.5 * rho1 / np.where(far, e2, 1.0), 0.0)
        W = rho1[:, None, None] * W
        second = rho1 + 2 * rho2 * e2 > 0.0
        W = W + np.where(second, 2 * rho2, 0.0)[:, None, None] * (r[:, :, None] * r[:, None, :])
    return np.einsum("eia,eij,eja->a", J, W, J)


def pivot_sequence(fb, f, lambda_rule=None, huber_delta=5.991, tau=1e-5, lambda_cap=5e10):
    """Eigen's LDLT transpositions (tr[k] >= k; the identity is (0, 1, 2, 3, 4, 5)) for frame f's first
    damped system, restated in numpy.  Eigen's left-looking factorisation compares diagonal entries that no
    earlier step has changed, so the sequence follows from the damped diagonal alone.  lambda_rule: None
    (lambda = tau min(cap, max diag), strategy 0), a number (lambda_init, strategy 0) or "strategy1"
    (diag (1 + 1e-5)).  Rows 0-2 are the translation, 3-5 the rotation.  A coverage measure for the tests'
    inputs: sums are in numpy's order, so a near tie may fall the other way than on the device."""
    h = _hessian_diag(fb, f, huber_delta)
    if lambda_rule is None:
        key = h + tau * min(lambda_cap, float(np.abs(h).max(initial=0.0)))
    elif isinstance(lambda_rule, str):
        assert lambda_rule == "strategy1"
        key = h + 1e-5 * h
    else:
        key = h + float(lambda_rule)
    key = np.abs(key)
    tr = []
    for k in range(6):
        idx = k
        for i in range(k + 1, 6):
            if key[i] > key[idx]:
                idx = i
        tr.append(idx)
        key[[k, idx]] = key[[idx, k]]
    return tuple(tr)


def reorder_envelope(fb, n_perm=8, is_outlier_in=None, n_thin=56, **opt):
    """How far the oracle's own answer moves when only the order of its per-edge sums changes: the oracle on
    `fb` and on n_perm edge permutations of it.  Returns dict(base = the oracle's result on `fb`, spread [F] =
    max abs pose difference to base over the permutations, iters_agree [F] = `iterations` equal in all of them,
    rchi2_spread [O] = max abs rchi2 difference per edge, in `fb`'s edge order).

    A frame of one or two edges has no order to change (a sum of two terms commutes), so its spread would be
    zero by construction while its H has rank 2 or 4 and its pose is set by rounding alone; a sum of three terms
    has three orders, so eight permutations see at most three outcomes.  On frames of fewer than four edges each
    run also moves every point and observation coordinate to a neighbouring double (ulp_nudge): the smallest
    perturbation of the same solve that reaches the oracle's sums at all.  Such a frame is cheap and, with the
    Huber gate of its few edges on a rounding residue, takes one of a few trajectories
    through rounds one to three, the rarer ones in about one run of eight: these frames get n_thin further
    nudged runs on their own."""
    import oracle_bind as ob
    fin = None if is_outlier_in is None else np.asarray(is_outlier_in)
    base = ob.estimate_pose(fb, is_outlier_in=fin, **opt)
    ptr = np.asarray(fb["obs_ptr"], np.int64)
    F, O = int(fb["n_frames"]), int(ptr[-1])
    spread, agree, rs = np.zeros(F), np.ones(F, bool), np.zeros(O)
    thin = np.nonzero(np.diff(ptr) < 4)[0]

    def fold(o, fr, rows, perm):
        """a perturbed run `o` of the frames `fr` (edges `rows` of fb, shuffled by perm) into the envelope"""
        d = np.abs(o["pose_Tcw"] - base["pose_Tcw"][fr]).reshape(len(fr), -1).max(axis=1, initial=0.0)
        spread[fr] = np.maximum(spread[fr], d)
        agree[fr] &= o["iterations"] == base["iterations"][fr]
        back = np.zeros(len(rows))
        back[perm] = o["rchi2"]
        with np.errstate(invalid="ignore"):
            rs[rows] = np.fmax(rs[rows], np.abs(back - base["rchi2"][rows]))

    for p in range(n_perm):
        fp, perm = permute_edges(fb, p + 1)
        fp = ulp_nudge(fp, thin, p + 1)
        fold(ob.estimate_pose(fp, is_outlier_in=None if fin is None else fin[perm], **opt), np.arange(F), np.arange(O), perm)
    if len(thin):
        rows = np.concatenate([np.arange(ptr[f], ptr[f + 1]) for f in thin]).astype(np.int64)
        sub = take(fb, thin)
        for p in range(n_thin):
            o = ob.estimate_pose(ulp_nudge(sub, range(len(thin)), n_perm + p + 1),
                                 is_outlier_in=None if fin is None else fin[rows], **opt)
            fold(o, thin, rows, np.arange(len(rows)))
    return dict(base=base, spread=spread, iters_agree=agree, rchi2_spread=rs)
