"""lh_insert_keyframe's definition (include/lego_ba.h) twice over: compose(), the three calls of the
library with the host in between that the fused call must equal bit for bit, and reference(), the same chain on the
NumPy references of the three parts, which needs no GPU.  scene() is the keyframe both test files run."""
import functools

import numpy as np

import gftt_ref
import images
import klt_ref
import track_ref as tk
import triangulate_ref as tr

F_HAS_POINT = 32
KEYS = ("kp_new", "kp_right", "success", "pt", "flags", "n_new", "n_candidates", "lambda_max", "n_right", "n_accepted")

ROWS, COLS = 121, 163
K = np.array([517.3, 516.5, COLS / 2, ROWS / 2])
DEPTH = 20.0
BASELINE = 6.0 * DEPTH / K[0]      # a disparity of 6 pixels at DEPTH: images.pair's shift of (-6, 0)
GATE = (0.4, 5.0, 24.0)


def _has(have_point, n):
    return np.ones(n, bool) if have_point is None else np.asarray(have_point).astype(bool)


def _finish(kl, n_have, have_point, det, st):
    """The result dict of Solver.insert_keyframe from the detector's and the stereo call's."""
    hp = np.concatenate([_has(have_point, n_have), np.zeros(len(kl) - n_have, bool)])
    pt, flags = st["pt"].copy(), st["flags"].copy()
    pt[hp] = 0.0
    flags[hp] = F_HAS_POINT
    return dict(kp_new=det["kp"], kp_right=st["kp2"], success=np.asarray(st["success"], bool), pt=pt, flags=flags,
                n_new=int(det["n_corners"]), n_candidates=int(det["n_candidates"]), lambda_max=float(det["lambda_max"]),
                n_right=int(np.sum(st["success"])), n_accepted=int(np.sum(flags == 0)),
                time_ms=det.get("time_ms", 0.0) + st.get("time_ms", 0.0))


def feature_list(have_kp, have_pts_w, have_point, corners):
    """kl (have_kp, then the corners) and every feature's points and has_point bytes (a corner has none)."""
    have = np.zeros((0, 2), np.float32) if have_kp is None else np.asarray(have_kp, np.float32).reshape(-1, 2)
    nh, m = len(have), len(corners)
    kl = np.concatenate([have, np.asarray(corners, np.float32).reshape(-1, 2)])
    hp = np.concatenate([_has(have_point, nh), np.zeros(m, bool)]).astype(np.uint8)
    X = None
    if have_pts_w is not None:
        X = np.concatenate([np.asarray(have_pts_w, np.float64).reshape(nh, 3), np.zeros((m, 3))])
    return have, kl, hp, X


def compose(solver, img_left, img_right, have_kp, have_pts_w, have_point, pose, cam_pose, cam_K, max_corners=150, quality=0.01,
            min_distance=20.0, exclude_half=10.0, max_level=3, max_iters=30, epsilon=0.01, min_eig=1e-4, thr=1e-3, gate=None,
            T_out=None):
    """detect_features -> track_ref.guess (the right camera) -> klt_stereo_landmarks(kp_right_init = guess), then flag 32
    and pt = 0 where the feature has a point.  Returns what Solver.insert_keyframe returns."""
    have = np.zeros((0, 2), np.float32) if have_kp is None else np.asarray(have_kp, np.float32).reshape(-1, 2)
    det = solver.detect_features(img_left, exclude=have if len(have) else None, max_corners=max_corners, quality=quality,
                                 min_distance=min_distance, exclude_half=exclude_half)
    have, kl, hp, X = feature_list(have, have_pts_w, have_point, det["kp"])
    cam_pose, cam_K = np.asarray(cam_pose, np.float64).reshape(2, 12), np.asarray(cam_K, np.float64).reshape(2, 4)
    if len(kl) == 0:
        st = dict(kp2=np.zeros((0, 2), np.float32), success=np.zeros(0, bool), pt=np.zeros((0, 3)), flags=np.zeros(0, np.uint8))
    else:
        g = tk.guess(X, hp, kl, pose, cam_pose[1], cam_K[1])
        st = solver.klt_stereo_landmarks(img_left, img_right, kl, cam_pose, K=cam_K, kp_right_init=g, max_level=max_level,
                                         max_iters=max_iters, epsilon=epsilon, min_eig=min_eig, thr=thr, gate=gate, T_out=T_out)
    return _finish(kl, len(have), have_point, det, st)


def reference(img_left, img_right, have_kp, have_pts_w, have_point, pose, cam_pose, cam_K, max_corners=150, quality=0.01,
              min_distance=20.0, exclude_half=10.0, max_level=3, max_iters=30, epsilon=0.01, min_eig=1e-4, thr=1e-3, gate=None,
              T_out=None):
    """The same chain on gftt_ref.detect_ref, klt_ref.track and triangulate_ref.triangulate_ref."""
    have = np.zeros((0, 2), np.float32) if have_kp is None else np.asarray(have_kp, np.float32).reshape(-1, 2)
    det = gftt_ref.detect_ref(img_left, exclude=have if len(have) else None, max_corners=max_corners, quality=quality,
                              min_distance=min_distance, exclude_half=exclude_half)
    have, kl, hp, X = feature_list(have, have_pts_w, have_point, det["kp"])
    cam_pose, cam_K = np.asarray(cam_pose, np.float64).reshape(2, 12), np.asarray(cam_K, np.float64).reshape(2, 4)
    n = len(kl)
    st = dict(kp2=np.zeros((n, 2), np.float32), success=np.zeros(n, bool), pt=np.zeros((n, 3)), flags=np.zeros(n, np.uint8))
    if n:
        g = tk.guess(X, hp, kl, pose, cam_pose[1], cam_K[1])
        t = klt_ref.track(img_left, img_right, kl, kp2_init=g, max_level=max_level, max_iters=max_iters, epsilon=epsilon,
                          min_eig=min_eig)
        st["kp2"], st["success"] = t["kp2"], t["success"]
        ok = np.flatnonzero(t["success"])
        st["flags"][~t["success"]] = tr.F_TRACK
        if len(ok):
            xy = np.stack([kl[ok].astype(np.float64), t["kp2"][ok].astype(np.float64)], 1)   # toVec2: [m, 2 views, 2]
            r = tr.triangulate_ref(cam_pose, xy, K=cam_K, thr=thr, gate=gate, T_out=T_out)
            st["pt"][ok], st["flags"][ok] = r["pt"], r["flags"]
    return _finish(kl, len(have), have_point, det, st)


def literal_flags(success, has_point, tri_flags):
    """Frontend::TriangulateNewPoints' own conditions, feature by feature (frontend_lego.cpp:116-117): a feature with a map
    point is skipped, one without a right-image match is skipped, the others are triangulated."""
    out = []
    for ok, hp, f in zip(success, has_point, tri_flags):
        if hp:                      # !features_left_[i]->map_point_.expired()
            out.append(F_HAS_POINT)
        elif not ok:                # features_right_[i] == nullptr
            out.append(tr.F_TRACK)
        else:
            out.append(int(f))
    return np.array(out, np.uint8)


def cameras(baseline=BASELINE):
    """cam_pose [2, 12] (the right camera -baseline along x) and cam_K [2, 4]"""
    return tr.stereo_poses(baseline), np.stack([K, K])


@functools.lru_cache(maxsize=None)
def scene(n_have=40, seed=3):
    """A 121 x 163 stereo pair with a disparity of 6 pixels; n_have features the frame has, 60 % of them with a map point
    at 0.8 .. 1.25 x DEPTH on their own ray; the frame at the identity."""
    left, right = images.pair(ROWS, COLS, shift=(-6.0, 0.0), seed=11)
    have = images.keypoints(ROWS, COLS, n_have, seed=seed, border=False)
    rng = np.random.default_rng(seed + 50)
    z = DEPTH * rng.uniform(0.8, 1.25, n_have)
    X = np.stack([(have[:, 0] - K[2]) / K[0] * z, (have[:, 1] - K[3]) / K[1] * z, z], 1)
    hp = (rng.uniform(size=n_have) < 0.6).astype(np.uint8)
    cam_pose, cam_K = cameras()
    for a in (left, right, have, X, hp, cam_pose, cam_K):
        a.setflags(write=False)
    return dict(img_left=left, img_right=right, have_kp=have, have_pts_w=X, have_point=hp, pose=tk.IDENTITY, cam_pose=cam_pose,
                cam_K=cam_K, max_corners=40, min_distance=8.0, gate=GATE)


def call(fn, sc, **kw):
    """fn(img_left, img_right, have_kp, have_pts_w, have_point, pose, cam_pose, cam_K, **the rest) on a scene dict."""
    a = dict(sc)
    a.update(kw)
    head = [a.pop(k) for k in ("img_left", "img_right", "have_kp", "have_pts_w", "have_point", "pose", "cam_pose", "cam_K")]
    return fn(*head, **a)
