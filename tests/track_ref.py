"""NumPy restatement of lh_track_frame's own steps (include/lego_ba.h): the tracker's guesses and the
edge selection, and the composition of the library's other entry points that the fused call must equal bit for bit.

NumPy's elementwise float64 operations are single correctly rounded operations and never fuse, so guess() is bitwise
lego-slam_amd/csrc/lh_track.h compiled for the host (tests/track_probe.cpp, -ffp-contract=off)."""
import ctypes as C
import os
import subprocess

import numpy as np

IDENTITY = np.array([1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])


def _rigid(M, x):
    """((m0 x0 + m1 x1) + m2 x2) + m3 per row of the row-major [R|t] M, on the columns x"""
    M = np.asarray(M, np.float64).reshape(3, 4)
    return [((M[r, 0] * x[0] + M[r, 1] * x[1]) + M[r, 2] * x[2]) + M[r, 3] for r in range(3)]


def guess(pts_w, has_point, kp1, pose, ext, K):
    """The tracker's guesses [n, 2] float32: Camera::world2pixel of the map point at the predicted pose where the
    feature has a point (has_point None: everywhere), kp1 elsewhere.  A float past FLT_MAX is +-inf."""
    kp1 = np.asarray(kp1, np.float32).reshape(-1, 2)
    n = len(kp1)
    hp = np.ones(n, bool) if has_point is None else np.asarray(has_point).astype(bool)
    if pts_w is None:
        assert not hp.any()
        return kp1.copy()
    X = np.asarray(pts_w, np.float64).reshape(n, 3)
    K = np.asarray(K, np.float64)
    with np.errstate(all="ignore"):
        Pc = _rigid(ext, _rigid(pose, [X[:, 0], X[:, 1], X[:, 2]]))
        u = (K[0] * Pc[0]) / Pc[2] + K[2]
        v = (K[1] * Pc[1]) / Pc[2] + K[3]
        g = np.stack([u, v], 1).astype(np.float32)
    return np.where(hp[:, None], g, kp1)


def select(success, has_point, kp2, pts_w):
    """The edges: the features with success and a point, ascending.  dict(idx, pts [m, 3], uv [m, 2] kp2 widened)."""
    ok = np.asarray(success).astype(bool)
    hp = np.ones(len(ok), bool) if has_point is None else np.asarray(has_point).astype(bool)
    idx = np.flatnonzero(ok & hp)
    pts = np.zeros((0, 3)) if pts_w is None else np.asarray(pts_w, np.float64).reshape(-1, 3)[idx]
    return dict(idx=idx, pts=np.ascontiguousarray(pts),
                uv=np.ascontiguousarray(np.asarray(kp2, np.float32).reshape(-1, 2)[idx].astype(np.float64)))


def frame_batch(sel, pose, K):
    """The one-frame batch (tests/frames.py layout) of a selection."""
    return dict(n_frames=1, obs_ptr=np.array([0, len(sel["idx"])], np.int64), pose_Tcw=np.asarray(pose, np.float64).reshape(1, 12),
                pts=sel["pts"], obs_uv=sel["uv"], K=np.asarray(K, np.float64))


def compose(solver, img_last, img_cur, kp1, pts_w, has_point, pose, K, cam_ext=None, **klt):
    """Frontend::Track as three calls with the host in between: guess -> klt_track -> select -> estimate_pose.
    Returns what Solver.track_frame returns (time_ms: the sum of the two device times)."""
    kp1 = np.asarray(kp1, np.float32).reshape(-1, 2)
    n = len(kp1)
    ext = IDENTITY if cam_ext is None else cam_ext
    out = dict(pose_Tcw=np.asarray(pose, np.float64).reshape(12).copy(), is_outlier=np.zeros(n, bool), edge_chi2=np.zeros(n),
               n_tracked=0, n_edges=0, n_inliers=0, iterations=0, time_ms=0.0, kp2=np.zeros((0, 2), np.float32),
               success=np.zeros(0, bool))
    if n == 0:
        return out
    t = solver.klt_track(img_last, img_cur, kp1, kp2_init=guess(pts_w, has_point, kp1, pose, ext, K), **klt)
    sel = select(t["success"], has_point, t["kp2"], pts_w)
    e = solver.estimate_pose(frame_batch(sel, pose, K))
    out.update(kp2=t["kp2"], success=t["success"], pose_Tcw=e["pose_Tcw"].reshape(12), n_tracked=int(t["success"].sum()),
               n_edges=len(sel["idx"]), n_inliers=int(e["n_inliers"][0]), iterations=int(e["iterations"][0]),
               time_ms=t["time_ms"] + e["time_ms"])
    out["is_outlier"][sel["idx"]] = e["is_outlier"]
    out["edge_chi2"][sel["idx"]] = e["edge_chi2"]
    return out


def host_library(build_dir):
    here = os.path.dirname(os.path.abspath(__file__))
    so = os.path.join(str(build_dir), "libtrack_probe.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-I",
                           os.path.join(os.path.dirname(here), "lego-slam_amd", "csrc"),
                           os.path.join(here, "track_probe.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.track_guess.argtypes = [C.c_int] + [C.c_void_p] * 7
    lib.track_guess.restype = None
    return lib


def host_guess(lib, pts_w, has_point, kp1, pose, ext, K):
    kp1 = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
    n = len(kp1)
    X = np.ascontiguousarray(pts_w, np.float64).reshape(n, 3)
    hp = None if has_point is None else np.ascontiguousarray(has_point, np.uint8)
    T, E, Kk = (np.ascontiguousarray(a, np.float64) for a in (pose, ext, K))
    out = np.zeros((n, 2), np.float32)
    lib.track_guess(n, X.ctypes.data, None if hp is None else hp.ctypes.data, kp1.ctypes.data, T.ctypes.data, E.ctypes.data,
                    Kk.ctypes.data, out.ctypes.data)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])
