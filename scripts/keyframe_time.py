"""Times of lh_insert_keyframe on the MI355X: a keyframe's detector, right-image tracker and
triangulation on a 1241 x 376 stereo pair at the reference's parameters (GFTT 150 / 0.01 / 20 with the boxes of +-10 around
the features the frame has, KLT 11 x 11 / 3 levels / 30 / 0.01), with about 100 features of which 80 % carry a map point
(InsertKeyframe) and with none (StereoInit); at most 150 new corners in both, the detector's own limit.  A third
shape, not the reference's, has a limit of 2 000 that the list does not reach: its slots past the list's end idle.  Three
variants, alternated call by call in one process after a warm-up:
  fused, both images     Solver.insert_keyframe(left, right, ...)
  fused, resident image  Solver.insert_keyframe(None, right, ...) after an untimed lh_track_frame priming call that makes
                         `left` resident (in the frontend, the frame's own lh_track_frame has done that)
  composed               the caller's sequence: Solver.detect_features, the list and track_ref.guess on the host,
                         Solver.klt_stereo_landmarks (its parts are listed below it; time_ms is the sum of the two calls')
time_ms is the HIP-event bracket from the first kernel to the last (copies excluded; the detector's host checks between
selection rounds included); wall is the host clock around the whole variant, the Python binding included in each.
Median and range of `reps` calls.  The three must agree bit for bit.

usage: python3 scripts/keyframe_time.py [reps] > profiles/keyframe_time.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "lego-slam_amd", "python")]
import numpy as np          # noqa: E402
import images               # noqa: E402
import keyframe_ref as kf   # noqa: E402
import lego_ba              # noqa: E402
import track_ref as tk      # noqa: E402
import triangulate_ref as tr   # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
ROWS, COLS = 376, 1241
K = np.array([718.856, 718.856, 607.1928, 185.2157])
DEPTH = 20.0
cam_pose, cam_K = tr.stereo_poses(6.0 * DEPTH / K[0]), np.stack([K, K])
GATE = (2.0, 5.0, 40.0)
NUM_FEATURES = 150


def have(n, seed=11):
    if n == 0:
        return None, None, None
    kp = images.keypoints(ROWS, COLS, n, seed=seed, border=False)
    rng = np.random.default_rng(seed)
    z = DEPTH * rng.uniform(0.8, 1.25, n)
    X = np.stack([(kp[:, 0] - K[2]) / K[0] * z, (kp[:, 1] - K[3]) / K[1] * z, z], 1)
    return kp, X, (rng.uniform(size=n) < 0.8).astype(np.uint8)


def line(name, dev, wall):
    d = "" if dev is None else f"time_ms median {np.median(dev):8.4f} (min {min(dev):.4f}, max {max(dev):.4f})"
    print(f"{name:<62} {d:<50} wall ms median {np.median(wall):8.3f} (min {min(wall):.3f}, max {max(wall):.3f})")


def same(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=np.asarray(a[k]).dtype.kind == "f") for k in kf.KEYS)


s = lego_ba.Solver()
left, right = images.pair(ROWS, COLS, shift=(-6.0, 0.0), seed=11)
none = np.zeros((0, 2), np.float32)
for n_have, limit in ((100, NUM_FEATURES), (0, NUM_FEATURES), (100, 2000)):
    kp, X, hp = have(n_have)
    kw = dict(max_corners=limit, gate=GATE)
    t = {k: [] for k in ("both", "resident", "composed", "detect", "host", "stereo")}
    d = {k: [] for k in ("both", "resident", "composed", "detect", "stereo")}
    clock = time.perf_counter
    for rep in range(-3, reps):
        t0 = clock()
        both = s.insert_keyframe(left, right, kp, X, hp, tk.IDENTITY, cam_pose, cam_K, **kw)
        t1 = clock()
        s.track_frame(None, left, none, None, None, tk.IDENTITY, K)   # untimed: `left` becomes the resident image
        t2 = clock()
        res = s.insert_keyframe(None, right, kp, X, hp, tk.IDENTITY, cam_pose, cam_K, **kw)
        t3 = clock()
        det = s.detect_features(left, exclude=kp, max_corners=kw["max_corners"])
        t4 = clock()
        _, kl, hp_all, X_all = kf.feature_list(kp, X, hp, det["kp"])
        g = tk.guess(X_all, hp_all, kl, tk.IDENTITY, cam_pose[1], cam_K[1])
        t5 = clock()
        st = s.klt_stereo_landmarks(left, right, kl, cam_pose, K=cam_K, kp_right_init=g, gate=GATE)
        t6 = clock()
        if rep < 0:
            continue
        for k, v in (("both", t1 - t0), ("resident", t3 - t2), ("composed", t6 - t3), ("detect", t4 - t3), ("host", t5 - t4),
                     ("stereo", t6 - t5)):
            t[k].append(v * 1e3)
        for k, v in (("both", both["time_ms"]), ("resident", res["time_ms"]), ("detect", det["time_ms"]),
                     ("stereo", st["time_ms"]), ("composed", det["time_ms"] + st["time_ms"])):
            d[k].append(v)
    comp = kf.compose(s, left, right, kp, X, hp, tk.IDENTITY, cam_pose, cam_K, **kw)
    n_pt = 0 if hp is None else int(hp.sum())
    print(f"1241x376, {n_have} features ({n_pt} with a point), at most {kw['max_corners']} new: candidates {both['n_candidates']}, "
          f"corners {both['n_new']}, tracked {both['n_right']} of {n_have + both['n_new']}, accepted {both['n_accepted']}; "
          f"fused == resident == composed: {same(both, res) and same(both, comp)}")
    line("  lh_insert_keyframe, both images", d["both"], t["both"])
    line("  lh_insert_keyframe, resident left image", d["resident"], t["resident"])
    line("  composed: detect_features + list, guess + klt_stereo_landmarks", d["composed"], t["composed"])
    line("      lh_detect_features", d["detect"], t["detect"])
    line("      the list and track_ref.guess (host, NumPy)", None, t["host"])
    line("      lh_klt_stereo_landmarks", d["stereo"], t["stereo"])
s.close()
