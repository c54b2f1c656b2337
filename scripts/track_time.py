"""Times of lh_track_frame on the MI355X: one frame of Frontend::Track on a 1241 x 376 pair at the
reference's KLT parameters, with 150 and with 2 000 features of which 80 % carry a map point.  Three variants,
alternated call by call in one process after a warm-up:
  fused, both images     Solver.track_frame(img_last, img_cur, ...)
  fused, resident image  Solver.track_frame(None, img_cur, ...) after an untimed priming call that makes img_last resident
  composed               the caller's sequence: track_ref.guess on the host, Solver.klt_track, track_ref.select on the
                         host, Solver.estimate_pose (its parts are listed below it; time_ms is the sum of the two calls')
time_ms is the HIP-event bracket from the first kernel to the last (copies excluded); wall is the host clock around the
whole variant, the Python binding included in each.  Median and range of `reps` calls.  The three must agree bit for bit.

usage: python3 scripts/track_time.py [reps] > profiles/track_time.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "lego-slam_amd", "python")]
import numpy as np          # noqa: E402
import images               # noqa: E402
import lego_ba              # noqa: E402
import track_ref as tk      # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
ROWS, COLS = 376, 1241
SHIFT = (2.3, -1.7)
K = np.array([718.856, 718.856, 607.1928, 185.2157])
KEYS = ("kp2", "success", "pose_Tcw", "is_outlier", "edge_chi2", "n_tracked", "n_edges", "n_inliers", "iterations")


def frame(n, seed=11):
    kp1 = images.keypoints(ROWS, COLS, n, seed=seed, border=False)
    rng = np.random.default_rng(seed)
    z = rng.uniform(8, 60, n)
    X = np.stack([(kp1[:, 0] - K[2]) / K[0] * z, (kp1[:, 1] - K[3]) / K[1] * z, z], 1)
    hp = (rng.uniform(size=n) < 0.8).astype(np.uint8)
    pitch, yaw = -0.6 * SHIFT[1] / K[1], 0.6 * SHIFT[0] / K[0]
    cp, sp, cy, sy = np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    R = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    return kp1, X, hp, np.hstack([R, np.array([[0.004], [-0.003], [0.006]])]).reshape(12)


def line(name, dev, wall):
    d = "" if dev is None else f"time_ms median {np.median(dev):8.4f} (min {min(dev):.4f}, max {max(dev):.4f})"
    print(f"{name:<58} {d:<50} wall ms median {np.median(wall):8.3f} (min {min(wall):.3f}, max {max(wall):.3f})")


def same(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=np.asarray(a[k]).dtype.kind == "f") for k in KEYS)


s = lego_ba.Solver()
last, cur = images.pair(ROWS, COLS, shift=SHIFT, seed=11)
none = np.zeros((0, 2), np.float32)
for n in (150, 2000):
    kp1, X, hp, pose = frame(n)
    t = {k: [] for k in ("both", "resident", "composed", "guess", "klt", "select", "pose")}
    d = {k: [] for k in ("both", "resident", "composed", "klt", "pose")}
    clock = time.perf_counter
    for rep in range(-3, reps):
        t0 = clock()
        both = s.track_frame(last, cur, kp1, X, hp, pose, K)
        t1 = clock()
        s.track_frame(None, last, none, None, None, pose, K)   # untimed: `last` becomes the resident image
        t2 = clock()
        res = s.track_frame(None, cur, kp1, X, hp, pose, K)
        t3 = clock()
        g = tk.guess(X, hp, kp1, pose, tk.IDENTITY, K)
        t4 = clock()
        kl = s.klt_track(last, cur, kp1, kp2_init=g)
        t5 = clock()
        sel = tk.select(kl["success"], hp, kl["kp2"], X)
        fb = tk.frame_batch(sel, pose, K)
        t6 = clock()
        e = s.estimate_pose(fb)
        t7 = clock()
        if rep < 0:
            continue
        for k, v in (("both", t1 - t0), ("resident", t3 - t2), ("composed", t7 - t3), ("guess", t4 - t3), ("klt", t5 - t4),
                     ("select", t6 - t5), ("pose", t7 - t6)):
            t[k].append(v * 1e3)
        for k, v in (("both", both["time_ms"]), ("resident", res["time_ms"]), ("klt", kl["time_ms"]), ("pose", e["time_ms"]),
                     ("composed", kl["time_ms"] + e["time_ms"])):
            d[k].append(v)
    comp = tk.compose(s, last, cur, kp1, X, hp, pose, K)
    print(f"1241x376, {n} features ({int(hp.sum())} with a point): tracked {both['n_tracked']}, edges {both['n_edges']}, "
          f"inliers {both['n_inliers']}, LM iterations {both['iterations']}; fused == resident == composed: "
          f"{same(both, res) and same(both, comp)}")
    line("  lh_track_frame, both images", d["both"], t["both"])
    line("  lh_track_frame, resident image", d["resident"], t["resident"])
    line("  composed: guess + klt_track + select + estimate_pose", d["composed"], t["composed"])
    line("      track_ref.guess (host, NumPy)", None, t["guess"])
    line("      lh_klt_track", d["klt"], t["klt"])
    line("      track_ref.select (host, NumPy)", None, t["select"])
    line("      lh_estimate_pose", d["pose"], t["pose"])
s.close()
