"""Device times of the triangulation entry points on the MI355X: lh_triangulate on 2 000 stereo
points and on 2 048 x 150 points in one call, and lh_stereo_landmarks on a 1241 x 376 pair with 2 000 keypoints
next to lh_lk_track alone on the same input.  time_ms is the HIP-event bracket around the kernels (copies
excluded); wall is the host clock around the whole call.  Median and range of `reps` calls after a warm-up.

usage: python3 scripts/triangulate_time.py [reps] > profiles/triangulate_time.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "lego-slam_amd", "python")]
import numpy as np          # noqa: E402
import images               # noqa: E402
import lego_ba              # noqa: E402
import triangulate_ref as tr  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30


def timed(name, call):
    for _ in range(3):
        call()
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(r["time_ms"])
    print(f"{name:<58} time_ms median {np.median(dev):8.4f} (min {min(dev):.4f}, max {max(dev):.4f})   "
          f"wall ms median {np.median(wall):8.3f} (min {min(wall):.3f}, max {max(wall):.3f})")
    return r


s = lego_ba.Solver()
poses = tr.stereo_poses()
Ks = np.stack([tr.K, tr.K])
for n in (2000, 2048 * 150):
    _, px, _ = tr.stereo_family(n, seed=1)
    r = timed(f"lh_triangulate, {n} stereo points (2 views, cam_K)", lambda: s.triangulate(poses, px, K=Ks))
    print(f"    accepted {r['n_accepted']} of {n}")
left, right = images.pair(376, 1241, shift=(-6.0, 0.0), seed=11)
k1 = images.keypoints(376, 1241, 2000, seed=11, border=False)
r = timed("lh_lk_track, 1241x376, 2000 keypoints", lambda: s.lk_track(left, right, k1, kp2_init=k1))
print(f"    tracked {int(r['success'].sum())}")
r = timed("lh_stereo_landmarks, 1241x376, 2000 keypoints",
          lambda: s.stereo_landmarks(left, right, k1, poses, K=Ks, kp_right_init=k1, gate=(2.0, 3.0, 80.0)))
print(f"    tracked {int(r['success'].sum())}, accepted {r['n_accepted']}")
s.close()
