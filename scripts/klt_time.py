"""Times of lh_klt_track on the MI355X: a 1241 x 376 pair at the reference's parameters (11 x 11,
max_level 3, 30 iterations, epsilon 0.01, has_initial with kp2 = kp1) with 2 000 and with 150 keypoints,
lh_klt_stereo_landmarks on the 2 000, and, for scale, lh_lk_track on the same input.  time_ms is the HIP-event
bracket from the first kernel to the last (copies of the inputs and outputs excluded); wall is the host clock around
the whole call.  Median and range of `reps` calls after a warm-up.  Beside each tracker case: the single-thread time
of the same arithmetic compiled for the host (tests/klt_probe.cpp on lego-slam_amd/csrc/lh_klt.h), whose kp2 and
success must equal the device's.

usage: python3 scripts/klt_time.py [reps] > profiles/klt_time.txt"""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "lego-slam_amd", "python")]
import numpy as np          # noqa: E402
import images               # noqa: E402
import klt_ref as kr        # noqa: E402
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
    print(f"{name:<62} time_ms median {np.median(dev):8.4f} (min {min(dev):.4f}, max {max(dev):.4f})   "
          f"wall ms median {np.median(wall):8.3f} (min {min(wall):.3f}, max {max(wall):.3f})")
    return r


def host_timed(name, call):
    call()
    wall = []
    for _ in range(max(5, reps // 3)):
        t0 = time.perf_counter()
        r = call()
        wall.append((time.perf_counter() - t0) * 1e3)
    print(f"{name:<62} {'':<48} wall ms median {np.median(wall):8.3f} (min {min(wall):.3f}, max {max(wall):.3f})")
    return r


s = lego_ba.Solver()
host = kr.host_library(tempfile.mkdtemp())
left, right = images.pair(376, 1241, shift=(-6.0, 0.0), seed=11)
poses, Ks = tr.stereo_poses(), np.stack([tr.K, tr.K])
for n in (2000, 150):
    k1 = images.keypoints(376, 1241, n, seed=11, border=False)
    g = timed(f"lh_klt_track, 1241x376, {n} keypoints, the reference's parameters", lambda: s.klt_track(left, right, k1, kp2_init=k1))
    c = host_timed("    the same arithmetic on the host, one thread", lambda: kr.host_track(host, left, right, k1, k1))
    same = np.array_equal(kr.bits(g["kp2"]), kr.bits(c["kp2"])) and np.array_equal(g["success"], c["success"])
    print(f"    tracked {int(g['success'].sum())} of {n}, host result equal: {same}")
k1 = images.keypoints(376, 1241, 2000, seed=11, border=False)
r = timed("lh_klt_stereo_landmarks, 1241x376, 2000 keypoints",
          lambda: s.klt_stereo_landmarks(left, right, k1, poses, K=Ks, kp_right_init=k1, gate=(2.0, 3.0, 80.0)))
print(f"    tracked {int(r['success'].sum())}, accepted {r['n_accepted']}")
r = timed("lh_lk_track (Gauss-Newton, 4 levels), the same input, for scale", lambda: s.lk_track(left, right, k1, kp2_init=k1))
print(f"    tracked {int(r['success'].sum())}")
s.close()
