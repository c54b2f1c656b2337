"""Times of lh_detect_features on the MI355X: a 1241 x 376 image with the frontend's parameters
(150 corners, quality 0.01, min_distance 20, 100 exclusion points), the same image with 2 000 corners at
min_distance 5, and the frontend's sequence detect -> lh_stereo_landmarks.  time_ms is the HIP-event bracket from
the first kernel to the last (it includes the host's checks between batches of selection rounds; copies of the
inputs and outputs are excluded); wall is the host clock around the whole call.  Median and range of `reps` calls
after a warm-up.  Beside each detector case: the single-thread time of the same arithmetic compiled for the host
(tests/gftt_probe.cpp on lego-slam_amd/csrc/lh_gftt.h), whose corners must equal the device's.

usage: python3 scripts/detect_time.py [reps] > profiles/detect_time.txt"""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "lego-slam_amd", "python")]
import numpy as np          # noqa: E402
import gftt_ref as gr       # noqa: E402
import images               # noqa: E402
import lego_ba              # noqa: E402
import triangulate_ref as tr  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30


def timed(name, call, dev_key="time_ms"):
    for _ in range(3):
        call()
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(r[dev_key])
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
host = gr.host_library(tempfile.mkdtemp())
left, right = images.pair(376, 1241, shift=(-6.0, 0.0), seed=11)
have = images.keypoints(376, 1241, 100, seed=11, border=False)
for label, kw in (("frontend: 150 corners, 0.01, 20, 100 exclusion points", dict(exclude=have)),
                  ("2000 corners, 0.01, min_distance 5", dict(max_corners=2000, min_distance=5.0))):
    g = timed(f"lh_detect_features, 1241x376, {label}", lambda: s.detect_features(left, **kw))
    c = host_timed("    the same arithmetic on the host, one thread", lambda: gr.host_detect(host, left, **kw))
    same = np.array_equal(g["kp"], c["kp"]) and g["n_candidates"] == c["n_candidates"]
    print(f"    candidates {g['n_candidates']}, corners {g['n_corners']}, lambda_max {g['lambda_max']:.1f}, "
          f"host corners equal: {same}")
poses, Ks = tr.stereo_poses(), np.stack([tr.K, tr.K])


def sequence():
    d = s.detect_features(left, exclude=have)
    st = s.stereo_landmarks(left, right, d["kp"], poses, K=Ks, kp_right_init=d["kp"], gate=(2.0, 3.0, 80.0))
    st["time_ms"] += d["time_ms"]
    return st


r = timed("detect -> lh_stereo_landmarks, 1241x376, frontend parameters", sequence)
print(f"    tracked {int(r['success'].sum())}, accepted {r['n_accepted']}")
s.close()
