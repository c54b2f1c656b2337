"""Times of lh_marginalize on the MI355X, after a solve on the same handle.  Two windows:
  C3         20 keyframes, 50 k landmarks, 400 k observations, pose 0 fixed (the bench workload), m = 1,
             degenerate_guard 1 (scripts/cov_time.py says why);
  reference  15 keyframes (map.h:82), 2 000 landmarks, no fixed pose, m = 0 (the oldest keyframe), as the backend
             would call it before Map::RemoveOldKeyframe.
time_ms is the call's HIP-event bracket (mask, snapshot, linearisation, assembly, elimination; the download excluded);
wall is the host clock around Solver.marginalize, the Python binding and the download included.  Median and range of
`reps` calls after a warm-up, alternated call by call with lh_covariance's poses-only call (anchor 0 on the window
without a fixed pose); for scale, the solve's own time_ms on the same handle (lh_solve_resident, array-free).

usage: python3 scripts/marg_time.py [reps] > profiles/marg_time.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "lego-slam_amd", "python")]
import numpy as np     # noqa: E402
import lego_ba         # noqa: E402
import windows         # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30


def line(name, dev, wall):
    print(f"  {name:<34} time_ms median {np.median(dev):8.4f} (min {min(dev):.4f}, max {max(dev):.4f})   "
          f"wall ms median {np.median(wall):8.3f} (min {min(wall):.3f}, max {max(wall):.3f})")


ref15 = lego_ba.generate_window(P=15, L=2000, k=8, seed=1, **windows.STABLE)   # (no pose_fixed: the live configuration)
for title, w, m, anchor, guard in (("C3: 20 keyframes, pose 0 fixed, m = 1, degenerate_guard 1", windows.window("C3", seed=1, family="stable"), 1, -1, 1),
                                   ("reference-sized: 15 keyframes, no fixed pose, m = 0", ref15, 0, 0, 0)):
    s = lego_ba.Solver(degenerate_guard=guard)
    s.upload(w)
    solve_ms = []
    for rep in range(-3, reps):
        r = s.solve_resident()
        if rep >= 0:
            solve_ms.append(r["time_ms"])
    P, L = w["n_poses"], len(w["lm_xyz"])
    out = dict(H_prior=np.zeros((6 * P, 6 * P)), b_prior=np.zeros(6 * P), lm_marginalised=np.zeros(L, np.uint8))
    dev = {"marg": [], "cov": []}
    wall = {"marg": [], "cov": []}
    for rep in range(-3, reps):
        t0 = time.perf_counter()
        c = s.marginalize(m, out=out)
        t1 = time.perf_counter()
        v = s.covariance(anchor=anchor)
        t2 = time.perf_counter()
        if rep >= 0:
            dev["marg"].append(c["time_ms"])
            wall["marg"].append((t1 - t0) * 1e3)
            dev["cov"].append(v["time_ms"])
            wall["cov"].append((t2 - t1) * 1e3)
    print(f"{title}: {L} landmarks, {len(w['obs_pose'])} observations; marginalised {c['n_landmarks']} landmarks, "
          f"{c['n_edges']} edges, {c['n_degenerate']} rank-deficient, pivots {c['min_pivot']:.3e} .. {c['max_pivot']:.3e}, {reps} calls")
    line("lh_marginalize", dev["marg"], wall["marg"])
    line("lh_covariance, poses", dev["cov"], wall["cov"])
    print(f"  {'lh_solve_resident (array-free)':<34} time_ms median {np.median(solve_ms):8.4f} (min {min(solve_ms):.4f}, "
          f"max {max(solve_ms):.4f})")
    s.close()
