"""Times of lh_covariance on the MI355X, after a solve on the same handle, in three shapes: the
poses' diagonal blocks alone, with the full Sigma_pp, and with the landmarks' Sigma_l.  Two windows:
  C3         20 keyframes, 50 k landmarks, 400 k observations, pose 0 fixed (the bench workload);
  reference  15 keyframes (map.h:82), 2 000 landmarks, no fixed pose, anchor = 0 (the oldest keyframe), as
             Backend::Optimize would call it.
time_ms is the call's HIP-event bracket (snapshot, linearisation, factor, inverse, landmark kernel; the download
excluded); wall is the host clock around Solver.covariance, the Python binding and the download included.  The shapes
are alternated call by call in one process after a warm-up; median and range of `reps` calls.  For scale: the
solve's own time_ms on the same handle (lh_solve_resident, array-free), and the time NumPy takes on the host for the
double evaluation of Sigma_pp alone (np.linalg.inv of S[f, f]; no linearisation).

usage: python3 scripts/cov_time.py [reps] > profiles/cov_time.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "lego-slam_amd", "python")]
import numpy as np     # noqa: E402
import lego_ba         # noqa: E402
import windows         # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
SHAPES = (("poses", dict()), ("poses + full", dict(full=True)), ("poses + landmarks", dict(landmarks=True)))


def line(name, dev, wall):
    print(f"  {name:<34} time_ms median {np.median(dev):8.4f} (min {min(dev):.4f}, max {max(dev):.4f})   "
          f"wall ms median {np.median(wall):8.3f} (min {min(wall):.3f}, max {max(wall):.3f})")


ref15 = lego_ba.generate_window(P=15, L=2000, k=8, seed=1, **windows.STABLE)   # (no pose_fixed: the live configuration)
# C3 runs with degenerate_guard = 1: the state its solve(10) returns has one landmark (of 50 000) whose H_ll is not
# positive definite; under guard 0 the solver rejects every later trial, as the reference does, and lh_covariance
# answers LH_E_SINGULAR, as defined.  With guard 1 that landmark is held fixed and its covariance is NaN.
for title, w, anchor, guard in (("C3: 20 keyframes, pose 0 fixed, degenerate_guard 1", windows.window("C3", seed=1, family="stable"), -1, 1),
                                ("reference-sized: 15 keyframes, no fixed pose, anchor 0", ref15, 0, 0)):
    s = lego_ba.Solver(degenerate_guard=guard)
    s.upload(w)
    solve_ms = []
    for rep in range(-3, reps):
        r = s.solve_resident()
        if rep >= 0:
            solve_ms.append(r["time_ms"])
    dev = {k: [] for k, _ in SHAPES}
    wall = {k: [] for k, _ in SHAPES}
    for rep in range(-3, reps):
        for k, kw in SHAPES:
            t0 = time.perf_counter()
            c = s.covariance(anchor=anchor, **kw)
            t1 = time.perf_counter()
            if rep >= 0:
                dev[k].append(c["time_ms"])
                wall[k].append((t1 - t0) * 1e3)
    # the host's double evaluation of Sigma_pp: np.linalg.inv of S[f, f], here recovered as the inverse of the
    # returned Sigma_pp[f, f] (the solver keeps S of a window this small in k_ctrl's LDS image, not in packed blocks)
    P = w["n_poses"]
    held = np.zeros(P, bool) if w.get("pose_fixed") is None else np.asarray(w["pose_fixed"]).astype(bool)
    if anchor >= 0:
        held[anchor] = True
    f = np.flatnonzero(np.repeat(~held, 6))
    S_ff = np.linalg.inv(s.covariance(anchor=anchor, full=True)["pose_cov_full"][np.ix_(f, f)])
    host = []
    for rep in range(-3, reps):
        t0 = time.perf_counter()
        np.linalg.inv(S_ff)
        if rep >= 0:
            host.append((time.perf_counter() - t0) * 1e3)
    print(f"{title}: {len(w['lm_xyz'])} landmarks, {len(w['obs_pose'])} observations, n_free {c['n_free']}, "
          f"pivots {c['min_pivot']:.3e} .. {c['max_pivot']:.3e}, {reps} calls")
    for k, _ in SHAPES:
        line("lh_covariance, " + k, dev[k], wall[k])
    print(f"  {'lh_solve_resident (array-free)':<34} time_ms median {np.median(solve_ms):8.4f} (min {min(solve_ms):.4f}, "
          f"max {max(solve_ms):.4f})")
    print(f"  {'NumPy inv of S[f, f] (host, double)':<34} wall ms median {np.median(host):8.4f} (min {min(host):.4f}, "
          f"max {max(host):.4f})")
    s.close()
