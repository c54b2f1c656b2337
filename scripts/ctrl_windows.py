"""The three large-window controllers under a kernel trace: a 128-keyframe banded window (k_ctrl_b), a 32-keyframe
dense one (k_ctrl_g) and the banded one again with PCG (k_ctrl_p), each solved resident N times (default 60) so
that its controller has some hundreds of launches.  Run it under gpu.sh's pytrace= step, with env=LH_LIB=... for
the library to compare against; the per-kernel averages are the step's summary.
usage: python3 scripts/ctrl_windows.py [N]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "lego-slam_amd", "python")]
import lego_ba      # noqa: E402
from windows import stable_window  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 60
band = stable_window(128, 50000, 3)
dense = stable_window(32, 4000, 1, pose_mode=1, k_min=2, k_max=8)
for ctl, w, kw in (("k_ctrl_b", band, {}), ("k_ctrl_g", dense, {}),
                   ("k_ctrl_p", band, dict(linear_solver=lego_ba.LH_SOLVER_PCG))):
    s = lego_ba.Solver(**kw)
    s.upload(w)
    for _ in range(N):
        r = s.solve_resident()
    assert s.controller() == ctl, s.controller()
    print(ctl, "solves", N, "iters", r["iterations"], "trials", r["trials"], "chi2 %.12e" % r["chi2_final"], flush=True)
    s.close()
