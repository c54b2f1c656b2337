"""Bitwise comparison of two builds of the library (LH_LIB) on the windows whose trajectories are most sensitive
to rounding: the headline C3 window, the live configuration, the gate-1 survey window, a 128-keyframe banded window
and the eval-first windows; then small windows that take every path of the large-window controllers' decision
(ctrl_take_decision): runs of rejections on k_ctrl_b (k_reduce decides; under LH_FORCE_RCCL=1 workgroup 0 does and
the rungs wait for it), k_ctrl_g and k_ctrl_p, and k_ctrl_g accepting.  Each build runs in its own process; the
parent compares every output array, the LM counts and the trace.  LH_NO_BATCH=1 in both, so that a change of the
batch path alone does not show; --batch leaves it unset, so the batches' decisions are compared too.
usage: python3 scripts/lib_bitwise.py [--batch] OTHER_LIB [THIS_LIB]"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if len(sys.argv) > 2 and sys.argv[1] == "--child":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "lego-slam_amd", "python")]
    import numpy as np
    import lego_ba
    from windows import RELIN_WINDOWS, STABLE, relin_window, stable_window, window
    out = {}

    def banded(P):
        w = lego_ba.generate_window(P=P, L=50000, k=8, seed=3, **dict(STABLE, outlier_frac=0.0))
        f = np.zeros(P, np.uint8)
        f[0] = 1
        w["pose_fixed"] = f
        return w

    cases = [("headline", window("C3", seed=0, family="stable_noout"), {}),
             ("live", window("C3", seed=0, family="default"), {}),
             ("survey gate 1", window("C3", seed=5, family="default"), dict(gate_mode=1)),
             ("P128", banded(128), {}),
             ("C2", window("C2", seed=0), {}),
             ("C2 fp32", window("C2", seed=0), dict(precision=lego_ba.LH_PREC_FP32_RESID))]
    # the large-window controllers' decision paths: (name, window, options, controller expected, env set at creation)
    relin = [("relin " + name, relin_window(gen), dict(opt, max_iters=3), ctl, None)
             for name, gen, opt, _, ctl in RELIN_WINDOWS if ctl != "k_ctrl"]
    dense = dict(pose_mode=1, k_min=2, k_max=8)
    cases = [c + (None, None) for c in cases] + relin + [
        ("relin k_ctrl_b self-deciding",) + relin[0][1:4] + ("LH_FORCE_RCCL",),
        ("k_ctrl_b accepting", stable_window(32, 4000, 1), {}, "k_ctrl_b", None),
        ("k_ctrl_g accepting", stable_window(32, 4000, 1, **dense), {}, "k_ctrl_g", None)]
    for name, w, kw, ctl, env in cases:
        if env:
            os.environ[env] = "1"
        s = lego_ba.Solver(**kw)
        r = s.solve(w)
        if env:
            del os.environ[env]
        assert ctl in (None, s.controller()), (name, s.controller())
        out[f"{name}/controller"] = np.array(s.controller())
        s.close()
        for k in ("pose_Tcw", "lm_xyz", "edge_robust_chi2", "trace_chi2", "trace_lambda"):
            out[f"{name}/{k}"] = r[k]
        out[f"{name}/scalars"] = np.array([r[k] for k in ("iterations", "trials", "accepted", "pcg_iterations",
                                                          "chi2_final", "lambda_final")])
    np.savez(sys.argv[2], **out)
    sys.exit(0)

import numpy as np  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--batch"]
res = []
with tempfile.TemporaryDirectory() as d:
    for lib in (args[1] if len(args) > 1 else None, args[0]):
        env = dict(os.environ)
        if "--batch" in sys.argv[1:]:
            env.pop("LH_NO_BATCH", None)
        else:
            env["LH_NO_BATCH"] = "1"
        if lib:
            env["LH_LIB"] = lib
        f = os.path.join(d, f"{len(res)}.npz")
        subprocess.run([sys.executable, __file__, "--child", f], env=env, check=True)
        res.append(dict(np.load(f)))
a, b = res
diff = {k: bool(np.array_equal(a[k], b[k])) for k in a}
print(json.dumps({"all_equal": all(diff.values()), "compared": len(diff),
                  "controllers": {k.rsplit("/", 1)[0]: str(a[k]) for k in a if k.endswith("controller")},
                  "scalars": {k: [a[k].tolist(), b[k].tolist()] for k in a if k.endswith("scalars")},
                  "differ": [k for k, v in diff.items() if not v]}))
