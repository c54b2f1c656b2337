"""The windows of the controller step tests (tests/test_step_ref_cpu.py, tests/test_ctrl_step_gpu.py): small windows,
each chosen for the controller path it reaches.  Every claim is asserted on the CPU from lego_ba.solve_config and the
oracle (tests/test_step_ref_cpu.py); the GPU test asserts the same controller and first decision on the device.

All windows: no robust kernel (huber_delta = 0), pose 0 fixed (the gauge), large initial errors
(windows._RELIN_NEAR / _RELIN_FAR), so that the first trial's decision is the same whatever the summation order.
Strategy-0 cases start at lambda_init = 1e-3; strategy 1 starts at its fixed 1e-5.

Every window's S + lambda D is positive definite at every lambda of its ladder (asserted on the oracle's S: the
Cholesky yardstick needs it).  With these perturbations a landmark can land next to a camera, its H_ll is then
ill-conditioned to 1e9 and beyond, and the computed S is indefinite by far more than lambda: such a window tests the
landmark inverse, not the controller, and the seeds and landmark counts below avoid them (lds_p21, g_p64 and b_p256
were moved off seeds whose S had eigenvalues of -419, -24 and -0.06).  The PCG cases are held to ob.pcg_solve's step
count, so their windows are ones where that count does not sit on a knife edge (test_step_ref_cpu.py: a stop
threshold 1.5 x higher or lower moves it by a few steps at the most).  A 96-pose window (seed 2) failed that: at its rung
4 the oracle's residual dips to 1.46e-6 ||b|| at step 534, rises again and passes 1e-6 at step 567, and the device,
whose dip reached 0.96e-6, stopped at 536 with a step 2e-3 away.  Hence 72 poses, seed 3.
"""
import numpy as np

import lego_ba
import windows

NEAR, FAR = windows._RELIN_NEAR, windows._RELIN_FAR
PCG = lego_ba.LH_SOLVER_PCG
S0 = dict(huber_delta=0.0, lambda_init=1e-3)
S1 = dict(huber_delta=0.0, strategy=1)


def _case(gen, pert, opts, ctrl, first, fixed=(0,), env=None, max_trials=10, rungs=None, **claim):
    """gen, pert: generate_window's arguments; opts: the solver's; ctrl: the controller the planner must choose;
    first: the first trial's decision ('A' / 'R'); env: LH_* switches set for the case; max_trials: the ladder's
    rungs; rungs: the rungs the GPU test checks (None: all); claim: further solve_config values."""
    return dict(gen=dict(gen, **pert), opts=opts, controller=ctrl, first=first, fixed=tuple(fixed), env=dict(env or {}),
                max_trials=max_trials, rungs=rungs, claim=claim)


_DENSE = dict(k=2, pose_mode=1)
_BAND_LDS = dict(P=20, L=400, k=8, seed=1)
_B_WIDE = dict(P=40, L=600, k=11, seed=2)
_P30 = dict(P=30, L=300, k=8, seed=1)
_P10 = dict(P=10, L=500, k=8, seed=3)

# id: what it reaches
#   lds_band   k_ctrl from the LDS image, a banded envelope (the host's envelope-limited unit table)
#   lds_dense  k_ctrl, a dense envelope
#   lds_p21    k_ctrl's largest window: 126 rows, two identity padding rows
#   lds_tiny   18 rows: most of the 128-row image is padding
#   lds_s1     k_ctrl, lambda diag(S)
#   g_p24      k_ctrl_g just past k_ctrl's envelope; g_p64 its largest window
#   b_p22      k_ctrl_b from the band image, one-row back substitution
#   b_p70      420 rows: NE = 432 differs from n; a fixed pose in the second fixed_bits word
#   b_wide     two-row back substitution (an envelope past 56 rows)
#   b_lu       the LU instantiation: the stream loaders take units
#   b_p256     BNMAX rows: the circular window wraps twelve times
#   b_s1       k_ctrl_b, lambda diag(S)
#   p_p30      k_ctrl_p on a dense pair list; p_p72 on the block-sparse one (past 64 poses)
#   lds_pcg    k_ctrl's LDS PCG (strategy 1)
#   lds_nd     the two-chain lds_ldlt_solve_nd (LH_ND=1) with ctrl_step_tail
#   lds_lad16  all LH_LAD rungs
#   b_wide_packed   k_ctrl_b's packed-block loaders (LH_NO_BIMG=1: the path of every sharded solve)
CASES = {
    "lds_band": _case(_BAND_LDS, FAR, S0, "k_ctrl", "R", img=1),
    "lds_dense": _case(dict(_DENSE, P=16, L=200, k_max=16, seed=1), NEAR, S0, "k_ctrl", "A"),
    "lds_p21": _case(dict(P=21, L=400, k=8, seed=1), NEAR, S0, "k_ctrl", "A"),
    "lds_tiny": _case(dict(_DENSE, P=3, L=30, k_max=3, seed=1), NEAR, S0, "k_ctrl", "A"),
    "lds_s1": _case(_P10, FAR, S1, "k_ctrl", "R"),
    "g_p24": _case(dict(_DENSE, P=24, L=400, k_max=8, seed=4), NEAR, S0, "k_ctrl_g", "R"),
    "g_p64": _case(dict(_DENSE, P=64, L=500, k_max=8, seed=3), NEAR, S0, "k_ctrl_g", "R"),
    "b_p22": _case(dict(P=22, L=300, k=8, seed=1), NEAR, S0, "k_ctrl_b", "A", band_narrow=True, bimg=1),
    "b_p70": _case(dict(P=70, L=600, k=2, k_max=8, seed=1), NEAR, S0, "k_ctrl_b", "A", fixed=(0, 66), band_narrow=True),
    "b_wide": _case(_B_WIDE, NEAR, S0, "k_ctrl_b", "A", band_narrow=False, bimg=1),
    "b_lu": _case(dict(_B_WIDE, k=15), NEAR, S0, "k_ctrl_b", "A", band_loader_units=True),
    "b_p256": _case(dict(P=256, L=3000, k=8, seed=4), NEAR, S0, "k_ctrl_b", "A", rungs=(0, 4, 9), band_narrow=True),
    "b_s1": _case(_P30, NEAR, S1, "k_ctrl_b", "R"),
    "p_p30": _case(_P30, NEAR, dict(S0, linear_solver=PCG), "k_ctrl_p", "R"),
    "p_p72": _case(dict(P=72, L=900, k=8, seed=3), NEAR, dict(S0, linear_solver=PCG), "k_ctrl_p", "A", sparse=True),
    "lds_pcg": _case(_P10, FAR, dict(S1, linear_solver=PCG), "k_ctrl", "R"),
    "lds_nd": _case(_BAND_LDS, FAR, S0, "k_ctrl", "R", env={"LH_ND": "1"}, nd=True, img=0),
    "lds_lad16": _case(_BAND_LDS, FAR, S0, "k_ctrl", "R", max_trials=16, ladder=16),
    "b_wide_packed": _case(_B_WIDE, NEAR, S0, "k_ctrl_b", "A", env={"LH_NO_BIMG": "1"}, band_narrow=False, bimg=0),
}
LDLT = [k for k, c in CASES.items() if c["opts"].get("linear_solver", 0) != PCG]
PCGS = [k for k, c in CASES.items() if c["opts"].get("linear_solver", 0) == PCG]

_cache = {}


def window(name):
    """The case's window, built once."""
    if name not in _cache:
        c = CASES[name]
        w = lego_ba.generate_window(**c["gen"])
        f = np.zeros(w["n_poses"], np.uint8)
        f[list(c["fixed"])] = 1
        w["pose_fixed"] = f
        _cache[name] = w
    return _cache[name]


def solver_opts(name):
    """The case's solver options (the reproducible Huber gate, as lin_cases: without a robust kernel it changes nothing)."""
    return dict(CASES[name]["opts"], gate_mode=1)


def oracle_opts(name):
    o = solver_opts(name)
    if "linear_solver" in o:
        o["linear_solver"] = 1 if o["linear_solver"] == PCG else 0
    return o


def set_env(monkeypatch, name):
    """The case's switches; the layout switches of other tests cleared."""
    for v in ("LH_NO_IMG", "LH_NO_BIMG", "LH_ND", "LH_NO_EVO", "LH_NO_LADDER", "LH_NO_BATCH", "LH_LADDER_LAZY"):
        monkeypatch.delenv(v, raising=False)
    for k, v in CASES[name]["env"].items():
        monkeypatch.setenv(k, v)


def config(name):
    """solve_config of the case (the environment already set: set_env)."""
    c = CASES[name]
    return lego_ba.solve_config(window(name), linear_solver=c["opts"].get("linear_solver", lego_ba.LH_SOLVER_LDLT),
                                max_trials=c["max_trials"])


def check_claims(name, cfg):
    """The case's planner claims against a solve_config dict; returns the mismatches."""
    c = CASES[name]
    bad = []
    if cfg["controller"] != c["controller"]:
        bad.append(("controller", cfg["controller"], c["controller"]))
    if cfg["ladder"] != c["max_trials"]:
        bad.append(("ladder", cfg["ladder"], c["max_trials"]))
    for k, v in c["claim"].items():
        if k == "sparse":
            P = window(name)["n_poses"]
            got = len(lego_ba.plan_window(window(name))["pair_pq"]) < P * (P + 1) // 2
        else:
            got = (cfg["nd_steps"] > 0) if k == "nd" else cfg[k]
        if got != v:
            bad.append((k, got, v))
    return bad
