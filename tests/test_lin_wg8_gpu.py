"""k_lin's eight-wave workgroup shape (k_lin<T, TRIAL, F32, 8>, lego-slam_amd/csrc/lh_lin.hip) on small windows.

The planner gives the shape to windows that fill the GPU (tests/test_plan_wg8.py); here LH_TEST_LIN_WG8=1, read at
upload like the other switches, forces it onto small windows at chunk sizes that reach its paths, and the four-wave
shape of the same build (the default of these windows) is the comparison:

    case      sub-batches per chunk        what it is for
    few       3 (and a 1)                  waves without a sub-batch: barriers and combines with exact zeros
    nine      9                            one wave runs a second sub-batch
    full25    25 (and a 7)                 the C3 shape: waves 0 the long one, 7 6 6 6 per SIMD
    u6        9, six poses                 U < 8, lane groups of 4 and 8
    mono      9, one camera                one pose table per slot; poses 0 and 1 fixed (the scale gauge)
    fixedmid  9, poses 0 and 4 fixed       a fixed pose inside the chunk windows

Checked per case, eight waves against four:
  * rho0 per edge after the initial linearisation: bitwise equal (an edge's rho0 is a function of its pose, landmark
    and pixel alone).  After one accepted trial the two shapes stand at candidates that differ in the last bits (the
    step solves a reduced system whose sums are grouped by wave), so there rho0 is held bitwise to the oracle's
    evaluation at the state each run returned, and between the shapes wherever no chunk has more than 4 sub-batches
    (waves 4..7 then add exact zeros and the whole solve is the four-wave solve bit for bit).  Measured (MI355X):
    few 0 of 1600 edges differ between the shapes; nine 855 of 2304, full25 1534 of 3648, u6 484 of 978, mono 906 of
    2016, fixedmid 488 of 2304, each by at most 7.4e-13 on rho0 up to 22; every run 0 edges off the oracle at its
    own returned state.
  * the reduced system after the initial linearisation and after a trial, in both k_reduce layouts, against the
    long-double linearisation with tests/test_lin_system_gpu.py's helpers and tolerance;
  * two solves of one upload: bitwise equal summary, trace, poses, landmarks;
  * the full solve against the oracle at the stable families' bar (tests/test_gpu_parity.py);
and on a window that rejects (tests/windows.py RELIN_WINDOWS[0]: batches of evaluate-only rungs, an evaluate-only
acceptance, the re-linearisation chain) the eight-wave run takes the oracle's and the four-wave run's decisions."""
import numpy as np
import pytest

import lego_ba
import lin_ref
import oracle_bind as ob
import windows
from test_lin_system_gpu import check_system, huber, oracle_distance, read_system, set_layout

pytestmark = pytest.mark.gpu

KNOB = "LH_TEST_LIN_WG8"
LAYOUTS = ("packed", "image")
SUMMARY = ("iterations", "trials", "accepted", "chi2_initial", "chi2_final", "lambda_final")


def _gen(fixed=(0,), mono=False, **kw):
    kw = dict(dict(windows.STABLE, outlier_frac=0.0), **kw)
    if mono:
        kw["right_frac"] = 0.0
    w = lego_ba.generate_window(**kw)
    if mono:
        assert not w["obs_cam"].any()
        w["cam_ext"] = np.ascontiguousarray(w["cam_ext"][:1])
    f = np.zeros(w["n_poses"], np.uint8)
    f[list(fixed)] = 1
    w["pose_fixed"] = f
    return w


# id: (window, chunk_landmarks, the sub-batches per chunk and window poses per chunk the case claims)
CASES = {
    "few": (lambda: _gen(P=8, L=200, k=8, seed=11), 24, {1, 3}, {8}),
    "nine": (lambda: _gen(P=8, L=288, k=8, seed=12), 72, {9}, {8}),
    "full25": (lambda: _gen(P=8, L=456, k=8, seed=13), 200, {7, 25}, {8}),
    "u6": (lambda: _gen(P=6, L=216, k=3, k_max=6, pose_mode=1, seed=14), 72, None, None),
    "mono": (lambda: _gen(fixed=(0, 1), mono=True, P=7, L=288, k=7, seed=15), 72, {9}, {7}),
    "fixedmid": (lambda: _gen(fixed=(0, 4), P=8, L=288, k=8, seed=16), 72, {9}, {8}),
}
NAMES = list(CASES)
_win, _runs, _ref = {}, {}, {}


def case(name):
    if name not in _win:
        make, chunk, sbs, us = CASES[name]
        w = make()
        pl = lego_ba.plan_window(w, chunk)
        ch = pl["chunks"]
        nsb = set(int(x) for x in ch["sb_end"] - ch["sb_begin"])
        assert int(ch["T"].max()) <= 3, name
        if sbs is not None:
            assert nsb == sbs and set(int(u) for u in ch["U"]) == us, (name, nsb, set(ch["U"]))
        else:   # u6: random pose subsets
            assert max(nsb) >= 9 and int(ch["U"].max()) < 8 and len(set(int(x) for x in pl["sbs"]["lg"])) > 1, (name, nsb)
        _win[name] = (w, chunk, dict(gate_mode=1), max(nsb))
    return _win[name]


def run(name, waves, monkeypatch, layout="image", **kw):
    """One solve of the case in the given shape: (result, shape, staged system reader's inputs); cached."""
    key = (name, waves, layout, tuple(sorted(kw.items())))
    if key in _runs:
        return _runs[key]
    w, chunk, opts, _ = case(name)
    set_layout(monkeypatch, layout)
    if waves == 8:
        monkeypatch.setenv(KNOB, "1")
    else:
        monkeypatch.delenv(KNOB, raising=False)
    env = kw.pop("env", ())
    for v in env:
        monkeypatch.setenv(v, "1")
    s = lego_ba.Solver(chunk_landmarks=chunk, **dict(opts, **kw))
    try:
        g = s.solve(w)
        assert s.lin_shape()[0] == waves, (name, s.lin_shape())
        R = None
        if kw.get("max_iters", 10) == 0:
            R = reference0(name)[0]
        elif env:
            R = lin_ref.linearise(w, pose=g["pose_Tcw"], lm=g["lm_xyz"], huber_delta=huber(opts))
        got = read_system(s, w, chunk, layout, R) if R is not None else None
        s.upload(w)
        again = [s.solve_resident(want_states=True, want_edges=True) for _ in range(2)] if not kw else None
    finally:
        s.close()
        for v in env:
            monkeypatch.delenv(v)
    _runs[key] = (g, got, R, again)
    return _runs[key]


def reference0(name):
    if name not in _ref:
        w, _, opts, _ = case(name)
        R = lin_ref.linearise(w, huber_delta=huber(opts))
        _ref[name] = (R, oracle_distance(w, opts, R))
    return _ref[name]


TRIAL = dict(max_iters=1, max_trials=1, env=("LH_NO_EVO", "LH_NO_LADDER", "LH_NO_BATCH"))


@pytest.mark.parametrize("name", NAMES)
def test_rho0_per_edge(name, monkeypatch):
    w, _, opts, max_sb = case(name)
    a8 = run(name, 8, monkeypatch, max_iters=0)[0]
    a4 = run(name, 4, monkeypatch, max_iters=0)[0]
    assert np.array_equal(a8["edge_robust_chi2"], a4["edge_robust_chi2"]), "initial linearisation"
    assert np.array_equal(a8["edge_robust_chi2"], ob.solve(w, max_iters=0, **opts)["edge_robust_chi2"])
    t8 = run(name, 8, monkeypatch, **TRIAL)[0]
    t4 = run(name, 4, monkeypatch, **TRIAL)[0]
    assert t8["accepted"] == t4["accepted"] == 1
    d = np.abs(t8["edge_robust_chi2"] - t4["edge_robust_chi2"])
    print(f"RHO0 {name}: after one trial {np.count_nonzero(d)} of {len(d)} edges differ between the shapes, "
          f"max {d.max():.2e} (rho0 up to {t4['edge_robust_chi2'].max():.2e})")
    for tag, t in (("8", t8), ("4", t4)):   # rho0 as a function of the returned state alone
        o = ob.solve(dict(w, pose_Tcw=t["pose_Tcw"], lm_xyz=t["lm_xyz"]), max_iters=0, **opts)
        bad = np.count_nonzero(t["edge_robust_chi2"] != o["edge_robust_chi2"])
        print(f"RHO0 {name}: {tag} waves, {bad} edges differ from the oracle at the returned state")
        assert bad == 0, (name, tag, bad)
    if max_sb <= 4:
        assert not d.any()
        for k in ("pose_Tcw", "lm_xyz", "trace_chi2"):
            assert np.array_equal(t8[k], t4[k]), k
    else:
        assert np.allclose(t8["edge_robust_chi2"], t4["edge_robust_chi2"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", NAMES)
def test_initial_linearisation(name, layout, monkeypatch):
    g, got, R, _ = run(name, 8, monkeypatch, layout=layout, max_iters=0)
    assert g["degenerate"] == 0 and g["trials"] == 0
    check_system("A8/" + layout, name, got, R, reference0(name)[1])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", NAMES)
def test_trial_linearisation(name, layout, monkeypatch):
    w, _, opts, _ = case(name)
    g, got, R1, _ = run(name, 8, monkeypatch, layout=layout, **TRIAL)
    assert g["accepted"] == 1 and g["trials"] == 1
    orc = oracle_distance(dict(w, pose_Tcw=g["pose_Tcw"], lm_xyz=g["lm_xyz"]), opts, R1)
    check_system("B8/" + layout, name, got, R1, orc)


def rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("name", NAMES)
def test_full_solve_deterministic_and_against_the_oracle(name, monkeypatch):
    w, _, opts, _ = case(name)
    g, _, _, (b, c) = run(name, 8, monkeypatch)
    for k in SUMMARY:
        assert g[k] == b[k] == c[k], k
    for k in ("trace_chi2", "trace_lambda", "pose_Tcw", "lm_xyz", "edge_robust_chi2"):
        assert np.array_equal(g[k], b[k]) and np.array_equal(b[k], c[k]), k
    runs = [ob.solve(w, n_threads=t, **opts) for t in (1, 2, 8)]
    chis = [r["chi2_final"] for r in runs]
    assert (max(chis) - min(chis)) / min(chis) < 1e-12, "window not reproducible under reordering"
    o = runs[0]
    assert g["iterations"] in {r["iterations"] for r in runs}
    assert rel(g["chi2_final"], o["chi2_final"]) < 1e-6
    assert rel(g["trace_chi2"][1], o["trace_chi2"][1]) < 1e-9
    assert np.allclose(g["pose_Tcw"], o["pose_Tcw"], atol=1e-6)
    assert np.allclose(g["lm_xyz"], o["lm_xyz"], atol=1e-6)
    g4 = run(name, 4, monkeypatch)[0]
    assert (g["iterations"], g["trials"], g["accepted"]) == (g4["iterations"], g4["trials"], g4["accepted"])


def _relin(waves, batch, monkeypatch):
    _, gen, opt, dec, ctrl = windows.RELIN_WINDOWS[0]
    w = windows.relin_window(gen)
    if waves == 8:
        monkeypatch.setenv(KNOB, "1")
    else:
        monkeypatch.delenv(KNOB, raising=False)
    if not batch:
        monkeypatch.setenv("LH_NO_BATCH", "1")
    else:
        monkeypatch.delenv("LH_NO_BATCH", raising=False)
    s = lego_ba.Solver(max_iters=3, **opt)
    try:
        r = s.solve(w)
        r["shape"], r["controller"], r["chains"], r["batch"] = s.lin_shape(), s.controller(), s.chains(), s.batch()
    finally:
        s.close()
    return r, dec, ctrl


@pytest.mark.parametrize("batch", [False, True])
def test_rejecting_window_takes_the_same_decisions(batch, monkeypatch):
    """The batch path (batch), the evaluate-only trials and the re-linearisation chain of an evaluate-only acceptance
    (both): the oracle's decision string, and the four-wave run's trace to 1e-9."""
    r8, dec, ctrl = _relin(8, batch, monkeypatch)
    r4, _, _ = _relin(4, batch, monkeypatch)
    assert r8["shape"][0] == 8 and r4["shape"][0] == 4 and r8["shape"][1:] == r4["shape"][1:]
    assert r8["controller"] == ctrl
    assert (r8["iterations"], r8["trials"], r8["accepted"]) == (3, len(dec), dec.count("A"))
    for k in ("iterations", "trials", "accepted", "chains", "batch"):
        assert r8[k] == r4[k], k
    assert r8["chains"] > r8["trials"] or batch          # a re-linearisation chain ran
    assert (r8["batch"][1] > 0) == batch
    assert len(r8["trace_chi2"]) == len(r4["trace_chi2"])
    assert np.allclose(r8["trace_chi2"], r4["trace_chi2"], rtol=1e-9)
    assert np.allclose(r8["trace_lambda"], r4["trace_lambda"], rtol=1e-6)
    assert rel(r8["chi2_final"], r4["chi2_final"]) < 1e-9 and r8["chi2_final"] < r8["chi2_initial"]
