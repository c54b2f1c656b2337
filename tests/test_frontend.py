"""Frontend pose-only LM: Frontend::EstimateCurrentPose
(src/frontend_lego.cpp:157-250) batched over frames, lh_estimate_pose.

The oracle (oracle/lego_oracle.c orc_estimate_pose) restates the reference
loop: four rounds of problem.solve(10) from the frame's pose on one VertexPose
with EdgeProjectionPoseOnly edges (lego_types.h:116-180), outlier flags after
each round, no robust cost on round four.  Parity is unpinned by reference
output (the reference cannot be built).

Tolerances: the per-edge residual is a bitwise mirror of the oracle; sums over a
frame's edges are in a different (fixed) order, so states agree to rounding.
The pose problem has no gauge freedom (6 DoF, >= 3 points): the final pose is
compared at 1e-8, flags exactly except edges within 1e-6 of the 5.991 threshold,
iteration counts on 90 % of frames (the absolute stop rule, problem.cpp:210, sits
on rounding noise once a round has converged).

The hard inputs (everything below "hard inputs").  The tests above run tests/frames.py at its defaults: the
start pose is 0.01 rad and 0.05 m off, no trial is ever rejected, the first linearisation of every frame pivots
rotation rows first and every step is ~0.01 rad.  The families below reach the rest of k_frames:

  rej-*     start poses 0.3 rad / 2 m off: rejected trials, the lambda ladder (lam *= ni, ni *= 2; lam * 11),
            an iteration ended by max_trials, the rollback, flags computed from a rejected candidate's residuals
  piv-*     the scene scaled to 2-10 % (frames.scale_scene): depths of 0.16-6 m put the translation entries of
            H above the rotation ones, so Eigen's pivot sequence (frames.pivot_sequence) varies, starts on a
            translation row and includes the identity
  ang-*     start poses ~1 rad off with one trial per round: the step angle is the rotation between input and
            output pose, above 0.8 rad (the library's sincos) in some frames and 0.3-0.8 rad (the upper terms
            of the Taylor series) in many; ang-3pt: three-point frames, whose undamped step exceeds 2.5 rad,
            where the series itself would be wrong
  ragged-*  1-513 edges (rank-deficient frames, the wave and workgroup edges) on the rej inputs
  opt-*     max_trials = 1, max_iters = 0
  many      1024 frames in one call against calls of 64 and the oracle on a sample
  plus non-finite input, placement in the batch and partial output pointers.

Tolerance: the oracle's own pose moves when only the order of its per-edge sums changes, by 1e-16 on a
well-conditioned frame and by 1e-8 and more on a few hard ones, so one number does not fit every frame.
frames.reorder_envelope runs the oracle on eight edge permutations; spread_f is the largest pose difference it
sees on frame f, and a frame's pose is compared at

    bar_f = 16 x max(spread_f, median of spread over the batch)

on all 12 entries.  The kernel differs from the oracle by such a reorder plus FMA contraction, one-ulp
reciprocal pivots and a one-ulp sin/cos: rounding-sized perturbations of the same 6x6 solve, which the same
conditioning amplifies; the factor 16 covers those and the tail that eight samples miss.  The bar is a function
of the oracle alone.  A permutation cannot perturb a frame of one or two edges and has three outcomes on three, so
frames of fewer than four edges also take a one-ulp nudge of their inputs, and 56 nudged runs of their own
(frames.reorder_envelope; the argument and the figures are in DESIGN.md 2.4).  So that it cannot hide a failure, every case asserts, before the device is called, that
at most 1/8 of its frames have bar_f > 1e-8 (CPU test test_case_envelope_cap); on the frames below 1e-8 the
per-edge chi2, the flags (except edges within 1e-6 + their own chi2 spread of 5.991) and n_inliers are checked
as above.  Iteration counts are compared on the frames where every permutation agreed: exactly for
max_iters <= 3, on 90 % for full solves.  The coverage each family claims is asserted from the oracle and
numpy alone in the CPU tests test_coverage_*.
"""
import functools

import numpy as np
import pytest

import frames
import lego_ba
import oracle_bind as ob


def rot_err(a, b):
    Ra, Rb = a.reshape(3, 4)[:, :3], b.reshape(3, 4)[:, :3]
    return float(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


# ------------------------------------------------------------------ CPU: the oracle
def test_oracle_recovers_pose():
    fb = frames.batch(0, 8)
    o = ob.estimate_pose(fb)
    for f in range(8):
        assert rot_err(o["pose_Tcw"][f], fb["pose_true"][f]) < 5e-3
        t = o["pose_Tcw"][f].reshape(3, 4)[:, 3] - fb["pose_true"][f].reshape(3, 4)[:, 3]
        assert np.linalg.norm(t) < 0.2
    # most tracking outliers are flagged (the last round is plain least squares over every edge)
    assert o["is_outlier"][fb["gross"]].mean() > 0.8


def test_oracle_rounds_semantics():
    """Rounds one to three are identical solves (same start, same edges: the flags never remove an
    edge); round four drops the robust cost (frontend_lego.cpp:223-225).  With no outliers and a
    loose start every edge is an inlier, so the flags are all clear and the pose is the plain
    least-squares optimum."""
    fb = frames.batch(3, 4, outlier_frac=0.0)
    o = ob.estimate_pose(fb)
    assert not o["is_outlier"][o["rchi2"] <= 5.991].any()
    assert np.all(o["iterations"] >= 4)
    plain = ob.estimate_pose(fb, huber_delta=0.0)   # no robust cost in any round: same final round
    assert np.allclose(plain["pose_Tcw"], o["pose_Tcw"], atol=1e-9)


def test_oracle_empty_and_tiny_frames():
    fb = frames.batch(1, 3, n_obs=[0, 1, 4])
    o = ob.estimate_pose(fb)
    assert np.array_equal(o["pose_Tcw"][0], fb["pose_Tcw"][0])   # solve() returns false: pose kept
    assert o["iterations"][0] == 0
    assert np.all(np.isfinite(o["pose_Tcw"]))


# ------------------------------------------------------------------ GPU
def _compare(g, o, fb):
    assert np.allclose(g["pose_Tcw"], o["pose_Tcw"], atol=1e-8, rtol=0)
    # the absolute stop rule (last_chi - chi < 1e-5, problem.cpp:210) sits on rounding noise once a
    # round has converged: an extra iteration or two moves the pose by far less than the bar above
    assert np.mean(g["iterations"] == o["iterations"]) >= 0.9
    near = np.abs(o["rchi2"] - 5.991) < 1e-6
    assert np.array_equal(g["is_outlier"][~near], o["is_outlier"][~near])
    assert np.allclose(g["edge_chi2"], o["rchi2"], rtol=1e-7, atol=1e-9)
    ptr = fb["obs_ptr"]
    for f in range(int(fb["n_frames"])):
        assert g["n_inliers"][f] == (ptr[f + 1] - ptr[f]) - int(g["is_outlier"][ptr[f]:ptr[f + 1]].sum())


@pytest.mark.gpu
def test_gpu_estimate_pose_matches_oracle():
    fb = frames.batch(0, 64)
    g = lego_ba.Solver().estimate_pose(fb)
    o = ob.estimate_pose(fb)
    _compare(g, o, fb)


@pytest.mark.gpu
def test_gpu_estimate_pose_ragged_and_flags_in():
    """Ragged frames (0, 1, 3, 300, 1000 edges: more edges than threads per frame) and features
    already flagged on entry (recomputed at the final estimate before classification, :208-210)."""
    sizes = [0, 1, 3, 150, 300, 1000, 7, 64]
    fb = frames.batch(5, len(sizes), n_obs=sizes)
    rng = np.random.default_rng(1)
    fin = rng.random(int(fb["obs_ptr"][-1])) < 0.1
    g = lego_ba.Solver().estimate_pose(fb, is_outlier_in=fin)
    o = ob.estimate_pose(fb, is_outlier_in=fin)
    _compare(g, o, fb)
    assert np.array_equal(g["pose_Tcw"][0], fb["pose_Tcw"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [dict(strategy=1), dict(huber_delta=0.0), dict(lambda_init=1e-2)])
def test_gpu_estimate_pose_options(opt):
    fb = frames.batch(2, 16)
    g = lego_ba.Solver(**opt).estimate_pose(fb)
    o = ob.estimate_pose(fb, **opt)
    _compare(g, o, fb)


@pytest.mark.gpu
def test_gpu_estimate_pose_deterministic():
    fb = frames.batch(4, 32)
    s = lego_ba.Solver()
    a, b = s.estimate_pose(fb), s.estimate_pose(fb)
    assert np.array_equal(a["pose_Tcw"], b["pose_Tcw"]) and np.array_equal(a["edge_chi2"], b["edge_chi2"])


# ================================================================== hard inputs
HARD = dict(rot_sigma=0.3, trans_sigma=2.0)
RAGGED = [1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 255, 256, 257, 511, 512, 513]
SHORT = dict(lambda_init=1e-12)                     # a lambda far too small: the first steps overshoot
MANY_SAMPLE = list(range(5, 1024, 16))              # the frames of the 1024-frame batch the oracle sees


@functools.lru_cache(maxsize=None)
def _batch(kind):
    if kind == "hard":
        return frames.batch(7, 32, **HARD)
    if kind == "mild":
        return frames.batch(7, 32)
    if kind == "hard-small":
        return frames.scale_scene(_batch("hard"), 0.02)
    if kind.startswith("scaled-"):
        return frames.scale_scene(frames.batch(9, 32, rot_sigma=0.05, trans_sigma=0.5), float(kind[7:]))
    if kind == "angles":
        return frames.batch(3, 64, rot_sigma=1.0, trans_sigma=1.0)
    if kind == "angles-3pt":
        return frames.batch(5, 64, n_obs=3, rot_sigma=1.0, trans_sigma=1.0)
    if kind == "ragged":
        return frames.batch(7, len(RAGGED), n_obs=RAGGED, **HARD)
    if kind == "many":
        return frames.batch(11, 1024, n_obs=20)
    if kind == "many-sample":
        return frames.take(_batch("many"), MANY_SAMPLE)
    raise KeyError(kind)


# case -> (batch, options); the options go to the oracle and to lego_ba.Solver alike
CASES = {
    "rej-1x10": ("hard", dict(max_iters=1, max_trials=10, **SHORT)),
    "rej-2x3": ("hard", dict(max_iters=2, max_trials=3, **SHORT)),
    "rej-2x4-plain": ("hard", dict(max_iters=2, max_trials=4, huber_delta=0.0, **SHORT)),
    "rej-1x10-s1": ("hard", dict(max_iters=1, max_trials=10, strategy=1)),
    "rej-3x10": ("hard", dict(max_iters=3, max_trials=10)),
    "rej-full": ("hard", dict()),
    "piv-0.02": ("scaled-0.02", dict()),
    "piv-0.05": ("scaled-0.05", dict()),
    "piv-0.1": ("scaled-0.1", dict()),
    "piv-0.02-s1": ("scaled-0.02", dict(strategy=1)),
    "piv-hard-2x4": ("hard-small", dict(max_iters=2, max_trials=4, **SHORT)),
    "piv-hard-full": ("hard-small", dict()),
    "ang-default": ("angles", dict(max_iters=1, max_trials=1)),
    "ang-plain": ("angles", dict(max_iters=1, max_trials=1, huber_delta=0.0, **SHORT)),
    "ang-3pt": ("angles-3pt", dict(max_iters=1, max_trials=1, huber_delta=0.0, **SHORT)),
    "ragged-full": ("ragged", dict()),
    "ragged-2x4": ("ragged", dict(max_iters=2, max_trials=4, **SHORT)),
    "opt-trials1": ("hard", dict(max_trials=1)),
    "opt-iters0": ("mild", dict(max_iters=0)),
    "many": ("many-sample", dict()),
}
REJ_SHORT = ["rej-1x10", "rej-2x3", "rej-2x4-plain", "rej-1x10-s1", "rej-3x10"]
PIV = ["piv-0.02", "piv-0.05", "piv-0.1", "piv-0.02-s1", "piv-hard-2x4", "piv-hard-full"]
ANG = ["ang-default", "ang-plain"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(batch, options, the oracle's reorder envelope): computed once, shared by the CPU and the GPU tests."""
    kind, opt = CASES[name]
    fb = _batch(kind)
    env = frames.reorder_envelope(fb, n_perm=8, **opt)
    for a in (env["spread"], env["iters_agree"], env["rchi2_spread"], *env["base"].values()):
        a.setflags(write=False)
    return fb, opt, env


def _floor(env):
    """max(spread_f, median spread): the envelope the bar is 16 x of."""
    sp = env["spread"]
    return np.maximum(sp, np.median(sp))


def _bars(env):
    return 16.0 * _floor(env)


def _step_angles(fb, o):
    return np.array([rot_err(o["pose_Tcw"][f], fb["pose_Tcw"][f]) for f in range(int(fb["n_frames"]))])


def _rejecting(o):
    return o["trials"] > o["iterations"]


def _rejects_max_trials_in_a_row(fb, opt):
    """Frames in which some round rejects max_trials candidates in a row, for max_iters = 1: a round is then one
    iteration of min(k + 1, max_trials) trials, k the rejections before the first accepted step, and rounds
    do not depend on each other (each restarts from the input pose; the flags remove no edge).  So one more
    allowed trial adds a trial exactly where all max_trials were rejected."""
    assert opt["max_iters"] == 1
    more = dict(opt, max_trials=opt["max_trials"] + 1)
    return ob.estimate_pose(fb, **more)["trials"] > ob.estimate_pose(fb, **opt)["trials"]


def _pivot_rule(opt):
    return "strategy1" if opt.get("strategy", 0) == 1 else opt.get("lambda_init")


def _pivot_sequences(name):
    fb, opt, _ = _case(name)
    return [frames.pivot_sequence(fb, f, _pivot_rule(opt), huber_delta=opt.get("huber_delta", 5.991))
            for f in range(int(fb["n_frames"]))]


# ------------------------------------------------------------------ CPU: the helpers
def test_frames_helpers():
    fb = frames.batch(5, 4, n_obs=[3, 0, 40, 7])
    fp, perm = frames.permute_edges(fb, 1)
    ptr = fb["obs_ptr"]
    for f in range(4):
        assert sorted(perm[ptr[f]:ptr[f + 1]]) == list(range(ptr[f], ptr[f + 1]))   # edges stay in their frame
    assert not np.array_equal(perm, np.arange(50)) and np.array_equal(fp["pts"], fb["pts"][perm])
    assert np.array_equal(fp["obs_uv"], fb["obs_uv"][perm]) and np.array_equal(fp["pose_Tcw"], fb["pose_Tcw"])
    # the same problem: the oracle agrees to rounding, per edge after undoing the permutation
    a, b = ob.estimate_pose(fb), ob.estimate_pose(fp)
    assert np.allclose(a["pose_Tcw"], b["pose_Tcw"], atol=1e-9, rtol=0)
    back = np.zeros(50)
    back[perm] = b["rchi2"]
    assert np.allclose(back, a["rchi2"], rtol=1e-7, atol=1e-9)
    # scale_scene: the projections at the start pose and at the truth are unchanged
    fs = frames.scale_scene(fb, 0.02)
    for key in ("pose_Tcw", "pose_true"):
        for f in (0, 2, 3):
            T, Ts = fb[key][f].reshape(3, 4), fs[key][f].reshape(3, 4)
            Pc = fb["pts"][ptr[f]:ptr[f + 1]] @ T[:, :3].T + T[:, 3]
            Ps = fs["pts"][ptr[f]:ptr[f + 1]] @ Ts[:, :3].T + Ts[:, 3]
            assert np.allclose(Ps, 0.02 * Pc, rtol=1e-12, atol=1e-13)
    assert np.array_equal(fs["obs_uv"], fb["obs_uv"]) and np.array_equal(fs["obs_ptr"], fb["obs_ptr"])
    # take / concat: frames are cut and joined whole
    t = frames.take(fb, [2, 0])
    assert list(t["obs_ptr"]) == [0, 40, 43] and np.array_equal(t["pts"][:40], fb["pts"][ptr[2]:ptr[3]])
    c = frames.concat(frames.take(fb, [0, 1]), frames.take(fb, [2, 3]))
    for k in ("obs_ptr", "pts", "obs_uv", "pose_Tcw", "gross"):
        assert np.array_equal(c[k], fb[k])


def test_pivot_sequence_restates_eigen():
    """frames.pivot_sequence against the definition: applying its transpositions to the damped diagonal sorts
    it the way Eigen's search does (each step takes the first largest of the rest)."""
    fb = _batch("scaled-0.05")
    for f in range(8):
        h = frames._hessian_diag(fb, f, 5.991)
        key = np.abs(h + 1e-5 * min(5e10, np.abs(h).max()))
        tr = frames.pivot_sequence(fb, f)
        assert all(tr[k] >= k for k in range(6))
        for k, i in enumerate(tr):
            assert key[i] == key[k:].max() and (i == k or key[i] > key[k])
            key[[k, i]] = key[[i, k]]
        assert np.all(np.diff(key) <= 0)


# ------------------------------------------------------------------ CPU: what the default inputs miss
def test_default_batch_is_narrow():
    """Why the hard inputs exist: on the batch of test_gpu_estimate_pose_matches_oracle no trial is rejected,
    no step exceeds 0.05 rad and every frame's first pivot sequence is (4, 3, 5, .): rotation rows first, then
    the two nearly tied translation rows 0 and 1 in either order (one sequence without the Huber weights).
    Fails if tests/frames.py drifts."""
    fb = frames.batch(0, 64)
    o = ob.estimate_pose(fb)
    assert np.array_equal(o["trials"], o["iterations"])
    seqs = {frames.pivot_sequence(fb, f) for f in range(64)}
    plain = {frames.pivot_sequence(fb, f, huber_delta=0.0) for f in range(64)}
    ang = _step_angles(fb, o)
    print(f"default batch: rejected trials {int((o['trials'] - o['iterations']).sum())}, sequences {sorted(seqs)}, "
          f"without Huber {sorted(plain)}, largest rotation input to output {ang.max():.3f} rad")
    assert seqs <= {(4, 3, 5, 3, 4, 5), (4, 3, 5, 4, 4, 5)} and plain == {(4, 3, 5, 4, 4, 5)}
    assert ang.max() < 0.05


# ------------------------------------------------------------------ CPU: the cap and the coverage of every case
@pytest.mark.parametrize("name", list(CASES))
def test_case_envelope_cap(name):
    """At most 1/8 of a case's frames may sit above the project's 1e-8 bar: the envelope cannot excuse a batch."""
    fb, opt, env = _case(name)
    sp, bar = env["spread"], _bars(env)
    F = int(fb["n_frames"])
    o = env["base"]
    print(f"{name}: {F} frames, spread median {np.median(sp):.2e} max {sp.max():.2e}, bar > 1e-8 on "
          f"{int((bar > 1e-8).sum())}, iterations agree on {int(env['iters_agree'].sum())}, frames that reject "
          f"{int(_rejecting(o).sum())}, most trials {int(o['trials'].max())}")
    assert (bar > 1e-8).sum() <= F // 8
    assert np.all(np.isfinite(o["pose_Tcw"]))


def test_coverage_rejections():
    union = np.zeros(32, bool)
    for name in REJ_SHORT + ["rej-full", "piv-hard-2x4", "piv-hard-full"]:
        fb, opt, env = _case(name)
        rej = _rejecting(env["base"])
        union |= rej[:32]
        print(f"{name}: frames that reject {np.nonzero(rej)[0].tolist()}, rejected trials "
              f"{(env['base']['trials'] - env['base']['iterations'])[rej].tolist()}")
        # at full scale three or four frames overshoot (two without the Huber weights), scaled to 2 % two to four
        assert rej.sum() >= (3 if name.startswith("rej-") and opt.get("huber_delta", 5.991) > 0.0 else 2)
        # the comparison of these frames is a tight one, not one the envelope excuses
        assert (rej & (_bars(env) <= 1e-8)).sum() >= 2
    assert union.sum() >= 3
    fb, opt, env = _case("rej-1x10")
    full = _rejects_max_trials_in_a_row(fb, opt)
    print(f"rej-1x10: frames with max_trials rejections in a row {np.nonzero(full)[0].tolist()}")
    assert full.sum() >= 1 and (full & (_bars(env) <= 1e-8)).any()
    for name in ("ragged-full", "ragged-2x4"):
        assert _rejecting(_case(name)[2]["base"]).sum() >= 2
    assert not _rejecting(_case("opt-trials1")[2]["base"]).any()   # max_trials = 1: a rejection ends the iteration


def test_coverage_pivot_sequences():
    seqs = set()
    for name in PIV:
        q = _pivot_sequences(name)
        print(f"{name}: {len(set(q))} sequences {sorted(set(q))}")
        seqs |= set(q)
    assert len(seqs) >= 8
    assert any(s[0] <= 2 for s in seqs)                     # a translation row first
    assert (0, 1, 2, 3, 4, 5) in seqs                       # no swap at all
    assert all(s[0] <= 2 for s in _pivot_sequences("piv-0.02"))
    assert all(s[0] >= 3 for s in _pivot_sequences("piv-0.1"))


def test_coverage_step_angles():
    for name in ANG:
        fb, opt, env = _case(name)
        ang = _step_angles(fb, env["base"])
        tight = _bars(env) <= 1e-8
        big, mid = tight & (ang > 0.8), tight & (ang > 0.3) & (ang <= 0.8)
        print(f"{name}: steps above 0.8 rad on tight frames {ang[big].round(3).tolist()}, 0.3-0.8 rad on {int(mid.sum())}")
        assert big.sum() >= 2 and mid.sum() >= 8
    # a damped step on 150 edges stays below ~1.3 rad, where the Taylor series to x^17 is still good to 1e-15: it
    # takes steps of 2.5 rad and more (remainder x^19 / 19! > 3e-10) to tell the library branch from the series.
    # Three-point frames (the minimal full-rank problem) take such steps from a start ~1 rad off.
    fb, opt, env = _case("ang-3pt")
    ang = _step_angles(fb, env["base"])
    gap = ang ** 19 / 1.21645100408832e17                    # the first term the series leaves out, x^19 / 19!
    far = (ang > 2.0) & (gap > 2 * _bars(env))
    print(f"ang-3pt: rotations {ang[far].round(3).tolist()} rad whose series remainder {gap[far].tolist()} is above "
          f"twice the frame's bar {_bars(env)[far].tolist()}")
    assert far.sum() >= 1


# ------------------------------------------------------------------ GPU: against the envelope
def _ratio(diff, floor):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(diff == 0.0, 0.0, diff / floor)


def _compare_env(g, env, fb, opt, name):
    o = env["base"]
    F, ptr = int(fb["n_frames"]), np.asarray(fb["obs_ptr"], np.int64)
    bar = _bars(env)
    diff = np.abs(g["pose_Tcw"] - o["pose_Tcw"]).reshape(F, -1).max(axis=1)
    ratio = _ratio(diff, _floor(env))
    print(f"envelope {name}: |gpu - oracle| / max(spread_f, median) max {ratio.max():.3g} p90 "
          f"{np.percentile(ratio, 90):.3g} (largest pose difference {diff.max():.2e}, median spread "
          f"{np.median(env['spread']):.2e})")
    assert np.all(diff <= bar), (name, np.nonzero(diff > bar)[0].tolist(), diff[diff > bar], bar[diff > bar])
    tight = bar <= 1e-8
    edge_tight = np.repeat(tight, np.diff(ptr))
    assert np.allclose(g["edge_chi2"][edge_tight], o["rchi2"][edge_tight], rtol=1e-7, atol=1e-9)
    near = np.abs(o["rchi2"] - 5.991) < 1e-6 + env["rchi2_spread"]
    sel = edge_tight & ~near
    assert np.array_equal(g["is_outlier"][sel], o["is_outlier"][sel])
    for f in range(F):
        assert g["n_inliers"][f] == (ptr[f + 1] - ptr[f]) - int(g["is_outlier"][ptr[f]:ptr[f + 1]].sum())
    agree = np.nonzero(env["iters_agree"])[0]
    miss = agree[g["iterations"][agree] != o["iterations"][agree]]
    print(f"iterations {name}: compared on {len(agree)} frames, different on {miss.tolist()} "
          f"(gpu {g['iterations'][miss].tolist()}, oracle {o['iterations'][miss].tolist()})")
    if opt.get("max_iters", 10) <= 3:
        assert len(miss) == 0
    else:
        assert len(miss) <= 0.1 * len(agree)


def _run_case(name):
    fb, opt, env = _case(name)
    assert (_bars(env) > 1e-8).sum() <= int(fb["n_frames"]) // 8   # on the oracle alone, before the device runs
    s = lego_ba.Solver(**opt)
    g = s.estimate_pose(fb)
    s.close()
    _compare_env(g, env, fb, opt, name)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("name", REJ_SHORT)
def test_gpu_rejected_trials_short_horizon(name):
    """One to three iterations from a start 0.3 rad / 2 m off: rejected trials with nothing after them to pull
    the result back, so the bars are ~1e-10: the solve, the lambda ladder and the rollback, compared tightly."""
    _run_case(name)


@pytest.mark.gpu
def test_gpu_rejected_trials_full_solve():
    _run_case("rej-full")


@pytest.mark.gpu
@pytest.mark.parametrize("name", PIV)
def test_gpu_pivot_orders(name):
    _run_case(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ANG + ["ang-3pt"])
def test_gpu_large_step_angles(name):
    _run_case(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged-full", "ragged-2x4"])
def test_gpu_ragged_hard_frames(name):
    """1 and 2 edges: a rank-deficient H (the zero-pivot and tiny-pivot paths of the solve)."""
    _run_case(name)


@pytest.mark.gpu
def test_gpu_max_trials_one():
    _run_case("opt-trials1")


@pytest.mark.gpu
def test_gpu_max_iters_zero():
    """No step at all: the pose comes back as it went in, the flags are those of the start pose's residuals
    (0.01 rad and 0.05 m off: some edges above the threshold, some below)."""
    fb, opt, env = _case("opt-iters0")
    o = env["base"]
    assert np.all(o["iterations"] == 0) and min(o["is_outlier"].sum(), (~o["is_outlier"]).sum()) >= 100
    g = _run_case("opt-iters0")
    assert np.array_equal(g["pose_Tcw"], fb["pose_Tcw"]) and np.all(g["iterations"] == 0)


# ------------------------------------------------------------------ GPU: non-finite input
@pytest.mark.gpu
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_gpu_nonfinite_point(bad):
    """One non-finite map point: every step of that frame is rejected (the cost is not finite), its pose comes
    back untouched after max_iters x max_trials trials per round, and no other frame notices."""
    clean = frames.batch(0, 4)
    fb = dict(clean, pts=clean["pts"].copy())
    fb["pts"][150 + 17, 1] = bad
    o = ob.estimate_pose(fb)
    assert o["iterations"][1] == 40 and o["trials"][1] == 400 and np.array_equal(o["pose_Tcw"][1], fb["pose_Tcw"][1])
    s = lego_ba.Solver()
    g, gc = s.estimate_pose(fb), s.estimate_pose(clean)
    s.close()
    assert np.array_equal(g["pose_Tcw"][1], fb["pose_Tcw"][1])
    assert g["iterations"][1] == 40
    e = slice(150, 300)
    nan_o = np.isnan(o["rchi2"][e])
    assert nan_o.sum() >= 1 and np.array_equal(np.isnan(g["edge_chi2"][e]), nan_o)
    assert np.allclose(g["edge_chi2"][e][~nan_o], o["rchi2"][e][~nan_o], rtol=1e-7, atol=1e-9)
    near = np.abs(o["rchi2"][e] - 5.991) < 1e-6
    assert np.array_equal(g["is_outlier"][e][~near], o["is_outlier"][e][~near])
    assert g["n_inliers"][1] == 150 - int(g["is_outlier"][e].sum())
    others = np.r_[0:150, 300:600]
    for k in ("edge_chi2", "is_outlier"):
        assert np.array_equal(g[k][others], gc[k][others])
    for k in ("pose_Tcw", "iterations", "n_inliers"):
        assert np.array_equal(g[k][[0, 2, 3]], gc[k][[0, 2, 3]])


# ------------------------------------------------------------------ GPU: placement in the batch
def _frame_of(g, fb, f):
    e = slice(int(fb["obs_ptr"][f]), int(fb["obs_ptr"][f + 1]))
    return [g["pose_Tcw"][f], g["iterations"][f], g["n_inliers"][f], g["edge_chi2"][e], g["is_outlier"][e]]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_gpu_frame_placement():
    """A frame's outputs do not depend on where its edges start: alone, after a 1-edge frame and after a 7-edge
    frame (its points then start 24 and 168 bytes into the arena's segment).  The frame is one that rejects."""
    hard = _batch("hard")
    f = int(np.nonzero(_rejecting(_case("rej-full")[2]["base"]))[0][0])
    one = frames.take(hard, [f])
    s = lego_ba.Solver()
    alone = _frame_of(s.estimate_pose(one), one, 0)
    for n in (1, 7):
        fb = frames.concat(frames.batch(3, 1, n_obs=n), one)
        assert int(fb["obs_ptr"][1]) == n
        assert _same(_frame_of(s.estimate_pose(fb), fb, 1), alone)
    s.close()


@pytest.mark.gpu
def test_gpu_more_frames_than_resident_workgroups():
    """1024 frames in one launch (more workgroups than the device holds at once) against the same frames in
    calls of 64, bitwise, and against the oracle on every 16th frame."""
    big = _batch("many")
    s = lego_ba.Solver()
    g = s.estimate_pose(big)
    for c in range(0, 1024, 64):
        idx = list(range(c, c + 64))
        part = frames.take(big, idx)
        gp = s.estimate_pose(part)
        for j, f in enumerate(idx):
            assert _same(_frame_of(gp, part, j), _frame_of(g, big, f)), f
    s.close()
    fb, opt, env = _case("many")
    rows = np.concatenate([np.arange(big["obs_ptr"][f], big["obs_ptr"][f + 1]) for f in MANY_SAMPLE])
    sample = {k: g[k][MANY_SAMPLE] for k in ("pose_Tcw", "iterations", "n_inliers")}
    sample.update({k: g[k][rows] for k in ("edge_chi2", "is_outlier")})
    _compare_env(sample, env, fb, opt, "many")


# ------------------------------------------------------------------ GPU: partial outputs through the C ABI
def _raw_estimate(s, fb, want):
    """lh_estimate_pose with only the output pointers in `want` set (pose_Tcw always)."""
    C = lego_ba.C
    F, O = int(fb["n_frames"]), int(fb["obs_ptr"][-1])
    keep = [np.ascontiguousarray(fb["obs_ptr"], np.int64), np.ascontiguousarray(fb["pose_Tcw"], np.float64),
            np.ascontiguousarray(fb["pts"], np.float64), np.ascontiguousarray(fb["obs_uv"], np.float64)]
    a = lego_ba.LhFrames()
    a.n_frames = F
    a.obs_ptr, a.pose_Tcw, a.pts_w, a.obs_uv = (x.ctypes.data for x in keep)
    a.is_outlier = None
    for i in range(4):
        a.K[i] = float(fb["K"][i])
    out = dict(pose_Tcw=np.full((F, 12), -7.0), edge_chi2=np.full(O, -7.0), iterations=np.full(F, -7, np.int32),
               n_inliers=np.full(F, -7, np.int32), is_outlier=np.full(O, 7, np.uint8))
    r = lego_ba.LhFramesResult()
    r.pose_Tcw = out["pose_Tcw"].ctypes.data
    for k in ("edge_chi2", "iterations", "n_inliers", "is_outlier"):
        setattr(r, k, out[k].ctypes.data if k in want else None)
    assert lego_ba.ba_lib().lh_estimate_pose(s.h, C.byref(a), C.byref(r)) == 0
    return out


@pytest.mark.gpu
def test_gpu_partial_outputs():
    """Every subset of the optional outputs: what is asked for is bitwise the all-outputs call's, what is not
    is left alone.  The batch has an empty frame and one edge in another."""
    names = ("edge_chi2", "iterations", "n_inliers", "is_outlier")
    fb = frames.batch(6, 5, n_obs=[5, 0, 150, 1, 40], **HARD)
    s = lego_ba.Solver()
    full = _raw_estimate(s, fb, names)
    assert np.all(full["edge_chi2"] >= 0) and np.all(full["iterations"] >= 0) and np.all(full["is_outlier"] <= 1)
    ref = s.estimate_pose(fb)
    assert np.array_equal(ref["pose_Tcw"], full["pose_Tcw"]) and np.array_equal(ref["edge_chi2"], full["edge_chi2"])
    for m in range(16):
        want = [k for i, k in enumerate(names) if m >> i & 1]
        out = _raw_estimate(s, fb, want)
        assert np.array_equal(out["pose_Tcw"], full["pose_Tcw"]), want
        for k in names:
            if k in want:
                assert np.array_equal(out[k], full[k]), (want, k)
            else:
                assert np.all(out[k] == (7 if k == "is_outlier" else -7)), (want, k)
    s.close()
