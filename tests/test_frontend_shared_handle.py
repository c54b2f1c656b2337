"""GPU test of what the frontend entry points share on one handle (lego-slam_amd/csrc/lh_frontend.cpp, lh_handle.h):
the event pool, the tracker's keypoints between lh_lk_track and lh_stereo_landmarks, the triangulation arenas between
lh_triangulate and lh_stereo_landmarks, buffers that grow from one call to the next, and the handle's destruction.

Every call is deterministic, so the reference of a call is the same call on a fresh handle, and every comparison is
by bits: each array and count a call returns, the times alone left out.  There is no tolerance in this file."""
import ast
import os

import numpy as np
import pytest

import frames
import images
import triangulate_ref as tr

pytestmark = pytest.mark.gpu

TIMES = ("time_ms", "time_prep_ms", "time_upload_ms", "time_download_ms")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c1_stable_noout_s0.npz")
FRONTEND = ("detect", "lk", "tri", "stereo", "pose")


def bits(v):
    a = np.asarray(v)
    return a.dtype.str, a.shape, a.tobytes()


def same(got, ref):
    assert got.keys() == ref.keys()
    for k in ref:
        if k not in TIMES:
            assert bits(got[k]) == bits(ref[k]), k


@pytest.fixture(scope="module")
def calls():
    """name -> (the call on a solver, its result on a fresh handle): computed once and left unchanged.
    Small shapes, then larger ones in which every buffer of the frontend grows."""
    import lego_ba
    z = np.load(GOLDEN)
    window = {k[3:]: z[k] for k in z.files if k.startswith("in_")}
    opt = dict(ast.literal_eval(str(z["opt_json"])))
    new = lambda: lego_ba.Solver(device=0, **opt)
    Ks = np.stack([tr.K, tr.K])
    out = {"new": new}

    def add(name, fn):
        s = new()
        out[name] = (fn, fn(s))
        s.close()
        return out[name][1]

    for tag, (rows, cols), n_tri, n_obs in (("", (64, 96), 65, 40), ("_big", (120, 160), 257, [90, 70, 80])):
        left, right = images.pair(rows, cols, shift=(-3.0, 0.0), seed=5)
        det = add("detect" + tag, lambda s, im=left: s.detect_features(im, max_corners=40, min_distance=5.0, want_eig=True))
        if tag:
            kp = images.keypoints(rows, cols, 62, seed=2)   # 70 with the ones on and past the frame's edges
            assert len(kp) == 70
        else:
            kp = det["kp"][:12].copy()
            assert len(kp) == 12
        add("lk" + tag, lambda s, a=left, b=right, k=kp: s.lk_track(a, b, k, levels=4))
        poses, px, _ = tr.stereo_family(n_tri, seed=3)
        add("tri" + tag, lambda s, p=poses, x=px: s.triangulate(p, x, K=Ks))
        add("stereo" + tag, lambda s, a=left, b=right, k=kp: s.stereo_landmarks(a, b, k, tr.stereo_poses(), K=Ks,
                                                                                 kp_right_init=k))
        fb = frames.batch(7, 1 if np.isscalar(n_obs) else len(n_obs), n_obs=n_obs)
        add("pose" + tag, lambda s, f=fb: s.estimate_pose(f))
    add("solve", lambda s: s.solve(window))
    out["bad"] = lambda s, a=left, b=right, k=kp: s.lk_track(a, b, k, levels=3)
    return out


def run(s, calls, name):
    fn, ref = calls[name]
    same(fn(s), ref)


def fails_badarg(s, calls):
    import lego_ba
    with pytest.raises(lego_ba.LhError) as e:
        calls["bad"](s)
    assert e.value.status == lego_ba.LH_E_BADARG


def test_fresh_results_are_not_trivial(calls):
    for tag in ("", "_big"):
        assert calls["lk" + tag][1]["success"].sum() > 0 and calls["stereo" + tag][1]["success"].sum() > 0
        assert calls["tri" + tag][1]["n_accepted"] > 0 and calls["pose" + tag][1]["n_inliers"].min() > 0
    assert calls["detect"][1]["n_corners"] >= 12 and calls["solve"][1]["iterations"] > 0


def test_shared_handle_sequence(calls):
    """Every entry point in turn on one handle, a solve in the middle, then the frontend again in reverse order at
    shapes that make every buffer grow, with a failing call between valid ones on both legs."""
    s = calls["new"]()
    run(s, calls, "detect")
    run(s, calls, "lk")
    fails_badarg(s, calls)        # returns before it enqueues anything, after the call has begun on the handle
    run(s, calls, "tri")
    run(s, calls, "stereo")
    run(s, calls, "pose")
    run(s, calls, "solve")
    for name in reversed(FRONTEND):
        run(s, calls, name + "_big")
        if name == "stereo":
            fails_badarg(s, calls)
    run(s, calls, "solve")        # and the solver's buffers are where the frontend left them
    run(s, calls, "stereo")       # small again, in the grown buffers
    s.close()


def test_create_use_close(calls):
    """Three handles in turn, each closed with every frontend buffer populated; a fourth still computes the same."""
    for _ in range(3):
        s = calls["new"]()
        for name in FRONTEND:
            run(s, calls, name)
        s.close()
    s = calls["new"]()
    run(s, calls, "detect")
    s.close()
