"""GPU tests of lh_insert_keyframe (include/lego_ba.h): a keyframe's detector, right-image tracker and
triangulation in one call.

The reference of the fused call is the composition of the entry points the library already tests against their own
oracles, with the host in between (tests/keyframe_ref.py compose): Solver.detect_features -> track_ref.guess ->
Solver.klt_stereo_landmarks, then flag 32 and pt = 0 on the features with a point.  Every call is deterministic and every
fused-against-composed comparison is by bits, with no tolerance (a NaN kp_right, whose payload lh_klt_track's definition
leaves open, matches a NaN).  Each case first asserts on the composed result that it reaches what it is there for.  One
case also meets the NumPy chain (keyframe_ref.reference): the corners, kp_right, success and the flags exactly, pt within
the tolerance tests/golden/triangulation_tol.json records for the triangulation."""
import ast
import ctypes as C
import functools
import os

import numpy as np
import pytest

import frames
import images
import keyframe_ref as kf
import track_ref as tk
import triangulate_ref as tr

pytestmark = pytest.mark.gpu

ROWS, COLS = kf.ROWS, kf.COLS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c1_stable_noout_s0.npz")
NONE = dict(have_kp=None, have_pts_w=None, have_point=None)
TRACK_KEYS = ("kp2", "success", "pose_Tcw", "is_outlier", "edge_chi2", "n_tracked", "n_edges", "n_inliers", "iterations")


@pytest.fixture(scope="module")
def solver():
    import lego_ba
    s = lego_ba.Solver(device=0)
    yield s
    s.close()


def fresh():
    import lego_ba
    return lego_ba.Solver(device=0)


def same(g, r, keys=kf.KEYS):
    for k in keys:
        a, b = np.asarray(g[k]), np.asarray(r[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == "f":
            nan = np.isnan(b)
            assert np.array_equal(np.isnan(a), nan), k
            assert np.array_equal(tk.bits(a)[~nan], tk.bits(b)[~nan]), k
        else:
            assert np.array_equal(a, b), k


def fused(s, sc, **kw):
    return kf.call(s.insert_keyframe, sc, **kw)


def composed(s, sc, **kw):
    return kf.call(functools.partial(kf.compose, s), sc, **kw)


@functools.lru_cache(maxsize=None)
def hostile_scene():
    """The keyframe scene with three of its map points moved: zero depth in the right camera, the camera centre, far
    outside the image.  In the scene itself every feature with a point tracks."""
    sc = kf.scene()
    X = sc["have_pts_w"].copy()
    rows = np.flatnonzero(sc["have_point"])[:3]
    X[rows[0]] = (1.0, 2.0, 0.0)                    # (+inf, +inf)
    X[rows[1]] = (kf.BASELINE, 0.0, 0.0)            # the right camera's centre: (NaN, NaN)
    X[rows[2]] = (400.0, 3.0, 5.0)
    X.setflags(write=False)
    return dict(sc, have_pts_w=X), rows


@functools.lru_cache(maxsize=None)
def composed_scene(which):
    """The composition on a scene, on a handle of its own: computed once, shared, left unchanged."""
    s = fresh()
    r = composed(s, {"scene": kf.scene(), "hostile": hostile_scene()[0]}[which])
    s.close()
    return r


def images_after():
    """A: the frame before the keyframe; C: the frame after it (the scene's left image moved on)"""
    before = images.pair(ROWS, COLS, shift=(-1.8, 1.1), seed=11)[1]
    after = images.pair(ROWS, COLS, shift=(1.5, -0.8), seed=11)[1]
    return before, after


def track_inputs(r, sc):
    """lh_track_frame's inputs after a keyframe: every feature, with the points the keyframe has and has accepted"""
    have = np.zeros((0, 2), np.float32) if sc["have_kp"] is None else sc["have_kp"]
    nh = len(have)
    kp1 = np.concatenate([have, r["kp_new"]])
    X = r["pt"].copy()
    hp = (r["flags"] == 0).astype(np.uint8)
    if nh:
        old = sc["have_point"].astype(bool)
        X[:nh][old] = sc["have_pts_w"][old]
        hp[:nh][old] = 1
    return kp1, X, hp, tk.IDENTITY, kf.K


def test_keyframe_at_the_cap(solver):
    sc, r = kf.scene(), composed_scene("scene")
    hp = sc["have_point"].astype(bool)
    assert (r["n_candidates"], r["n_new"]) == (259, 40) and len(r["flags"]) == 80          # 88 corners without the cap
    assert set(np.unique(r["flags"])) >= {0, 2, 4, 6, 16, 32} and r["n_accepted"] == (r["flags"] == 0).sum() > 0
    assert np.all(r["flags"][:40][hp] == 32) and not (r["flags"][:40][~hp] == 32).any() and not r["pt"][:40][hp].any()
    assert 0 < r["n_right"] == r["success"].sum() < 80
    g = fused(solver, sc)
    same(g, r)
    # the NumPy chain
    ref = kf.call(kf.reference, sc)
    same(g, ref, ("kp_new", "kp_right", "success", "flags", "n_new", "n_candidates", "lambda_max", "n_right", "n_accepted"))
    tri = ref["flags"] < 16
    rel = np.linalg.norm(g["pt"][tri] - ref["pt"][tri], axis=1) / np.linalg.norm(ref["pt"][tri], axis=1)
    print(f"pt against LAPACK on {tri.sum()} features: rel max {rel.max():.3e} (tol {tr.recorded_tolerance('stereo'):.3e})")
    assert rel.max() <= tr.recorded_tolerance("stereo") and not g["pt"][~tri].any()


def test_features_with_a_point_that_fail_to_track(solver):
    (sc, rows), r = hostile_scene(), composed_scene("hostile")
    assert not r["success"][rows].any() and np.isnan(r["kp_right"][rows[1]]).all()
    assert np.all(r["flags"][rows] == 32) and not r["pt"][rows].any()
    base = composed_scene("scene")
    others = np.ones(len(r["flags"]), bool)
    others[rows] = False
    for k in ("kp_right", "success", "pt", "flags"):                                       # nobody else is touched
        assert np.array_equal(tk.bits(r[k][others]), tk.bits(base[k][others])), k
    same(fused(solver, sc), r)


def test_keyframe_below_the_cap(solver):
    sc = kf.scene()
    r = composed(solver, sc, min_distance=20.0)
    assert r["n_new"] == 28 < sc["max_corners"] and len(r["flags"]) == 68 and r["n_accepted"] > 0
    same(fused(solver, sc, min_distance=20.0), r)
    # and with T_out: accepted points move, the others keep their value
    T = np.hstack([tk_rotation(0.02, -0.03), np.array([[0.5], [-0.2], [1.0]])]).reshape(12)
    rt = composed(solver, sc, min_distance=20.0, T_out=T)
    acc = r["flags"] == 0
    assert np.array_equal(rt["flags"], r["flags"]) and not np.array_equal(rt["pt"][acc], r["pt"][acc])
    assert np.array_equal(tk.bits(rt["pt"][~acc]), tk.bits(r["pt"][~acc]))
    same(fused(solver, sc, min_distance=20.0, T_out=T), rt)


def tk_rotation(pitch, yaw):
    cp, sp, cy, sy = np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    return np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])


def test_stereo_init():
    """n_have = 0, T_out NULL, on a fresh handle; the left image is resident afterwards: no priming call."""
    sc = dict(kf.scene(), max_corners=150, **NONE)
    _, after = images_after()
    s = fresh()
    r = composed(s, sc)
    assert (r["n_candidates"], r["n_new"]) == (444, 127) and r["n_accepted"] > 0 and not (r["flags"] == 32).any()
    t = track_inputs(r, sc)
    ref = s.track_frame(sc["img_left"], after, *t)
    s.close()
    assert ref["n_tracked"] > 100 and ref["n_edges"] == r["n_accepted"] - (~ref["success"] & (r["flags"] == 0)).sum() > 0
    s = fresh()
    same(fused(s, sc), r)
    same(s.track_frame(None, after, *t), ref, TRACK_KEYS)
    s.close()


def test_resident_image():
    import lego_ba
    sc, r = kf.scene(), composed_scene("scene")
    before, after = images_after()
    B = sc["img_left"]
    t0 = track_inputs(r, sc)
    s = fresh()
    track_ref = s.track_frame(B, after, *t0)                              # track(B, C) on a handle of its own
    s.close()
    assert track_ref["n_edges"] > 0 and track_ref["iterations"] > 0
    for max_level in (3, 1):                                               # 1: the keyframe call builds levels 2 and 3 of B
        s = fresh()
        s.track_frame(before, B, *t0, max_level=max_level)
        same(fused(s, sc, img_left=None), r)                               # B is resident: == a fresh handle's call with B
        same(s.track_frame(None, after, *t0), track_ref, TRACK_KEYS)       # and it still is, unchanged
        same(fused(s, sc, img_left=None, img_right=B, max_level=1),        # `after` is resident now
             fused(s, sc, img_left=after, img_right=B, max_level=1))
        s.close()
    # none resident; an argument error in between; another size
    s = fresh()
    with pytest.raises(lego_ba.LhError) as e:
        fused(s, sc, img_left=None)
    assert e.value.status == lego_ba.LH_E_STATE
    same(fused(s, sc), r)                                                  # B becomes resident
    for kw in (dict(max_level=7), dict(max_corners=0), dict(min_distance=-1.0)):
        with pytest.raises(lego_ba.LhError) as e:
            fused(s, sc, img_left=None, **kw)
        assert e.value.status == lego_ba.LH_E_BADARG, kw
    small = np.ascontiguousarray(B[:100, :150])
    with pytest.raises(lego_ba.LhError) as e:
        fused(s, sc, img_left=None, img_right=small)
    assert e.value.status == lego_ba.LH_E_STATE
    same(fused(s, sc, img_left=None), r)                                   # B is still there
    same(s.track_frame(None, after, *t0), track_ref, TRACK_KEYS)
    fused(s, sc, img_left=small, img_right=small, **NONE)                  # the other size becomes resident
    with pytest.raises(lego_ba.LhError) as e:
        fused(s, sc, img_left=None)
    assert e.value.status == lego_ba.LH_E_STATE
    s.close()


def many_features(n):
    """n features the frame has on the scene's images, every second one with a point"""
    kp = images.keypoints(ROWS, COLS, n, seed=5, border=False)
    z = kf.DEPTH * np.random.default_rng(n).uniform(0.8, 1.25, n)
    X = np.stack([(kp[:, 0] - kf.K[2]) / kf.K[0] * z, (kp[:, 1] - kf.K[3]) / kf.K[1] * z, z], 1)
    return dict(kf.scene(), have_kp=kp, have_pts_w=X, have_point=(np.arange(n) % 2).astype(np.uint8), exclude_half=1.5)


@pytest.mark.parametrize("n_have,max_corners", [(0, 7), (1, 7), (63, 7), (64, 7), (65, 7), (257, 7), (250, 40)])
def test_list_sizes(solver, n_have, max_corners):
    """The list's length around the wave, the finish kernel's tile and its stride; (250, 40): n crosses 256 with room
    left under the cap."""
    sc = many_features(n_have)
    kw = dict(max_corners=max_corners, min_distance=20.0 if max_corners == 40 else 8.0)
    r = composed(solver, sc, **kw)
    n = n_have + r["n_new"]
    if max_corners == 40:
        assert 0 < r["n_new"] < 40 and n_have < 256 < n
    else:
        assert r["n_new"] == 7
    assert (r["flags"][:n_have] == 32).sum() == n_have // 2 and r["n_right"] > 0.7 * n
    same(fused(solver, sc, **kw), r)
    if n_have:                                                             # has_point NULL: every feature has a point
        rn = composed(solver, sc, have_point=None, **kw)
        assert np.all(rn["flags"][:n_have] == 32) and rn["n_accepted"] == (rn["flags"] == 0).sum()
        same(fused(solver, sc, have_point=None, **kw), rn)


def test_no_corner(solver):
    sc = kf.scene()
    flat = np.full((ROWS, COLS), 77, np.uint8)
    g = fused(solver, sc, img_left=flat, img_right=flat, **NONE)
    same(g, composed(solver, sc, img_left=flat, img_right=flat, **NONE))
    assert (g["n_new"], g["n_candidates"], g["lambda_max"], g["n_right"], g["n_accepted"]) == (0, 0, 0.0, 0, 0)
    assert g["kp_new"].shape == (0, 2) and g["kp_right"].shape == (0, 2) and g["flags"].shape == (0,)
    # a flat image and features: nothing tracks
    r = composed(solver, sc, img_left=flat, img_right=flat)
    assert r["n_new"] == 0 and r["n_right"] == 0 and set(np.unique(r["flags"])) == {16, 32}
    same(fused(solver, sc, img_left=flat, img_right=flat), r)
    # every pixel inside an exclusion box: no allowed pixel, lambda_max 0; the features still track
    r = composed(solver, sc, exclude_half=500.0)
    assert (r["n_new"], r["n_candidates"], r["lambda_max"]) == (0, 0, 0.0) and r["n_right"] > 30 and len(r["flags"]) == 40
    same(fused(solver, sc, exclude_half=500.0), r)


def test_strided_rows_equal_the_packed_call(solver):
    """121 x 163 inside 121 x 200 buffers whose padding is 255."""
    sc = kf.scene()
    b1, b2 = np.full((ROWS, 200), 255, np.uint8), np.full((ROWS, 200), 255, np.uint8)
    b1[:, :COLS], b2[:, :COLS] = sc["img_left"], sc["img_right"]
    same(fused(solver, sc, img_left=b1[:, :COLS], img_right=b2[:, :COLS]), composed_scene("scene"))
    same(composed(solver, sc, img_left=b1[:, :COLS], img_right=b2[:, :COLS]), composed_scene("scene"))


def test_shared_handle():
    """insert_keyframe between the other entry points leaves each bitwise its fresh-handle result, and is itself the
    composition's at a small shape, a larger one (every buffer grows) and the small one again."""
    import lego_ba
    import test_frontend_shared_handle as sh
    z = np.load(GOLDEN)
    opt = dict(ast.literal_eval(str(z["opt_json"])))
    new = lambda: lego_ba.Solver(device=0, **opt)
    left, right = images.pair(64, 96, shift=(-3.0, 0.0), seed=5)
    kp = images.keypoints(64, 96, 20, seed=2)
    Ks = np.stack([tr.K, tr.K])
    small = dict(kf.scene(), img_left=left, img_right=right, have_kp=kf.scene()["have_kp"][:12] * 0.5,
                 have_pts_w=kf.scene()["have_pts_w"][:12], have_point=kf.scene()["have_point"][:12], max_corners=20)
    large = many_features(257)
    z0 = np.full(len(kp), 20.0)
    Xt = np.stack([(kp[:, 0] - 48.0) / 500.0 * z0, (kp[:, 1] - 32.0) / 500.0 * z0, z0], 1)
    others = {
        "detect": lambda s: s.detect_features(left, max_corners=40, min_distance=5.0, want_eig=True),
        "klt": lambda s: s.klt_track(left, right, kp),
        "lk": lambda s: s.lk_track(left, right, kp, levels=4),
        "tri": lambda s: s.triangulate(*tr.stereo_family(65, seed=3)[:2], K=Ks),
        "stereo": lambda s: s.klt_stereo_landmarks(left, right, kp, tr.stereo_poses(), K=Ks, kp_right_init=kp),
        "lkstereo": lambda s: s.stereo_landmarks(left, right, kp, tr.stereo_poses(), K=Ks, kp_right_init=kp),
        "pose": lambda s: s.estimate_pose(frames.batch(7, 1, n_obs=40)),
        "track": lambda s: s.track_frame(left, right, kp, Xt, None, tk.IDENTITY, (500.0, 500.0, 48.0, 32.0)),
        "solve": lambda s: s.solve({k[3:]: z[k] for k in z.files if k.startswith("in_")}),
    }
    ref = {}
    for name, fn in others.items():
        s = new()
        ref[name] = fn(s)
        s.close()
    s = new()
    kf_ref = {"small": composed(s, small), "large": composed(s, large, max_corners=40, min_distance=20.0)}
    s.close()
    assert kf_ref["small"]["n_new"] > 0 and kf_ref["large"]["n_new"] > 0
    s = new()
    for name, fn in others.items():
        same(fused(s, small), kf_ref["small"])
        sh.same(fn(s), ref[name])
    same(fused(s, large, max_corners=40, min_distance=20.0), kf_ref["large"])
    for name in reversed(list(others)):
        sh.same(others[name](s), ref[name])
        same(fused(s, small), kf_ref["small"])          # small again, in the grown buffers
    s.close()


def test_argument_errors(solver):
    import lego_ba
    sc = kf.scene()
    lib = lego_ba.ba_lib()
    for kw in (dict(max_level=4), dict(max_level=-1), dict(max_iters=0), dict(epsilon=0.0), dict(epsilon=float("nan")),
               dict(min_eig=-1e-9), dict(min_eig=float("nan")), dict(max_corners=0), dict(max_corners=-3),
               dict(quality=-0.1), dict(quality=float("nan")), dict(min_distance=-1.0), dict(min_distance=float("nan"))):
        with pytest.raises(lego_ba.LhError) as e:
            fused(solver, sc, **kw)
        assert e.value.status == lego_ba.LH_E_BADARG, kw
    tiny = np.zeros((11, 40), np.uint8)
    with pytest.raises(lego_ba.LhError) as e:
        fused(solver, sc, img_left=tiny, img_right=tiny)
    assert e.value.status == lego_ba.LH_E_BADARG
    # the raw structs: step < cols and each null pointer
    nh, mc = len(sc["have_kp"]), sc["max_corners"]
    keep = dict(l=np.ascontiguousarray(sc["img_left"]), r=np.ascontiguousarray(sc["img_right"]),
                kp=np.ascontiguousarray(sc["have_kp"]), X=np.ascontiguousarray(sc["have_pts_w"]),
                hp=np.ascontiguousarray(sc["have_point"]), kn=np.zeros((mc, 2), np.float32),
                kr=np.zeros((nh + mc, 2), np.float32), ok=np.zeros(nh + mc, np.uint8), pt=np.zeros((nh + mc, 3)),
                fl=np.zeros(nh + mc, np.uint8))
    a = lego_ba.LhKeyframeInput()
    a.cols, a.rows, a.step = COLS, ROWS, COLS
    a.img_left, a.img_right = keep["l"].ctypes.data, keep["r"].ctypes.data
    a.n_have, a.have_kp, a.have_pts_w, a.have_point = nh, keep["kp"].ctypes.data, keep["X"].ctypes.data, keep["hp"].ctypes.data
    a.exclude_half, a.max_corners, a.quality_level, a.min_distance = 10.0, mc, 0.01, sc["min_distance"]
    a.max_level, a.max_iters, a.epsilon, a.min_eig_threshold = 3, 30, 0.01, 1e-4
    for i in range(12):
        a.pose_Tcw[i] = tk.IDENTITY[i]
    for i in range(24):
        a.cam_pose[i] = sc["cam_pose"].reshape(24)[i]
    for i in range(8):
        a.cam_K[i] = sc["cam_K"].reshape(8)[i]
    a.sing_ratio_thr, a.gate = 1e-3, 1
    a.y_max, a.z_min, a.z_max = sc["gate"]
    res = lego_ba.LhKeyframeResult()
    res.kp_new, res.kp_right, res.success = keep["kn"].ctypes.data, keep["kr"].ctypes.data, keep["ok"].ctypes.data
    res.pt, res.flags = keep["pt"].ctypes.data, keep["fl"].ctypes.data
    call = lambda: lib.lh_insert_keyframe(solver.h, C.byref(a), C.byref(res))
    good = composed_scene("scene")

    def ok_and_equal():
        assert call() == lego_ba.LH_OK
        assert (res.n_new, res.n_right, res.n_accepted) == (good["n_new"], good["n_right"], good["n_accepted"])
        assert np.array_equal(keep["fl"], good["flags"]) and np.array_equal(tk.bits(keep["pt"]), tk.bits(good["pt"]))
    ok_and_equal()
    assert lib.lh_insert_keyframe(None, C.byref(a), C.byref(res)) == lego_ba.LH_E_BADARG
    assert lib.lh_insert_keyframe(solver.h, None, C.byref(res)) == lego_ba.LH_E_BADARG
    assert lib.lh_insert_keyframe(solver.h, C.byref(a), None) == lego_ba.LH_E_BADARG
    a.step = COLS - 1
    assert call() == lego_ba.LH_E_BADARG
    a.step = COLS
    for field in ("img_right", "have_kp"):
        old = getattr(a, field)
        setattr(a, field, None)
        assert call() == lego_ba.LH_E_BADARG, field
        setattr(a, field, old)
    for field in ("kp_new", "kp_right", "success", "pt", "flags"):
        old = getattr(res, field)
        setattr(res, field, None)
        assert call() == lego_ba.LH_E_BADARG, field
        setattr(res, field, old)
    a.n_have = -1
    assert call() == lego_ba.LH_E_BADARG
    a.n_have = nh
    a.max_corners = (1 << 24) - nh + 1                                     # the list's capacity past 2^24
    assert call() == lego_ba.LH_E_BADARG
    a.max_corners = mc
    # a null have_pts_w: an error when some feature can have a point
    a.have_pts_w = None
    assert call() == lego_ba.LH_E_BADARG
    a.have_point = None
    assert call() == lego_ba.LH_E_BADARG
    zero = np.zeros(nh, np.uint8)
    a.have_point = zero.ctypes.data
    assert call() == lego_ba.LH_OK and not (keep["fl"] == 32).any() and res.n_new == good["n_new"]
    a.have_pts_w, a.have_point = keep["X"].ctypes.data, keep["hp"].ctypes.data
    ok_and_equal()                                                         # and no error above changed the resident image
    a.img_left = None
    ok_and_equal()
