"""GPU tests of lh_track_frame (include/lego_ba.h): one frame of Frontend::Track in one call.

The reference of the fused call is the composition of the entry points the library already tests against their own
oracles, with the host in between (tests/track_ref.py compose): track_ref.guess -> Solver.klt_track(kp2_init=guess) ->
track_ref.select -> Solver.estimate_pose.  Every call is deterministic and every comparison is by bits: kp2, success,
pose_Tcw, is_outlier, edge_chi2, n_tracked, n_edges, n_inliers, iterations.  There is no tolerance in this file (a NaN
kp2, whose payload lh_klt_track's definition leaves open, matches a NaN).  Each case first asserts on the composed
result that it reaches what it is there for."""
import ast
import ctypes as C
import functools
import os

import numpy as np
import pytest

import frames
import images
import track_ref as tk
import triangulate_ref as tr

pytestmark = pytest.mark.gpu

ROWS, COLS = 121, 163
SHIFT = (2.3, -1.7)
K = np.array([517.3, 516.5, COLS / 2, ROWS / 2])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c1_stable_noout_s0.npz")
KEYS = ("kp2", "success", "pose_Tcw", "is_outlier", "edge_chi2", "n_tracked", "n_edges", "n_inliers", "iterations")


def rotation(pitch, yaw):
    cp, sp, cy, sy = np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    return np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])


@functools.lru_cache(maxsize=None)
def scene(n_kp=300, seed=3, shift=SHIFT):
    """The last frame at the identity; the image content moves by `shift`, as under a small rotation of the camera.
    Map points: the keypoints back-projected at depths U(8, 60), on about 80 % of the features, about 8 % of them
    displaced sideways by 3-10 % of their depth.  Predicted pose: 0.6 of that rotation, slightly perturbed."""
    i1, i2 = images.pair(ROWS, COLS, shift=shift, seed=seed)
    kp1 = images.keypoints(ROWS, COLS, n_kp, seed)
    rng = np.random.default_rng(seed + 50)
    n = len(kp1)
    z = rng.uniform(8, 60, n)
    X = np.stack([(kp1[:, 0] - K[2]) / K[0] * z, (kp1[:, 1] - K[3]) / K[1] * z, z], 1)
    hp = (rng.uniform(size=n) < 0.8).astype(np.uint8)
    moved = rng.uniform(size=n) < 0.08
    X[moved, 0] += rng.choice([-1.0, 1.0], moved.sum()) * rng.uniform(0.03, 0.10, moved.sum()) * z[moved]
    R = rotation(-0.6 * shift[1] / K[1] + 2e-4, 0.6 * shift[0] / K[0] - 3e-4)
    pose = np.hstack([R, np.array([[0.004], [-0.003], [0.006]])]).reshape(12)
    for a in (i1, i2, kp1, X, hp, pose):
        a.setflags(write=False)
    return dict(img_last=i1, img_cur=i2, kp1=kp1, pts_w=X, has_point=hp, pose=pose, K=K)


def third_image():
    """C of the resident-image cases: B moved on by another shift"""
    return images.pair(ROWS, COLS, shift=(SHIFT[0] + 1.9, SHIFT[1] - 1.2), seed=3)[1]


@pytest.fixture(scope="module")
def solver():
    import lego_ba
    s = lego_ba.Solver(device=0)
    yield s
    s.close()


def fresh():
    import lego_ba
    return lego_ba.Solver(device=0)


def same(g, r, keys=KEYS):
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
    a = dict(sc)
    a.update(kw)
    return s.track_frame(a.pop("img_last"), a.pop("img_cur"), a.pop("kp1"), a.pop("pts_w"), a.pop("has_point"),
                         a.pop("pose"), a.pop("K"), **a)


def composed(s, sc, **kw):
    a = dict(sc)
    a.update(kw)
    return tk.compose(s, a.pop("img_last"), a.pop("img_cur"), a.pop("kp1"), a.pop("pts_w"), a.pop("has_point"),
                      a.pop("pose"), a.pop("K"), **a)


@functools.lru_cache(maxsize=None)
def composed_frame(n_kp):
    """The composition on the scene, on a handle of its own: computed once, shared, left unchanged."""
    s = fresh()
    r = composed(s, scene(n_kp))
    s.close()
    return r


def test_frame_inside_the_fast_path(solver):
    sc, r = scene(), composed_frame(300)
    hp, ok = sc["has_point"].astype(bool), r["success"]
    assert len(hp) == 308
    assert (ok & ~hp).sum() > 0                    # tracked features without a point
    assert (~ok & hp).sum() > 0                    # features with a point that fail to track
    assert 0 < r["n_edges"] < 256                  # k_frames' one-edge-per-thread path
    assert r["n_edges"] == (ok & hp).sum() and r["n_tracked"] == ok.sum()
    assert r["iterations"] >= 2
    assert 0 < r["is_outlier"].sum() < r["n_edges"] and r["n_inliers"] == r["n_edges"] - r["is_outlier"].sum()
    assert not np.array_equal(r["pose_Tcw"], sc["pose"])
    same(fused(solver, sc), r)


def test_frame_past_the_fast_path(solver):
    """About 640 keypoints: the pack crosses tile boundaries and k_frames takes its strided path."""
    sc, r = scene(632), composed_frame(632)
    assert len(sc["kp1"]) == 640 and r["n_edges"] > 256 and r["iterations"] >= 2
    assert 0 < r["is_outlier"].sum() < r["n_edges"]
    same(fused(solver, sc), r)


@functools.lru_cache(maxsize=None)
def sure_features():
    """The features that track from either guess, the projected point and kp1: a feature's track depends on nothing but
    its own guess, so whatever has_point says, all of them track and has_point alone decides the edges."""
    sc = scene()
    s = fresh()
    ok = composed(s, sc, has_point=None)["success"] & composed(s, sc, has_point=np.zeros(len(sc["kp1"]), np.uint8))["success"]
    s.close()
    return np.flatnonzero(ok)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_pack_edges(solver, n):
    """Around the wave and the tile: has_point all ones, alternating, and only the last feature."""
    full = scene()
    inner = sure_features()[:n]
    assert len(inner) == n
    sc = dict(full, kp1=full["kp1"][inner], pts_w=full["pts_w"][inner])
    last = np.zeros(n, np.uint8)
    last[-1] = 1
    for name, hp in (("ones", np.ones(n, np.uint8)), ("null", None), ("alternating", (np.arange(n) % 2).astype(np.uint8)),
                     ("last", last)):
        r = composed(solver, sc, has_point=hp)
        assert r["n_tracked"] == n, name
        assert r["n_edges"] == (n if hp is None else int(hp.sum())), name
        same(fused(solver, sc, has_point=hp), r)


def test_hostile_guesses(solver):
    """A point at zero depth in the camera, one behind it, one far outside the image: no error, success 0 where the
    composition says so, every other feature unchanged."""
    sc = dict(scene(), pose=tk.IDENTITY)                   # the camera frame is the world's: Pc is the point itself
    base = composed(solver, sc)
    hp = sc["has_point"].copy()
    X = sc["pts_w"].copy()
    rows = np.flatnonzero(hp.astype(bool) & base["success"])[:5]
    X[rows[0]] = (1.0, 2.0, 0.0)                           # zero depth: (+inf, +inf)
    X[rows[1]] = (0.0, 0.0, 0.0)                           # the camera centre: (NaN, NaN)
    X[rows[2]] = (0.3, -0.2, -12.0)                        # behind the camera
    X[rows[3]] = (400.0, 3.0, 5.0)                         # far outside the image
    X[rows[4]] = (1e39, 1.0, 1e-3)                         # past FLT_MAX
    g0 = tk.guess(X, hp, sc["kp1"], sc["pose"], tk.IDENTITY, K)
    assert np.isposinf(g0[rows[0]]).all() and np.isnan(g0[rows[1]]).all() and np.isposinf(g0[rows[4], 0])
    assert np.isfinite(g0[rows[2]]).all() and g0[rows[3], 0] > 10 * COLS
    r = composed(solver, sc, pts_w=X)
    assert not r["success"][rows[[0, 1, 3, 4]]].any() and r["n_edges"] > 0
    g = fused(solver, sc, pts_w=X)
    same(g, r)
    others = np.ones(len(hp), bool)
    others[rows] = False
    same({k: g[k][others] for k in ("kp2", "success")}, {k: base[k][others] for k in ("kp2", "success")}, ("kp2", "success"))


def test_no_edge(solver):
    sc = scene()
    n = len(sc["kp1"])
    # no feature has a point (and then pts_w may be NULL)
    for pts in (sc["pts_w"], None):
        g = fused(solver, sc, has_point=np.zeros(n, np.uint8), pts_w=pts)
        same(g, composed(solver, sc, has_point=np.zeros(n, np.uint8), pts_w=pts))
        assert g["n_tracked"] > 0 and (g["n_edges"], g["n_inliers"], g["iterations"]) == (0, 0, 0)
        assert tk.bits(g["pose_Tcw"]).tolist() == tk.bits(sc["pose"]).tolist()
        assert not g["is_outlier"].any() and not g["edge_chi2"].any()
    # every track fails: keypoints inside a flat block
    i1, i2 = sc["img_last"].copy(), sc["img_cur"].copy()
    i1[30:80, 40:110] = 77
    i2[30:80, 40:110] = 77
    rng = np.random.default_rng(9)
    kp = np.stack([rng.uniform(58, 92, 40), rng.uniform(48, 62, 40)], 1).astype(np.float32)
    z = np.full(40, 20.0)
    X = np.stack([(kp[:, 0] - K[2]) / K[0] * z, (kp[:, 1] - K[3]) / K[1] * z, z], 1)
    flat = dict(sc, img_last=i1, img_cur=i2, kp1=kp, pts_w=X, has_point=None, pose=tk.IDENTITY)
    r = composed(solver, flat)
    assert not r["success"].any()
    g = fused(solver, flat)
    same(g, r)
    assert (g["n_tracked"], g["n_edges"], g["n_inliers"], g["iterations"]) == (0, 0, 0, 0)
    assert tk.bits(g["pose_Tcw"]).tolist() == tk.bits(tk.IDENTITY).tolist()
    # no feature at all
    g = fused(solver, sc, kp1=np.zeros((0, 2), np.float32), pts_w=np.zeros((0, 3)), has_point=np.zeros(0, np.uint8))
    assert g["kp2"].shape == (0, 2) and g["success"].shape == (0,)
    assert (g["n_tracked"], g["n_edges"], g["n_inliers"], g["iterations"]) == (0, 0, 0, 0)
    assert tk.bits(g["pose_Tcw"]).tolist() == tk.bits(sc["pose"]).tolist()


def other_calls(s):
    """Every other entry point once, at shapes that make their buffers (the tracker's among them) grow."""
    z = np.load(GOLDEN)
    left, right = images.pair(150, 200, shift=(-3.0, 0.0), seed=5)
    kp = images.keypoints(150, 200, 400, seed=2)
    Ks = np.stack([tr.K, tr.K])
    s.klt_track(left, right, kp)
    s.detect_features(left, max_corners=40, min_distance=5.0)
    s.klt_stereo_landmarks(left, right, kp, tr.stereo_poses(), K=Ks, kp_right_init=kp)
    s.estimate_pose(frames.batch(7, 2, n_obs=[400, 90]))
    s.solve({k[3:]: z[k] for k in z.files if k.startswith("in_")})


def test_resident_image():
    import lego_ba
    sc = scene()
    A, B, Cimg = sc["img_last"], sc["img_cur"], third_image()
    s = fresh()
    ref = fused(s, sc, img_last=B, img_cur=Cimg)                    # track(B, C) on a fresh handle
    s.close()
    assert ref["n_edges"] > 0 and ref["iterations"] > 0
    for between in (False, True):
        s = fresh()
        same(fused(s, sc), composed_frame(300))                       # track(A, B)
        if between:
            other_calls(s)
        same(fused(s, sc, img_last=None, img_cur=Cimg), ref)          # track(None, C)
        same(fused(s, sc, img_last=None, img_cur=A, max_level=1),     # and C is resident now, with any max_level
             fused(s, sc, img_last=Cimg, img_cur=A, max_level=1))
        same(fused(s, sc, img_last=None), composed_frame(300))        # A resident with two levels: the others are built
        s.close()
    # no resident image; one of another size; an argument error in between; the priming call
    s = fresh()
    with pytest.raises(lego_ba.LhError) as e:
        fused(s, sc, img_last=None)
    assert e.value.status == lego_ba.LH_E_STATE
    none = dict(kp1=np.zeros((0, 2), np.float32), pts_w=None, has_point=None)
    g = fused(s, sc, img_last=None, img_cur=B, **none)                # priming: n_points == 0
    assert g["n_tracked"] == 0 and tk.bits(g["pose_Tcw"]).tolist() == tk.bits(sc["pose"]).tolist()
    with pytest.raises(lego_ba.LhError) as e:
        fused(s, sc, img_last=None, img_cur=Cimg, max_level=7)
    assert e.value.status == lego_ba.LH_E_BADARG
    same(fused(s, sc, img_last=None, img_cur=Cimg), ref)              # B is still there
    small = np.ascontiguousarray(A[:100, :150])
    with pytest.raises(lego_ba.LhError) as e:
        fused(s, sc, img_last=None, img_cur=small)
    assert e.value.status == lego_ba.LH_E_STATE
    same(fused(s, sc, img_last=None, img_cur=A, max_level=1),         # a state error leaves C resident
         fused(s, sc, img_last=Cimg, img_cur=A, max_level=1))
    fused(s, sc, img_last=None, img_cur=small, **none)                # prime at the other size
    with pytest.raises(lego_ba.LhError) as e:
        fused(s, sc, img_last=None, img_cur=B)
    assert e.value.status == lego_ba.LH_E_STATE
    s.close()


def test_strided_rows_equal_the_packed_call(solver):
    """121 x 163 inside 121 x 200 buffers whose padding is 255."""
    sc = scene()
    b1, b2 = np.full((ROWS, 200), 255, np.uint8), np.full((ROWS, 200), 255, np.uint8)
    b1[:, :COLS], b2[:, :COLS] = sc["img_last"], sc["img_cur"]
    same(fused(solver, sc, img_last=b1[:, :COLS], img_cur=b2[:, :COLS]), composed_frame(300))


def test_shared_handle():
    """track_frame between the other frontend calls leaves each bitwise its fresh-handle result, and is itself the
    composition's at a small shape, a larger one (every buffer grows) and the small one again."""
    import test_frontend_shared_handle as sh
    z = np.load(GOLDEN)
    opt = dict(ast.literal_eval(str(z["opt_json"])))
    import lego_ba
    new = lambda: lego_ba.Solver(device=0, **opt)
    left, right = images.pair(64, 96, shift=(-3.0, 0.0), seed=5)
    kp = images.keypoints(64, 96, 20, seed=2)
    Ks = np.stack([tr.K, tr.K])
    others = {
        "detect": lambda s: s.detect_features(left, max_corners=40, min_distance=5.0, want_eig=True),
        "klt": lambda s: s.klt_track(left, right, kp),
        "lk": lambda s: s.lk_track(left, right, kp, levels=4),
        "tri": lambda s: s.triangulate(*tr.stereo_family(65, seed=3)[:2], K=Ks),
        "stereo": lambda s: s.klt_stereo_landmarks(left, right, kp, tr.stereo_poses(), K=Ks, kp_right_init=kp),
        "pose": lambda s: s.estimate_pose(frames.batch(7, 1, n_obs=40)),
    }
    ref = {}
    for name, fn in others.items():
        s = new()
        ref[name] = fn(s)
        s.close()
    small = scene()
    inner = np.arange(40)
    small = dict(small, kp1=small["kp1"][inner], pts_w=small["pts_w"][inner], has_point=small["has_point"][inner])
    s = new()
    track_ref = {"small": composed(s, small), "large": composed(s, scene(632))}
    s.close()
    s = new()
    for name, fn in others.items():
        same(fused(s, small), track_ref["small"])
        sh.same(fn(s), ref[name])
    same(fused(s, scene(632)), track_ref["large"])
    for name in reversed(list(others)):
        sh.same(others[name](s), ref[name])
        same(fused(s, small), track_ref["small"])        # small again, in the grown buffers
    s.close()


def test_partial_outputs(solver):
    sc, r = scene(), composed_frame(300)
    rest = tuple(k for k in KEYS if k not in ("is_outlier", "edge_chi2"))
    for flag, chi2 in ((False, False), (True, False), (False, True)):
        g = fused(solver, sc, want_outlier=flag, want_chi2=chi2)
        assert (g["is_outlier"] is None) == (not flag) and (g["edge_chi2"] is None) == (not chi2)
        same(g, r, rest + (("is_outlier",) if flag else ()) + (("edge_chi2",) if chi2 else ()))


def test_argument_errors(solver):
    import lego_ba
    sc = scene()
    lib = lego_ba.ba_lib()
    n = len(sc["kp1"])
    for kw in (dict(max_level=4), dict(max_level=-1), dict(max_iters=0), dict(epsilon=0.0), dict(epsilon=float("nan")),
               dict(min_eig=-1e-9), dict(min_eig=float("nan"))):
        with pytest.raises(lego_ba.LhError) as e:
            fused(solver, sc, **kw)
        assert e.value.status == lego_ba.LH_E_BADARG, kw
    tiny = np.zeros((11, 40), np.uint8)
    with pytest.raises(lego_ba.LhError) as e:
        fused(solver, sc, img_last=tiny, img_cur=tiny)
    assert e.value.status == lego_ba.LH_E_BADARG
    # the raw structs: step < cols and each null pointer
    a, _keep, k2, ok = solver._klt_input(sc["img_last"], sc["img_cur"], sc["kp1"], None, 3, 30, 0.01, 1e-4)
    X, hp = np.ascontiguousarray(sc["pts_w"]), np.ascontiguousarray(sc["has_point"])
    t = lego_ba.LhTrackInput()
    t.klt, t.pts_w, t.has_point = a, X.ctypes.data, hp.ctypes.data
    for i in range(12):
        t.pose_Tcw[i], t.cam_ext[i] = sc["pose"][i], tk.IDENTITY[i]
    for i in range(4):
        t.K[i] = K[i]
    res = lego_ba.LhTrackResult()
    res.kp2, res.success = k2.ctypes.data, ok.ctypes.data
    call = lambda: lib.lh_track_frame(solver.h, C.byref(t), C.byref(res))
    assert call() == lego_ba.LH_OK and res.n_edges == composed_frame(300)["n_edges"]
    assert lib.lh_track_frame(None, C.byref(t), C.byref(res)) == lego_ba.LH_E_BADARG
    assert lib.lh_track_frame(solver.h, None, C.byref(res)) == lego_ba.LH_E_BADARG
    assert lib.lh_track_frame(solver.h, C.byref(t), None) == lego_ba.LH_E_BADARG
    t.klt.step = COLS - 1
    assert call() == lego_ba.LH_E_BADARG
    t.klt.step = COLS
    for field in ("img2", "kp1"):
        keep = getattr(t.klt, field)
        setattr(t.klt, field, None)
        assert call() == lego_ba.LH_E_BADARG, field
        setattr(t.klt, field, keep)
    for field in ("kp2", "success"):
        keep = getattr(res, field)
        setattr(res, field, None)
        assert call() == lego_ba.LH_E_BADARG, field
        setattr(res, field, keep)
    t.klt.n_points = -1
    assert call() == lego_ba.LH_E_BADARG
    t.klt.n_points = n
    # a null pts_w: an error when some feature can have a point
    t.pts_w = None
    assert call() == lego_ba.LH_E_BADARG
    t.has_point = None
    assert call() == lego_ba.LH_E_BADARG
    zero = np.zeros(n, np.uint8)
    t.has_point = zero.ctypes.data
    assert call() == lego_ba.LH_OK and res.n_edges == 0
    t.pts_w, t.has_point = X.ctypes.data, hp.ctypes.data
    assert call() == lego_ba.LH_OK and res.n_edges == composed_frame(300)["n_edges"]
