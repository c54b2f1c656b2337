"""GPU tests of lh_klt_track / lh_klt_stereo_landmarks (include/lego_ba.h): k_klt_pyr and k_klt_track
against the NumPy restatement of the definition (tests/klt_ref.py), kp2 and success bit for bit.  Every case first
asserts, on the restatement alone, that its input reaches the branch it is there for (the exit counts in the comments
are the restatement's); none hangs on a threshold being nearly met (no minEig within 1e-3 relative of the threshold).
OpenCV is not available here: parity with cv::calcOpticalFlowPyrLK itself is not tested."""
import ctypes as C
import functools

import numpy as np
import pytest

import images
import klt_ref as kr
import triangulate_ref as tr

ROWS, COLS = 121, 163            # 163 -> 82 -> 41 -> 21 wide: odd and even levels
SHIFT = (2.3, -1.7)
FAR = (9.6, 4.2)


@functools.lru_cache(maxsize=None)
def scene(rows=ROWS, cols=COLS, shift=SHIFT, seed=3, n=60, flat=False, uniform=False):
    i1, i2 = images.pair(rows, cols, shift=shift, seed=seed)
    if flat:
        i1[30:80, 40:110] = 77
        i2[30:80, 40:110] = 77
    if uniform:   # in [-3, size + 3): an image too small for images.keypoints' inner margin
        rng = np.random.default_rng(seed)
        k1 = np.stack([rng.uniform(-3, cols + 3, n), rng.uniform(-3, rows + 3, n)], 1).astype(np.float32)
    else:
        k1 = images.keypoints(rows, cols, n, seed)
    for a in (i1, i2, k1):
        a.setflags(write=False)
    return i1, i2, k1


def guess_of(k1, guess):
    return None if guess is None else (k1 + np.array(guess, np.float32)).astype(np.float32)


# name -> (scene arguments, guess offset or None, tracker arguments)
CASES = {
    "odd_levels": (dict(), None, dict()),
    "odd_levels_guess": (dict(), (0.8 * SHIFT[0], 0.8 * SHIFT[1]), dict()),
    "short_30x40": (dict(rows=30, cols=40, n=20), None, dict()),
    "short_24x47": (dict(rows=24, cols=47, n=20), None, dict()),
    "short_13x17": (dict(rows=13, cols=17, n=16, uniform=True), None, dict()),
    "cap_48x64": (dict(rows=48, cols=64, shift=(5.5, -3.0), n=40), None, dict()),
    "cap_two_iters": (dict(), None, dict(max_iters=2)),
    "flat_block": (dict(flat=True), None, dict()),
    "far": (dict(shift=FAR), None, dict()),
    "far_guess": (dict(shift=FAR), (40.0, -30.0), dict()),
    "far_one_level": (dict(shift=FAR), None, dict(max_level=0)),
    "one_frame": (dict(rows=376, cols=1241, n=500), (0.0, 0.0), dict()),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    sc, guess, kw = CASES[name]
    i1, i2, k1 = scene(**sc)
    return kr.track(i1, i2, k1, guess_of(k1, guess), **kw)


def coverage(name):
    """What the case must reach, asserted on the restatement alone."""
    r = reference(name)
    n = len(r["success"])
    tracked = int(r["success"].sum())
    assert kr.min_eig_clear(r, CASES[name][2].get("min_eig", 1e-4)), name
    if name.startswith("odd_levels"):   # 4 levels; exits by epsilon and by oscillation (6 and 4); range fails at level 0 (2)
        assert r["levels"] == 4 and n == 68
        assert kr.count(r, kr.X_EPS) > 0 and kr.count(r, kr.X_OSC) > 0
        assert kr.count(r, kr.X_RANGE_P, 0) + kr.count(r, kr.X_RANGE_Q, 0) > 0
        assert 0 < tracked < n
    elif name.startswith("short"):   # the pyramid's early stop
        assert r["levels"] == {"short_30x40": 2, "short_24x47": 2, "short_13x17": 1}[name]
        assert r["levels"] == len(kr.pyramid(scene(**CASES[name][0])[0], 3)) < 4
        assert kr.count(r, kr.X_EPS) + kr.count(r, kr.X_OSC) > 0
    elif name.startswith("cap"):   # a point leaving by max_iters
        assert kr.count(r, kr.X_MAX_ITERS) > 0
        if name == "cap_two_iters":
            assert r["iters"].max() == 2 and kr.count(r, kr.X_MAX_ITERS) > 100
    elif name == "flat_block":   # min-eig fails at level 0 give success 0
        lost = r["exits"][:, 0] == kr.X_MIN_EIG
        assert lost.sum() > 0 and not r["success"][lost].any()
        assert 0 < tracked < n
    elif name.startswith("far"):   # some point moves > 11 px within a level: its taps leave the staged window
        assert r["moved"].max() > 11
        assert 24 <= tracked <= 63 and n == 68
    elif name == "one_frame":
        assert r["levels"] == 4 and tracked > n // 2
    return r


@pytest.fixture(scope="module")
def solver():
    import lego_ba
    s = lego_ba.Solver(device=0)
    yield s
    s.close()


def assert_same(g, r, nan=False):
    """nan: a NaN keypoint's kp2 is NaN (whose payload the definition leaves open); every other value bit for bit"""
    assert np.array_equal(g["success"], r["success"])
    fin = ~np.isnan(r["kp2"]) if nan else np.ones(r["kp2"].shape, bool)
    assert np.array_equal(np.isnan(g["kp2"]), ~fin)
    assert np.array_equal(kr.bits(g["kp2"])[fin], kr.bits(r["kp2"])[fin])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_klt_bitwise_vs_restatement(solver, name):
    r = coverage(name)
    sc, guess, kw = CASES[name]
    i1, i2, k1 = scene(**sc)
    assert_same(solver.klt_track(i1, i2, k1, kp2_init=guess_of(k1, guess), **kw), r)


@pytest.mark.gpu
def test_gpu_klt_strided_rows_equal_the_packed_call(solver):
    """121 x 163 inside a 121 x 200 buffer whose padding is 255: no tap reads a row's padding."""
    i1, i2, k1 = scene()
    b1, b2 = np.full((ROWS, 200), 255, np.uint8), np.full((ROWS, 200), 255, np.uint8)
    b1[:, :COLS], b2[:, :COLS] = i1, i2
    v1, v2 = b1[:, :COLS], b2[:, :COLS]
    assert v1.strides == (200, 1) and not v1.flags["C_CONTIGUOUS"]
    g = solver.klt_track(v1, v2, k1)
    assert_same(g, solver.klt_track(i1, i2, k1))
    assert_same(g, reference("odd_levels"))


@pytest.mark.gpu
def test_gpu_klt_stereo_landmarks_is_klt_track_then_triangulate(solver):
    """One stereo frame (a horizontal shift as disparity): kp2 and success are bitwise klt_track's, pt and flags bitwise
    triangulate's on them, failed tracks carry bit 4 alone."""
    rows, cols = 120, 160
    left, right = images.pair(rows, cols, shift=(-6.0, 0.0), seed=11)
    k1 = images.keypoints(rows, cols, 100, seed=11)
    poses = tr.stereo_poses()
    Ks = np.stack([tr.K, tr.K])
    c, s_ = np.cos(-0.2), np.sin(-0.2)
    T = np.array([c, 0, s_, 0.4, 0, 1, 0, 0.1, -s_, 0, c, -3.0])
    kl = solver.klt_track(left, right, k1, kp2_init=k1)
    assert_same(kl, kr.track(left, right, k1, k1))
    st = solver.klt_stereo_landmarks(left, right, k1, poses, K=Ks, kp_right_init=k1, T_out=T)
    assert np.array_equal(kr.bits(st["kp2"]), kr.bits(kl["kp2"])) and np.array_equal(st["success"], kl["success"])
    ok = kl["success"]
    assert 0 < ok.sum() < len(ok)
    pairs = np.stack([k1, kl["kp2"]], 1).astype(np.float64)[ok]           # floats widened, as toVec2 does
    tri = solver.triangulate(poses, pairs, K=Ks, T_out=T)
    f64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
    assert np.array_equal(st["flags"][ok], tri["flags"])
    assert np.array_equal(f64(st["pt"][ok]), f64(tri["pt"]))
    assert np.all(st["flags"][~ok] == tr.F_TRACK) and not np.any(st["pt"][~ok])
    assert st["n_accepted"] == tri["n_accepted"] == int(np.sum(st["flags"] == 0))
    assert not np.any(st["flags"][ok] & tr.F_TRACK)


@pytest.mark.gpu
def test_gpu_klt_growth_small_large_small():
    """The buffers grow and are reused: small, large, small on one handle give the bits of fresh calls."""
    import lego_ba
    s = lego_ba.Solver(device=0)
    small, large = ("short_30x40", "odd_levels")
    for name in (small, large, small):
        sc, guess, kw = CASES[name]
        i1, i2, k1 = scene(**sc)
        assert_same(s.klt_track(i1, i2, k1, kp2_init=guess_of(k1, guess), **kw), reference(name))
    s.close()


@pytest.mark.gpu
def test_gpu_klt_empty_errors_and_nan(solver):
    import lego_ba
    i1, i2, k1 = scene()
    r = solver.klt_track(i1, i2, np.zeros((0, 2), np.float32))
    assert r["kp2"].shape == (0, 2) and r["success"].shape == (0,)
    poses = tr.stereo_poses()
    st = solver.klt_stereo_landmarks(i1, i2, np.zeros((0, 2), np.float32), poses)
    assert st["pt"].shape == (0, 3) and st["n_accepted"] == 0
    bad = [dict(max_level=4), dict(max_level=-1), dict(max_iters=0), dict(epsilon=0.0), dict(epsilon=-1.0),
           dict(epsilon=float("nan")), dict(min_eig=-1e-9), dict(min_eig=float("nan"))]
    for kw in bad:
        with pytest.raises(lego_ba.LhError) as e:
            solver.klt_track(i1, i2, k1, **kw)
        assert e.value.status == lego_ba.LH_E_BADARG, kw
        with pytest.raises(lego_ba.LhError) as e:
            solver.klt_stereo_landmarks(i1, i2, k1, poses, **kw)
        assert e.value.status == lego_ba.LH_E_BADARG, kw
    for shape in ((11, 40), (40, 11)):                                    # a size < 12
        with pytest.raises(lego_ba.LhError) as e:
            solver.klt_track(np.zeros(shape, np.uint8), np.zeros(shape, np.uint8), k1[:3])
        assert e.value.status == lego_ba.LH_E_BADARG
    # step < cols, and each null pointer with n_points > 0
    a, _keep, k2, ok = solver._klt_input(i1, i2, k1, None, 3, 30, 0.01, 1e-4)
    res = lego_ba.LhLkResult()
    res.kp2, res.success = k2.ctypes.data, ok.ctypes.data
    lib = lego_ba.ba_lib()
    assert lib.lh_klt_track(solver.h, C.byref(a), C.byref(res)) == lego_ba.LH_OK
    a.step = COLS - 1
    assert lib.lh_klt_track(solver.h, C.byref(a), C.byref(res)) == lego_ba.LH_E_BADARG
    a.step = COLS
    for field in ("img1", "img2", "kp1"):
        keep = getattr(a, field)
        setattr(a, field, None)
        assert lib.lh_klt_track(solver.h, C.byref(a), C.byref(res)) == lego_ba.LH_E_BADARG, field
        setattr(a, field, keep)
    for field in ("kp2", "success"):
        keep = getattr(res, field)
        setattr(res, field, None)
        assert lib.lh_klt_track(solver.h, C.byref(a), C.byref(res)) == lego_ba.LH_E_BADARG, field
        setattr(res, field, keep)
    a.n_points = -1
    assert lib.lh_klt_track(solver.h, C.byref(a), C.byref(res)) == lego_ba.LH_E_BADARG
    # a NaN or infinite keypoint (or guess) gives success 0 and is no error; its neighbours are untouched
    kn = k1.copy()
    kn[3] = (np.nan, 20.0)
    kn[5] = (30.0, np.inf)
    g = solver.klt_track(i1, i2, kn)
    assert_same(g, kr.track(i1, i2, kn), nan=True)
    assert not g["success"][3] and not g["success"][5]
    keepers = np.ones(len(k1), bool)
    keepers[[3, 5]] = False
    ref = reference("odd_levels")
    assert np.array_equal(kr.bits(g["kp2"][keepers]), kr.bits(ref["kp2"][keepers]))
    init = k1.copy()
    init[7] = (np.nan, np.nan)
    g = solver.klt_track(i1, i2, k1, kp2_init=init)
    assert_same(g, kr.track(i1, i2, k1, init), nan=True)
    assert not g["success"][7]
