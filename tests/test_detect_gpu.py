"""GPU tests of lh_detect_features (include/lego_ba.h; kernels: lego-slam_amd/csrc/lh_gftt.hip) against the NumPy
restatement of its definition (tests/gftt_ref.py).  Every comparison is exact: lambda by bits, keypoints, their
order, the counts, lambda_max.  There is no tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

import gftt_ref as gr
import images
import triangulate_ref as tr

pytestmark = pytest.mark.gpu

# the eig kernel's tile is 32 x 8: 150 x 203 is more than two tiles and a remainder both ways
SHAPES = [((37, 61), 61), ((48, 64), 80), ((3, 3), 3), ((5, 200), 200), ((200, 5), 5), ((150, 203), 203)]


@pytest.fixture(scope="module")
def solver():
    import lego_ba
    s = lego_ba.Solver(device=0)
    yield s
    s.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def scenes():
    """name -> (image, its reference lambda image), computed once and left unchanged."""
    out = {}
    for (shape, step) in SHAPES:
        for kind, img in (("texture", images.pair(*shape, seed=5)[0]), ("noise", gr.noise(*shape, seed=6))):
            img = gr.strided(img, step)
            out[(kind,) + shape] = (img, gr.eig_image(img))
    out["ties"] = (gr.tiled_ties(), gr.eig_image(gr.tiled_ties()))
    return out


def check(g, r, want_eig=False):
    """Everything lh_detect_features returns against the reference, exactly."""
    assert g["n_candidates"] == r["n_candidates"]
    assert g["n_corners"] == r["n_corners"]
    assert bits(g["lambda_max"]) == bits(r["lambda_max"])
    assert np.array_equal(g["kp"], r["kp"])
    assert np.array_equal(bits(g["response"]), bits(r["response"]))
    if want_eig:
        assert np.array_equal(bits(g["eig"]), bits(r["eig"]))


@pytest.mark.parametrize("kind", ["texture", "noise"])
@pytest.mark.parametrize("shape,step", SHAPES)
def test_eig_image_bitwise(solver, scenes, kind, shape, step):
    img, lam = scenes[(kind,) + shape]
    assert img.strides[0] == step
    g = solver.detect_features(img, want_eig=True)
    check(g, gr.detect_ref(img, lam=lam), want_eig=True)


@pytest.mark.parametrize("kw", [dict(), dict(min_distance=3.0, max_corners=0), dict(min_distance=5.0, max_corners=0),
                                dict(min_distance=7.5, max_corners=0), dict(min_distance=20.0, max_corners=0),
                                dict(min_distance=0.5, max_corners=0), dict(min_distance=0.5, max_corners=8),
                                dict(min_distance=5.0, max_corners=1), dict(min_distance=5.0, max_corners=8),
                                dict(min_distance=1.0, max_corners=0, quality=0.0)])
def test_selection(solver, scenes, kw):
    for key in (("noise", 150, 203), ("texture", 150, 203), ("noise", 37, 61), ("texture", 48, 64), ("noise", 5, 200)):
        img, lam = scenes[key]
        r = gr.detect_ref(img, lam=lam, **kw)
        check(solver.detect_features(img, **kw), r)
        if key == ("noise", 150, 203):
            assert r["n_candidates"] > 1500 and 0 < r["n_corners"] <= r["n_candidates"]


def test_unlimited_corners_with_a_small_capacity(solver, scenes):
    """max_corners <= 0: at most kp_capacity corners are written, n_corners is the true count."""
    img, lam = scenes[("noise", 150, 203)]
    r = gr.detect_ref(img, lam=lam, max_corners=0, min_distance=5.0)
    g = solver.detect_features(img, max_corners=0, min_distance=5.0, capacity=10)
    assert g["n_corners"] == r["n_corners"] > 10 and np.array_equal(g["kp"], r["kp"][:10])
    g = solver.detect_features(img, max_corners=0, min_distance=5.0, capacity=0)
    assert g["n_corners"] == r["n_corners"] and len(g["kp"]) == 0


def test_ties(solver, scenes):
    """A 12 x 12 block tiled to 45 x 67: many candidates per lambda (tests/test_detect_cpu.py shows that the other
    tie-break gives other corners)."""
    img, lam = scenes["ties"]
    kw = dict(min_distance=7.0, max_corners=8)
    r = gr.detect_ref(img, lam=lam, **kw)
    assert r["n_corners"] == 8 and len(np.unique(r["response"])) < 8
    check(solver.detect_features(img, want_eig=True, **kw), r, want_eig=True)
    for kw in (dict(min_distance=7.0, max_corners=0), dict(min_distance=0.5, max_corners=0), dict(min_distance=13.0)):
        check(solver.detect_features(img, **kw), gr.detect_ref(img, lam=lam, **kw))


def test_mask_and_exclusion_boxes(solver, scenes):
    img, lam = scenes[("noise", 37, 61)]
    rows, cols = img.shape
    kw = dict(min_distance=3.0, max_corners=0)
    # boxes touching and crossing all four borders, half-integer edges, one far outside, one not a number
    ex = np.array([[10.0, 10.0], [0.0, 18.0], [-4.5, 5.0], [60.0, 20.0], [64.5, 30.5], [30.0, 0.0], [25.5, -9.5],
                   [40.0, 36.0], [14.5, 44.5], [15.5, 26.5], [200.0, 10.0], [np.nan, 5.0]], np.float32)
    r = gr.detect_ref(img, lam=lam, exclude=ex, **kw)
    plain = gr.detect_ref(img, lam=lam, **kw)
    assert 0 < r["n_candidates"] < plain["n_candidates"]
    check(solver.detect_features(img, exclude=ex, **kw), r)
    for half in (0.0, 0.5, 2.5):
        check(solver.detect_features(img, exclude=ex, exclude_half=half, **kw),
              gr.detect_ref(img, lam=lam, exclude=ex, exclude_half=half, **kw))
    # a caller mask (any nonzero byte allows) combined with boxes
    mask = np.random.default_rng(8).integers(0, 3, img.shape).astype(np.uint8) * 127
    mask[:, :3] = 0
    check(solver.detect_features(img, exclude=ex, mask=mask, **kw), gr.detect_ref(img, lam=lam, exclude=ex, mask=mask, **kw))
    check(solver.detect_features(img, mask=mask, **kw), gr.detect_ref(img, lam=lam, mask=mask, **kw))
    # the strongest pixel masked: lambda_max comes from elsewhere, and with it the threshold
    y, x = np.unravel_index(np.argmax(lam), lam.shape)
    for m in (dict(exclude=np.array([[x, y]], np.float32), exclude_half=0.0),
              dict(mask=np.where(lam == lam.max(), 0, 1).astype(np.uint8))):
        r = gr.detect_ref(img, lam=lam, quality=0.3, **m, **kw)
        assert r["lambda_max"] < plain["lambda_max"]
        check(solver.detect_features(img, quality=0.3, **m, **kw), r)
    # lambda_max on the image border (no candidate lies there): only the borders are allowed
    edge = np.zeros(img.shape, np.uint8)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = 1
    g = solver.detect_features(img, mask=edge, **kw)
    assert g["n_corners"] == 0 and g["n_candidates"] == 0 and g["lambda_max"] == lam[edge != 0].max() > 0
    # everything masked, by the mask and by boxes: no corners, LH_OK
    for m in (dict(mask=np.zeros(img.shape, np.uint8)), dict(exclude=np.array([[30.0, 18.0]], np.float32), exclude_half=100.0)):
        g = solver.detect_features(img, **m, **kw)
        assert g["n_corners"] == 0 and g["n_candidates"] == 0 and g["lambda_max"] == 0.0 and len(g["kp"]) == 0
    # a constant image: lambda is 0 everywhere
    g = solver.detect_features(np.full((rows, cols), 77, np.uint8), want_eig=True, **kw)
    assert g["n_corners"] == 0 and g["n_candidates"] == 0 and g["lambda_max"] == 0.0 and not g["eig"].any()


def test_repeatable_across_buffer_growth(solver, scenes):
    """Small, large, small on one handle: the same bits as each on a fresh handle."""
    import lego_ba
    keys = [("noise", 37, 61), ("noise", 150, 203), ("texture", 48, 64), ("noise", 37, 61)]
    kw = dict(min_distance=5.0, max_corners=0, want_eig=True)
    ex = np.array([[20.0, 20.0]], np.float32)
    fresh = []
    for k in keys[:3]:
        s = lego_ba.Solver(device=0)
        fresh.append(s.detect_features(scenes[k][0], exclude=ex, **kw))
        s.close()
    fresh.append(fresh[0])
    s = lego_ba.Solver(device=0)
    for k, f in zip(keys, fresh):
        g = s.detect_features(scenes[k][0], exclude=ex, **kw)
        check(g, f, want_eig=True)
        check(g, gr.detect_ref(scenes[k][0], lam=scenes[k][1], exclude=ex, min_distance=5.0, max_corners=0))
    s.close()


def test_detect_then_stereo_landmarks(solver):
    """The frontend's sequence on one 120 x 160 pair: the detector's keypoints feed lh_stereo_landmarks as they are."""
    left, right = images.pair(120, 160, shift=(-6.0, 0.0), seed=11)
    ex = images.keypoints(120, 160, 6, seed=3, border=False)
    kw = dict(exclude=ex, max_corners=40, min_distance=8.0)
    d, r = solver.detect_features(left, **kw), gr.detect_ref(left, **kw)
    check(d, r)
    assert d["kp"].dtype == np.float32 and 10 < d["n_corners"] <= 40
    poses, Ks = tr.stereo_poses(), np.stack([tr.K, tr.K])
    a = solver.stereo_landmarks(left, right, d["kp"], poses, K=Ks, kp_right_init=d["kp"])
    b = solver.stereo_landmarks(left, right, r["kp"], poses, K=Ks, kp_right_init=r["kp"])
    for k in ("kp2", "success", "flags"):
        assert np.array_equal(a[k], b[k])
    assert np.array_equal(bits(a["pt"]), bits(b["pt"])) and a["n_accepted"] == b["n_accepted"]
    assert a["success"].sum() > 0
    check(solver.detect_features(left, **kw), r)   # and the detector's buffers survive the other entry points


def test_errors(solver):
    import lego_ba
    lib = lego_ba.ba_lib()
    img = gr.noise(16, 24, seed=1)
    kp, ex = np.zeros((8, 2), np.float32), np.zeros((2, 2), np.float32)

    def call(**over):
        a, r = lego_ba.LhDetectInput(), lego_ba.LhDetectResult()
        a.cols, a.rows, a.step, a.img = 24, 16, 24, img.ctypes.data
        a.exclude_half, a.max_corners, a.quality_level, a.min_distance = 10.0, 8, 0.01, 3.0
        r.kp, r.kp_capacity = kp.ctypes.data, 8
        for k, v in over.items():
            setattr(r if k in ("kp", "kp_capacity") else a, k, v)
        return lib.lh_detect_features(solver.h, C.byref(a), C.byref(r)), r

    assert call()[0] == lego_ba.LH_OK
    bad = [dict(img=None), dict(kp=None), dict(cols=2), dict(rows=2), dict(step=23), dict(n_exclude=-1),
           dict(n_exclude=2), dict(kp_capacity=-1), dict(kp_capacity=7), dict(mask=img.ctypes.data, mask_step=23),
           dict(quality_level=-0.5), dict(min_distance=float("nan"))]
    for over in bad:
        assert call(**over)[0] == lego_ba.LH_E_BADARG, over
    assert lib.lh_detect_features(solver.h, None, None) == lego_ba.LH_E_BADARG
    st, r = call(n_exclude=2, exclude_pt=ex.ctypes.data)
    assert st == lego_ba.LH_OK and r.n_corners > 0                 # the handle still works
    st, r = call(max_corners=0, kp_capacity=3)                     # no limit: capacity bounds what is written
    assert st == lego_ba.LH_OK and r.n_corners > 3
