"""GPU tests of lh_triangulate and lh_stereo_landmarks (include/lego_ba.h): k_triangulate (Givens QR + one-sided
Jacobi SVD, one lane per point, lego-slam_amd/csrc/lh_tri.hip) against legoslam::triangulation restated on
LAPACK (tests/triangulate_ref.py).

Bounds: flags equal the reference's exactly (tests/test_triangulate_cpu.py asserts that no reference ratio of
these sets lies within 1e-6 of the threshold); points within 100x the reference's own recorded one-ulp
sensitivity (tests/golden/triangulation_tol.json); sigma3 / sigma2 within 1e-9 relative wherever the
reference's exceeds 1e-12."""
import ctypes as C

import numpy as np
import pytest

import images
import triangulate_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    import lego_ba
    s = lego_ba.Solver(device=0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def stereo():
    poses, xy, px = tr.stereo_set()
    return dict(poses=poses, xy=xy, px=px, ref=tr.triangulate_ref(poses, xy.reshape(-1, 2)))


@pytest.fixture(scope="module")
def csr():
    poses, ptr, vp, xy = tr.csr_set()
    return dict(poses=poses, ptr=ptr, vp=vp, xy=xy, ref=tr.triangulate_ref(poses, xy, ptr, vp))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def same_bits(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("pt", "flags", "sing_ratio"))


def check_against_reference(g, r, which):
    """Test 2's checks: flags, points, ratio.  Prints each figure before it asserts."""
    rel = np.linalg.norm(g["pt"] - r["pt"], axis=1) / np.linalg.norm(r["pt"], axis=1)
    big = r["sing_ratio"] > 1e-12
    rr = np.abs(g["sing_ratio"] - r["sing_ratio"])[big] / r["sing_ratio"][big]
    print(f"{which} n={len(rel)}: pt rel max {rel.max():.3e} (tol {tr.recorded_tolerance(which):.3e}), "
          f"ratio rel max {rr.max() if rr.size else 0.0:.3e}, flags differ {int(np.sum(g['flags'] != r['flags']))}")
    assert np.array_equal(g["flags"], r["flags"])
    assert g["n_accepted"] == int(np.sum(r["flags"] == 0))
    assert rel.max() <= tr.recorded_tolerance(which)
    assert np.all(rr <= 1e-9)


def test_reference_gtest_case(solver):
    """LEGOSLAMTest.Triangulation (test/legoslam_test_triangulation.cpp:5-23) through the CSR path: the reference's
    own expectation, EXPECT_TRUE and EXPECT_NEAR 0.01 on (30, 20, 10)."""
    poses, xy, pw, near = tr.gtest_case()
    g = solver.triangulate(poses, xy, view_ptr=[0, 3], view_pose=[0, 1, 2])
    assert g["flags"][0] == 0 and g["n_accepted"] == 1
    assert np.all(np.abs(g["pt"][0] - pw) < near)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_stereo_family_fixed_views(solver, stereo, n):
    g = solver.triangulate(stereo["poses"], stereo["xy"][:n])
    check_against_reference(g, {k: v[:n] for k, v in stereo["ref"].items() if k != "n_accepted"}, "stereo")


def test_batch_independence(solver, stereo):
    """A point's bits do not depend on its batch position or the batch size."""
    xy = stereo["xy"]
    full = solver.triangulate(stereo["poses"], xy)
    rejected = int(np.flatnonzero(stereo["ref"]["flags"])[0])
    for j in (0, 63, 64, 200, 256, rejected):
        alone = solver.triangulate(stereo["poses"], xy[j:j + 1])
        first = solver.triangulate(stereo["poses"], np.concatenate([xy[j:j + 1], xy[:64]]))
        for k in ("pt", "flags", "sing_ratio"):
            assert np.array_equal(bits(full[k][j:j + 1]), bits(alone[k])), (j, k)
            assert np.array_equal(bits(full[k][j:j + 1]), bits(first[k][:1])), (j, k)


def test_csr_mixed_view_counts(solver, csr):
    """2, 3, 5 and 17 views per point over 4 rotated poses; with more views than poses a point uses a pose again."""
    cnt = np.diff(csr["ptr"])
    assert set(cnt) == {2, 3, 5, 17}
    i17 = int(np.flatnonzero(cnt == 17)[0])
    assert len(set(csr["vp"][csr["ptr"][i17]:csr["ptr"][i17 + 1]])) == 4
    g = solver.triangulate(csr["poses"], csr["xy"], view_ptr=csr["ptr"], view_pose=csr["vp"])
    check_against_reference(g, csr["ref"], "csr")


def test_cam_K_path_is_bitwise_the_normalised_path(solver, stereo):
    """cam_K: (u - cx) / fx, (v - cy) / fy on the device, in Camera::pixel2camera's order (camera.cpp:21-25)."""
    Ks = np.stack([tr.K, tr.K + np.array([0.0, 0.0, 0.5, 0.0])])   # the second camera's own principal point
    px = stereo["px"]
    a = solver.triangulate(stereo["poses"], px, K=Ks)
    b = solver.triangulate(stereo["poses"], tr.pixel2camera(px, Ks[None, :, :]))
    assert same_bits(a, b)
    assert 0 < a["n_accepted"] < len(px)


def project(poses, pw):
    """Exact normalised coordinates of world points pw [n, 3] in every pose: [n, P, 2]."""
    m = np.asarray(poses).reshape(-1, 3, 4)
    y = np.einsum("pij,nj->npi", m[:, :, :3], pw) + m[None, :, :, 3]
    return y[:, :, :2] / y[:, :, 2:3]


def test_gates_and_T_out(solver):
    poses = tr.stereo_poses()
    gate = (2.0, 3.0, 80.0)   # pworld[1] <= 2, stereo depth limits (frontend_lego.cpp:133-136)
    pw = np.array([[1.0, 3.0, 20.0],     # y > y_max
                   [0.5, 0.2, 2.0],      # z <= z_min
                   [4.0, 1.0, 90.0],     # z > z_max
                   [1.0, 2.5, 1.0],      # y and z
                   [-2.0, 1.0, 10.0], [3.0, -1.5, 40.0], [0.3, 0.1, 79.0], [-8.0, 1.9, 33.0]])
    want = np.array([tr.F_Y, tr.F_Z, tr.F_Z, tr.F_Y | tr.F_Z, 0, 0, 0, 0], np.uint8)
    xy = project(poses, pw)
    c, s_ = np.cos(0.3), np.sin(0.3)
    T = np.array([c, 0, s_, 1.5, 0, 1, 0, -0.25, -s_, 0, c, 7.0])
    plain = solver.triangulate(poses, xy)
    g = solver.triangulate(poses, xy, gate=gate, T_out=T)
    r = tr.triangulate_ref(poses, xy.reshape(-1, 2), gate=gate, T_out=T)
    assert np.array_equal(plain["flags"], np.zeros(8, np.uint8))
    assert np.array_equal(g["flags"], want) and np.array_equal(r["flags"], want)
    assert g["n_accepted"] == 4 and plain["n_accepted"] == 8
    rej = want != 0
    assert np.array_equal(bits(g["pt"][rej]), bits(plain["pt"][rej]))   # a rejected point keeps its untransformed value
    Tm = T.reshape(3, 4)
    moved = plain["pt"][~rej] @ Tm[:, :3].T + Tm[:, 3]
    assert np.allclose(g["pt"][~rej], moved, rtol=1e-13, atol=0)
    assert np.allclose(g["pt"][~rej], pw[~rej] @ Tm[:, :3].T + Tm[:, 3], rtol=1e-9, atol=0)
    only_T = solver.triangulate(poses, xy, T_out=T)                     # no gate: every point is transformed
    assert np.array_equal(only_T["flags"], np.zeros(8, np.uint8))
    assert np.allclose(only_T["pt"], plain["pt"] @ Tm[:, :3].T + Tm[:, 3], rtol=1e-13, atol=0)


def test_degenerate_inputs(solver):
    """Ordinary inputs that strain the SVD: none may fault, hang or turn into a NaN where the reference has none."""
    sp = tr.stereo_poses()
    for xy in ([0.1, 0.2], [-0.4583, 0.0397], [0.2331, -0.3917]):   # two identical views: sigma2 ~ sigma3 ~ 0
        g = solver.triangulate(np.stack([sp[1], sp[1]]), np.array([xy, xy]))
        assert g["flags"][0] & tr.F_RATIO and g["n_accepted"] == 0
    g = solver.triangulate(sp, np.zeros((1, 2, 2)))                  # parallel rays: the point at infinity, v[3] = 0
    assert g["flags"][0] & tr.F_NONFINITE and g["n_accepted"] == 0
    rng = np.random.default_rng(5)                                   # exact correspondences: sigma3 ~ 1e-16 sigma0
    d = rng.uniform(3.0, 80.0, 130)
    pw = np.stack([rng.uniform(-0.5, 0.5, 130) * d, rng.uniform(-0.4, 0.4, 130) * d, d], 1)
    g = solver.triangulate(sp, project(sp, pw))
    assert np.array_equal(g["flags"], np.zeros(130, np.uint8)) and g["n_accepted"] == 130
    assert np.all(np.isfinite(g["sing_ratio"])) and g["sing_ratio"].max() < 1e-12
    assert np.allclose(g["pt"], pw, rtol=1e-9, atol=0)


def test_errors(solver):
    import lego_ba
    poses, xy, _ = tr.stereo_set()
    xy = xy[:4].reshape(-1, 2)
    bad = [dict(view_ptr=[0, 2, 3, 5], view_pose=[0, 1, 0, 0, 1]),        # a 1-view point
           dict(view_ptr=[0, 2, 4], view_pose=[0, 1, 0, 2]),              # pose index out of range
           dict(view_ptr=[0, 4, 2, 6], view_pose=[0, 1, 0, 1, 0, 1])]     # view_ptr decreases
    for kw in bad:
        with pytest.raises(lego_ba.LhError) as e:
            solver.triangulate(poses, xy, **kw)
        assert e.value.status == lego_ba.LH_E_BADARG
    a, r = lego_ba.LhTriInput(), lego_ba.LhTriResult()                    # a null pt
    flags = np.zeros(4, np.uint8)
    a.n_points, a.n_poses, a.sing_ratio_thr = 4, 2, 1e-3
    a.pose_Tcw, a.view_xy = poses.ctypes.data, xy.ctypes.data
    r.flags = flags.ctypes.data
    assert lego_ba.ba_lib().lh_triangulate(solver.h, C.byref(a), C.byref(r)) == lego_ba.LH_E_BADARG
    a.n_points = 0                                                        # nothing to do: LH_OK, even without outputs
    assert lego_ba.ba_lib().lh_triangulate(solver.h, C.byref(a), C.byref(r)) == lego_ba.LH_OK
    g = solver.triangulate(poses, np.zeros((0, 2)))
    assert g["pt"].shape == (0, 3) and g["n_accepted"] == 0
    assert solver.triangulate(poses, xy)["n_accepted"] >= 0              # the handle still works


def test_stereo_landmarks_is_lk_track_then_triangulate(solver):
    """One stereo frame (240 x 320, 300 keypoints and 8 on or past the borders, a horizontal shift as disparity):
    kp2 and success are bitwise lk_track's, pt and flags bitwise triangulate's on them, failed tracks carry bit 4."""
    rows, cols = 240, 320
    left, right = images.pair(rows, cols, shift=(-6.0, 0.0), seed=11)
    k1 = images.keypoints(rows, cols, 300, seed=11)
    poses = tr.stereo_poses()
    Ks = np.stack([tr.K, tr.K])
    c, s_ = np.cos(-0.2), np.sin(-0.2)
    T = np.array([c, 0, s_, 0.4, 0, 1, 0, 0.1, -s_, 0, c, -3.0])
    lk = solver.lk_track(left, right, k1, kp2_init=k1)
    st = solver.stereo_landmarks(left, right, k1, poses, K=Ks, kp_right_init=k1, T_out=T)
    assert np.array_equal(st["kp2"], lk["kp2"]) and np.array_equal(st["success"], lk["success"])
    ok = lk["success"]
    assert 0 < ok.sum() < len(ok)
    pairs = np.stack([k1, lk["kp2"]], 1).astype(np.float64)[ok]           # floats widened, as toVec2 does
    tri = solver.triangulate(poses, pairs, K=Ks, T_out=T)
    assert np.array_equal(st["flags"][ok], tri["flags"])
    assert np.array_equal(bits(st["pt"][ok]), bits(tri["pt"]))
    assert np.all(st["flags"][~ok] == tr.F_TRACK) and not np.any(st["pt"][~ok])
    assert st["n_accepted"] == tri["n_accepted"] == int(np.sum(st["flags"] == 0))
    assert not np.any(st["flags"][ok] & tr.F_TRACK)
