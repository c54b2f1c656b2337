"""CPU tests of lh_track_frame's definition (include/lego_ba.h): the NumPy restatement of the guesses
and of the edge selection (tests/track_ref.py), k_track_guess's arithmetic (lego-slam_amd/csrc/lh_track.h, plain C++)
compiled for the host (tests/track_probe.cpp, -ffp-contract=off) against it bit for bit, and the layout of the two new
structs against their ctypes mirrors.  No compute call on the library is made here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lego_ba
import track_ref as tk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.array([517.3, 516.5, 81.5, 60.5])
C_, S_ = np.cos(0.3), np.sin(0.3)
EXTRINSICS = {
    "identity": tk.IDENTITY,
    "rotated_translated": np.array([C_, 0.0, S_, 0.12, 0.0, 1.0, 0.0, -0.05, -S_, 0.0, C_, 0.3]),
}
POSE = np.array([0.9998, -0.012, 0.016, 0.05, 0.0121, 0.9999, -0.004, -0.02, -0.0159, 0.0042, 0.9998, 0.11])


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return tk.host_library(tmp_path_factory.mktemp("track"))


def same_floats(a, b):
    """Bit for bit; a NaN (whose payload the definition leaves open) matches a NaN."""
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan)
    assert np.array_equal(tk.bits(a)[~nan], tk.bits(b)[~nan])


def random_case(seed, n=257):
    rng = np.random.default_rng(seed)
    kp1 = np.stack([rng.uniform(0, 163, n), rng.uniform(0, 121, n)], 1).astype(np.float32)
    z = rng.uniform(2, 60, n)
    X = np.stack([(kp1[:, 0] - K[2]) / K[0] * z, (kp1[:, 1] - K[3]) / K[1] * z, z], 1) + rng.normal(0, 0.05, (n, 3))
    hp = (rng.uniform(size=n) < 0.8).astype(np.uint8)
    return kp1, X, hp


@pytest.mark.parametrize("ext", list(EXTRINSICS))
def test_host_build_of_the_guess_matches_restatement_bitwise(host, ext):
    kp1, X, hp = random_case(1)
    X[5] = (1.0, 2.0, -7.5)                     # behind the camera: a finite pixel, mirrored through the centre
    hp[5] = 1
    E = EXTRINSICS[ext]
    for pose in (tk.IDENTITY, POSE):
        for has_point in (hp, None):
            r = tk.guess(X, has_point, kp1, pose, E, K)
            g = tk.host_guess(host, X, has_point, kp1, pose, E, K)
            assert r.dtype == np.float32 and r.shape == (len(kp1), 2)
            same_floats(g, r)
            assert np.isfinite(r).all()
            if has_point is not None:           # no point: kp1 passes through
                none = hp == 0
                assert 0 < none.sum() < len(hp)
                assert np.array_equal(tk.bits(r[none]), tk.bits(kp1[none]))
                assert not np.array_equal(r[~none], kp1[~none])


def test_guess_of_zero_depth_behind_the_camera_and_past_flt_max(host):
    """Identity pose and extrinsic, so that Pc is the point itself."""
    X = np.array([[1.0, 2.0, 0.0],              # Pc2 == 0: (+inf, +inf)
                  [-1.0, 0.0, 0.0],             #           (-inf, NaN)
                  [0.0, 0.0, 0.0],              #           (NaN, NaN)
                  [1.0, 1.0, -5.0],             # behind the camera
                  [1e38, 2.0, 1e-3],            # u = 5.2e43 > FLT_MAX: +inf; v finite
                  [-1e38, 2.0, 1e-3],           # -inf
                  [0.0, 0.0, 4.0],              # the principal point
                  [3.0, 3.0, 0.0]])             # no point: kp1, whatever the point is
    hp = np.array([1, 1, 1, 1, 1, 1, 1, 0], np.uint8)
    kp1 = np.arange(16, dtype=np.float32).reshape(8, 2)
    r = tk.guess(X, hp, kp1, tk.IDENTITY, tk.IDENTITY, K)
    same_floats(tk.host_guess(host, X, hp, kp1, tk.IDENTITY, tk.IDENTITY, K), r)
    assert r[0].tolist() == [np.inf, np.inf]
    assert r[1, 0] == -np.inf and np.isnan(r[1, 1]) and np.isnan(r[2]).all()
    assert r[3].tolist() == [np.float32(K[0] * 1.0 / -5.0 + K[2]), np.float32(K[1] * 1.0 / -5.0 + K[3])]
    assert r[4, 0] == np.inf and r[5, 0] == -np.inf and np.isfinite(r[4:6, 1]).all()
    assert K[0] * 1e38 / 1e-3 < np.finfo(np.float64).max           # the double is finite: the conversion overflows
    assert r[6].tolist() == [np.float32(K[2]), np.float32(K[3])]
    assert np.array_equal(r[7], kp1[7])
    # the largest doubles that still round to FLT_MAX, and the first that does not (round to nearest even)
    fmax = float(np.finfo(np.float32).max)
    edge = np.array([[fmax, 0.0, 1.0], [fmax * (1 + 2.0 ** -26), 0.0, 1.0], [fmax * (1 + 2.0 ** -24), 0.0, 1.0]])
    unit = np.array([1.0, 1.0, 0.0, 0.0])
    r = tk.guess(edge, None, np.zeros((3, 2), np.float32), tk.IDENTITY, tk.IDENTITY, unit)
    same_floats(tk.host_guess(host, edge, None, np.zeros((3, 2), np.float32), tk.IDENTITY, tk.IDENTITY, unit), r)
    assert r[:, 0].tolist() == [np.float32(fmax), np.float32(fmax), np.inf]


def test_guess_is_the_projection():
    """Against the matrix form E * T (the reference's order) in float64: equal to rounding."""
    kp1, X, _ = random_case(2)
    E, T = (np.vstack([a.reshape(3, 4), [0, 0, 0, 1]]) for a in (EXTRINSICS["rotated_translated"], POSE))
    Pc = (E @ T @ np.hstack([X, np.ones((len(X), 1))]).T).T
    uv = np.stack([K[0] * Pc[:, 0] / Pc[:, 2] + K[2], K[1] * Pc[:, 1] / Pc[:, 2] + K[3]], 1)
    g = tk.guess(X, None, kp1, POSE, EXTRINSICS["rotated_translated"], K)
    assert np.abs(g - uv).max() <= 2.0 ** -23 * np.abs(uv).max() + 1e-9


def test_select_keeps_tracked_features_with_a_point_in_order():
    ok = np.array([1, 0, 1, 1, 0, 1], bool)
    hp = np.array([1, 1, 0, 1, 0, 1], np.uint8)
    kp2 = (np.arange(12, dtype=np.float32) + np.float32(0.1)).reshape(6, 2)
    X = np.arange(18, dtype=np.float64).reshape(6, 3)
    s = tk.select(ok, hp, kp2, X)
    assert s["idx"].tolist() == [0, 3, 5]
    assert np.array_equal(s["pts"], X[[0, 3, 5]])
    assert s["uv"].dtype == np.float64 and np.array_equal(s["uv"], kp2[[0, 3, 5]].astype(np.float64))
    assert tk.select(ok, None, kp2, X)["idx"].tolist() == [0, 2, 3, 5]
    assert len(tk.select(np.zeros(6, bool), hp, kp2, X)["idx"]) == 0
    fb = tk.frame_batch(s, POSE, K)
    assert fb["obs_ptr"].tolist() == [0, 3] and fb["pose_Tcw"].shape == (1, 12)


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "lego_ba.h"
#define P(s, f) printf(#s "." #f " %zu\n", offsetof(s, f));
int main(void) {
  printf("lh_track_input %zu\n", sizeof(lh_track_input));
  printf("lh_track_result %zu\n", sizeof(lh_track_result));
  P(lh_track_input, klt) P(lh_track_input, pts_w) P(lh_track_input, has_point) P(lh_track_input, pose_Tcw)
  P(lh_track_input, cam_ext) P(lh_track_input, K)
  P(lh_track_result, kp2) P(lh_track_result, success) P(lh_track_result, pose_Tcw) P(lh_track_result, is_outlier)
  P(lh_track_result, edge_chi2) P(lh_track_result, n_tracked) P(lh_track_result, n_edges) P(lh_track_result, n_inliers)
  P(lh_track_result, iterations) P(lh_track_result, time_ms)
  printf("abi %d\n", LH_ABI_VERSION);
  return 0;
}
"""


def test_track_struct_layout_matches_header(tmp_path):
    c = tmp_path / "layout.c"
    c.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    cls = {"lh_track_input": lego_ba.LhTrackInput, "lh_track_result": lego_ba.LhTrackResult}
    assert got.pop("abi") == lego_ba.LH_ABI_VERSION == 5
    n_fields = 0
    for key, v in got.items():
        if "." in key:
            s, f = key.split(".")
            assert getattr(cls[s], f).offset == v, key
            n_fields += 1
        else:
            assert C.sizeof(cls[key]) == v, key
    assert n_fields == len(lego_ba.LhTrackInput._fields_) + len(lego_ba.LhTrackResult._fields_)


def test_track_frame_is_declared_and_exported():
    assert "lh_track_frame" in lego_ba.ABI_SYMBOLS
    assert "lh_track_frame" in open(os.path.join(ROOT, "include", "lego_ba.h")).read()
    assert hasattr(lego_ba.ba_lib(), "lh_track_frame")
