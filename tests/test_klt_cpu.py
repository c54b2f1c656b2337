"""CPU tests of lh_klt_track's definition (include/lego_ba.h): the NumPy restatement
(tests/klt_ref.py) on scenes with a known flow, and the kernels' arithmetic (lego-slam_amd/csrc/lh_klt.h, plain C++)
compiled for the host (tests/klt_probe.cpp, -ffp-contract=off) against it, bit for bit, on the GPU suite's cases.
OpenCV is not available here: parity with cv::calcOpticalFlowPyrLK itself is not tested."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import images
import klt_ref as kr
import lego_ba
import test_klt_gpu as cases
from test_lk import true_flow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return kr.host_library(tmp_path_factory.mktemp("klt"))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_host_build_of_the_kernel_arithmetic_matches_restatement_bitwise(host, name):
    """kp2 and success of the whole tracker, on every case of the GPU suite (each reaches the exits it is there for)."""
    r = cases.coverage(name)
    sc, guess, kw = cases.CASES[name]
    i1, i2, k1 = cases.scene(**sc)
    g = kr.host_track(host, i1, i2, k1, cases.guess_of(k1, guess), **kw)
    assert np.array_equal(g["success"], r["success"])
    assert np.array_equal(kr.bits(g["kp2"]), kr.bits(r["kp2"]))


def test_host_build_on_strided_rows_and_nonfinite_points(host):
    i1, i2, k1 = cases.scene()
    b1, b2 = np.full((cases.ROWS, 200), 255, np.uint8), np.full((cases.ROWS, 200), 255, np.uint8)
    b1[:, :cases.COLS], b2[:, :cases.COLS] = i1, i2
    r = cases.reference("odd_levels")
    g = kr.host_track(host, b1[:, :cases.COLS], b2[:, :cases.COLS], k1)
    assert np.array_equal(kr.bits(g["kp2"]), kr.bits(r["kp2"])) and np.array_equal(g["success"], r["success"])
    kn = k1.copy()
    kn[3] = (np.nan, 20.0)
    kn[5] = (30.0, np.inf)
    kn[6] = (-1e30, 1e30)
    r, g = kr.track(i1, i2, kn), kr.host_track(host, i1, i2, kn)
    assert not r["success"][[3, 5, 6]].any() and np.array_equal(g["success"], r["success"])
    assert np.array_equal(g["kp2"], r["kp2"], equal_nan=True)


@pytest.mark.parametrize("rows,cols", [(121, 163), (81, 47), (17, 13)])
def test_pyramid_matches_restatement_on_random_bytes(host, rows, cols):
    """163 x 121, 47 x 81 and 13 x 17 (cols x rows): odd sizes, the REFLECT_101 folds, every level that exists."""
    img = np.random.default_rng(rows * cols).integers(0, 256, (rows, cols), dtype=np.uint8)
    levels = kr.pyramid(img, 3)
    assert len(levels) == host.klt_level_count(cols, rows, 3) == {163: 4, 47: 3, 13: 1}[cols]
    assert host.klt_level_count(cols, rows, 1) == min(len(levels), 2) and host.klt_level_count(cols, rows, 0) == 1
    for a, b in zip(levels, levels[1:]):
        assert b.shape == ((a.shape[0] + 1) // 2, (a.shape[1] + 1) // 2) and min(b.shape) > 11
        assert np.array_equal(kr.host_pyr_down(host, a), b)
    last = levels[-1].shape
    assert len(levels) == 4 or min((last[0] + 1) // 2, (last[1] + 1) // 2) <= 11
    assert np.array_equal(kr.host_pyr_down(host, img), kr.pyr_down(img))   # one level down, built or not
    padded = np.full((rows, cols + 9), 255, np.uint8)
    padded[:, :cols] = img
    assert np.array_equal(kr.host_pyr_down(host, padded[:, :cols]), kr.pyr_down(img))


def test_pyr_down_of_a_constant_and_of_an_impulse():
    """Known answers: the weights sum to 256, and an impulse at an even pixel spreads as w w^T."""
    assert np.all(kr.pyr_down(np.full((13, 18), 201, np.uint8)) == 201)
    img = np.zeros((21, 21), np.uint8)
    img[10, 10] = 255
    out = kr.pyr_down(img).astype(int)
    w = np.array([1, 6, 1])
    assert np.array_equal(out[4:7, 4:7], (255 * np.outer(w, w) + 128) >> 8) and out.sum() == out[4:7, 4:7].sum()


@pytest.mark.parametrize("shift", [(2.3, -1.7), (9.6, 4.2)])
def test_restatement_tracks_a_moved_texture(shift):
    """images.pair(240, 320), the textured inner third of the points as test_lk.py picks them, the reference's call
    (has_initial with kp2 = kp1).  Measured here: median 0.037 / 0.053 px, 90th percentile 0.073 / 0.074 px, all 83
    picked points tracked."""
    rows, cols = 240, 320
    i1, i2 = images.pair(rows, cols, shift=shift, seed=3)
    k1 = images.keypoints(rows, cols, 300, seed=3, border=False)
    inner = (k1[:, 0] > 20) & (k1[:, 0] < cols - 20) & (k1[:, 1] > 20) & (k1[:, 1] < rows - 20)
    c = images.cornerness(i1, k1)
    inner &= c >= np.percentile(c[inner], 67)
    r = kr.track(i1, i2, k1, kp2_init=k1)
    err = np.linalg.norm(r["kp2"] - k1 - true_flow(k1, shift, 3), axis=1)
    good = r["success"] & inner
    print(f"shift {shift}: median {np.median(err[good]):.4f} p90 {np.percentile(err[good], 90):.4f} "
          f"tracked {good.sum()} of {inner.sum()}")
    assert good.sum() > 0.9 * inner.sum()
    assert np.median(err[good]) < 0.1 and np.percentile(err[good], 90) < 0.25


def test_flat_image_fails_everywhere_and_keeps_the_guess(host):
    img = np.full((120, 160), 77, np.uint8)
    k1 = images.keypoints(120, 160, 20, seed=1)
    for init in (None, k1 + np.float32(1.25)):
        r = kr.track(img, img, k1, kp2_init=init)
        assert not r["success"].any() and np.array_equal(r["kp2"], k1 if init is None else init)
        assert set(np.unique(r["exits"])) <= {kr.X_MIN_EIG, kr.X_RANGE_P}
        g = kr.host_track(host, img, img, k1, init)
        assert not g["success"].any() and np.array_equal(kr.bits(g["kp2"]), kr.bits(r["kp2"]))


def test_header_declares_the_entry_points():
    """Additions only: the two calls are declared, bound and exported; the ABI version stays 5."""
    hdr = open(os.path.join(ROOT, "include", "lego_ba.h")).read()
    assert "int lh_klt_track(lh_handle *h, const lh_klt_input *in, lh_lk_result *out);" in hdr
    assert "int lh_klt_stereo_landmarks(lh_handle *h, const lh_klt_stereo_input *in, lh_stereo_result *out);" in hdr
    assert "#define LH_ABI_VERSION 5" in hdr
    lib = lego_ba.ba_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", lego_ba.BA_LIB], capture_output=True, text=True).stdout
    for sym in ("lh_klt_track", "lh_klt_stereo_landmarks"):
        assert sym in lego_ba.ABI_SYMBOLS and hasattr(lib, sym)
        assert f" T {sym}\n" in out
    src = open(os.path.join(ROOT, "lego-slam_amd", "csrc", "lh_klt.hip")).read()
    for k in ("k_klt_pyr", "k_klt_track"):
        assert k in src
    res = open(os.path.join(ROOT, "lego-slam_amd", "Makefile")).read()
    assert "$(LIBDIR)/lh_klt.o" in res.split("KERNEL_OBJS =")[1].split("\n")[0]   # resource_check covers the kernels


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "lego_ba.h"
#define P(s, f) printf(#s "." #f " %zu\n", offsetof(s, f));
int main(void) {
  printf("lh_klt_input %zu\n", sizeof(lh_klt_input));
  printf("lh_klt_stereo_input %zu\n", sizeof(lh_klt_stereo_input));
  P(lh_klt_input, cols) P(lh_klt_input, rows) P(lh_klt_input, step) P(lh_klt_input, img1) P(lh_klt_input, img2)
  P(lh_klt_input, n_points) P(lh_klt_input, kp1) P(lh_klt_input, has_initial) P(lh_klt_input, max_level)
  P(lh_klt_input, max_iters) P(lh_klt_input, epsilon) P(lh_klt_input, min_eig_threshold)
  P(lh_klt_stereo_input, klt) P(lh_klt_stereo_input, pose_Tcw) P(lh_klt_stereo_input, cam_K)
  P(lh_klt_stereo_input, sing_ratio_thr) P(lh_klt_stereo_input, gate) P(lh_klt_stereo_input, y_max)
  P(lh_klt_stereo_input, z_min) P(lh_klt_stereo_input, z_max) P(lh_klt_stereo_input, T_out)
  return 0;
}
"""


def test_ctypes_struct_layout_matches_header(tmp_path):
    c = tmp_path / "layout.c"
    c.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    cls = {"lh_klt_input": lego_ba.LhKltInput, "lh_klt_stereo_input": lego_ba.LhKltStereoInput}
    seen = 0
    for key, v in got.items():
        if "." in key:
            s, f = key.split(".")
            assert getattr(cls[s], f).offset == int(v), key
            seen += 1
        else:
            assert C.sizeof(cls[key]) == int(v), key
    assert seen == sum(len(k._fields_) for k in cls.values())
    names = [f[0] for f in lego_ba.LhKltStereoInput._fields_[1:]]
    assert names == [f[0] for f in lego_ba.LhStereoInput._fields_[1:]]   # lh_stereo_input's fields after .lk
