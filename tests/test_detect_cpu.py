"""CPU tests of lh_detect_features' definition (include/lego_ba.h): the NumPy restatement
(tests/gftt_ref.py) on a hand-made image, and the kernels' arithmetic (lego-slam_amd/csrc/lh_gftt.h, plain C++)
compiled for the host (tests/gftt_probe.cpp) against it, bit for bit.  OpenCV is not available here: parity with
cv::goodFeaturesToTrack itself is not tested."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import gftt_ref as gr
import images
import lego_ba

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return gr.host_library(tmp_path_factory.mktemp("gftt"))


def test_isolated_square_returns_its_four_corners():
    """(a) One bright square on a dark ground: four candidates, the square's corner pixels, all of one lambda, in
    descending raster order (the tie-break); tests/golden/detect_square.json records them."""
    want = json.load(open(os.path.join(gr.GOLDEN, "detect_square.json")))
    img = gr.square(want["rows"], want["cols"])
    x0, x1, y0, y1 = want["square_x0"], want["square_x1"], want["square_y0"], want["square_y1"]
    assert np.all(img[y0:y1 + 1, x0:x1 + 1] == 220) and np.sum(img == 220) == (x1 - x0 + 1) * (y1 - y0 + 1)
    r = gr.detect_ref(img, max_corners=0, min_distance=want["min_distance"])
    assert r["kp"].tolist() == want["kp"] and r["n_candidates"] == 4
    assert sorted(want["kp"]) == sorted([[x, y] for x in (float(x0), float(x1)) for y in (float(y0), float(y1))])
    assert r["response"].tolist() == want["response"] and r["lambda_max"] == want["response"][0]
    lam = r["eig"]
    for x, y in want["kp"]:   # each is the maximum of its 3x3 neighbourhood, and nothing else in the image is
        x, y = int(x), int(y)
        assert lam[y, x] == lam[y - 1:y + 2, x - 1:x + 2].max()
    assert gr.detect_ref(img, max_corners=2, min_distance=3.0)["kp"].tolist() == want["kp"][:2]
    # the corners are 7 apart along x and 5 along y.  min_distance 7: (x0, y1) is exactly 7 away and stays (the test
    # is <), the two upper corners fall; 7.5: (x0, y1) falls too, and (x0, y0), sqrt(74) from the first, stays
    assert gr.detect_ref(img, max_corners=0, min_distance=7.0)["kp"].tolist() == [want["kp"][0], want["kp"][1]]
    assert gr.detect_ref(img, max_corners=0, min_distance=7.5)["kp"].tolist() == [want["kp"][0], want["kp"][3]]
    assert gr.detect_ref(img, max_corners=0, min_distance=9.0)["kp"].tolist() == [want["kp"][0]]


@pytest.mark.parametrize("shape,step", [((37, 61), 61), ((48, 64), 80), ((3, 3), 3)])
def test_host_build_of_the_kernel_arithmetic_matches_reference_bitwise(host, shape, step):
    """(b) lambda, every pixel, bit for bit: the per-pixel definition (lh_gftt_lambda_at) and the two-pass order."""
    for img in (images.pair(*shape, seed=5)[0], gr.noise(*shape, seed=6)):
        img = gr.strided(img, step)
        want = gr.eig_image(img)
        assert np.array_equal(bits(gr.host_eig(host, img, direct=True)), bits(want))
        assert np.array_equal(bits(gr.host_eig(host, img)), bits(want))
        assert want.max() > 0 or shape == (3, 3)


def test_lambda_extremes(host):
    """The largest gradients an 8-bit image has (a checker of 0 / 255 columns, a step edge, a lone pixel)."""
    chk = np.zeros((9, 11), np.uint8)
    chk[:, ::2] = 255
    edge = np.zeros((9, 11), np.uint8)
    edge[:, 5:] = 255
    dot = np.zeros((9, 11), np.uint8)
    dot[4, 5] = 255
    for img in (chk, chk.T.copy(), edge, edge.T.copy(), dot, np.full((9, 11), 255, np.uint8)):
        assert np.array_equal(bits(gr.host_eig(host, img, direct=True)), bits(gr.eig_image(img)))
    gx, _ = gr.gradients(edge)
    assert np.abs(gx).max() == 1020


def test_box_rounding_on_half_integers(host):
    """(c) [rint(p - w), rint(p + w)], round half to even, float32: p - 10 = 4.5 -> 4, 5.5 -> 6; negative; past
    the image; not a number."""
    cols, rows = 61, 37
    cases = [(14.5, 15.5, 10.0), (15.5, 14.5, 10.0), (3.5, 2.5, 10.0), (-4.5, -11.0, 10.0), (-10.5, -11.5, 10.0),
             (70.5, 46.5, 10.0), (71.5, 5.0, 10.0), (5.0, 47.6, 10.0), (30.0, 18.0, 0.5), (30.5, 18.5, 0.0),
             (float("nan"), 5.0, 10.0), (1e9, 5.0, 10.0), (30.25, 18.75, 100.0), (16777217.0, 3.0, 10.0)]
    for px, py, w in cases:
        out = np.zeros(4, np.int32)
        host.gftt_box(px, py, w, cols, rows, out.ctypes.data)
        bx, by = gr.box_axis(px, w, cols), gr.box_axis(py, w, rows)
        for got, want in ((out[:2], bx), (out[2:], by)):
            assert (got[0] > got[1]) if want is None else (tuple(got) == want), (px, py, w)
    assert gr.box_axis(14.5, 10.0, cols) == (4, 24) and gr.box_axis(15.5, 10.0, cols) == (6, 26)   # half to even
    assert gr.box_axis(-4.5, 10.0, cols) == (0, 6) and gr.box_axis(-10.5, 10.0, cols) == (0, 0)   # rint(-0.5) = -0
    assert gr.box_axis(-11.5, 10.0, cols) is None
    assert gr.box_axis(70.5, 10.0, cols) == (60, 60) and gr.box_axis(71.5, 10.0, cols) is None    # rint(61.5) = 62


def test_order_preserving_key(host):
    v = [-3.5, -1e-9, 0.0, 1e-300, 1.0, 2880000.0, 1.9e7]
    for a in v:
        assert host.gftt_key_roundtrip(a) == a
    for a, b in zip(v, v[1:]):
        assert host.gftt_key_less(a, b) == 1 and host.gftt_key_less(b, a) == 0


def test_tied_image_depends_on_the_tie_break():
    """The GPU suite's tie case, on the reference alone: many candidates, few distinct lambdas, and the first 8
    corners change when ties go to the smaller index instead."""
    img = gr.tiled_ties()
    lam = gr.eig_image(img)
    idx, _ = gr.candidates(lam, gr.allowed(img.shape), 0.01)
    vals = lam.ravel()[idx]
    assert len(idx) > 150 and len(np.unique(vals)) < 20
    other = idx[np.lexsort((idx, -vals))]
    assert gr.select(idx, img.shape[1], 7.0, 8).tolist() != gr.select(other, img.shape[1], 7.0, 8).tolist()


@pytest.mark.parametrize("kw", [dict(), dict(min_distance=3.0, max_corners=0), dict(min_distance=7.5, max_corners=8),
                                dict(min_distance=0.5, max_corners=0), dict(min_distance=0.5, max_corners=8)])
def test_host_detector_matches_reference(host, kw):
    """The whole definition a second time, in C++ on the kernels' helpers (std::sort, a cell grid): candidates,
    order, selection, with exclusion boxes and a mask."""
    img = gr.noise(45, 67, seed=2)
    ex = np.array([[14.5, 15.5], [-3.0, 40.0], [66.0, 2.0]], np.float32)
    mask = np.ones(img.shape, np.uint8)
    mask[20:30, 30:50] = 0
    for im in (img, gr.tiled_ties()):
        r, g = gr.detect_ref(im, exclude=ex, mask=mask, **kw), gr.host_detect(host, im, exclude=ex, mask=mask, **kw)
        assert np.array_equal(g["kp"], r["kp"]) and g["n_corners"] == r["n_corners"] > 0
        assert g["n_candidates"] == r["n_candidates"] and g["lambda_max"] == r["lambda_max"]


def test_header_declares_the_entry_point():
    """(d) Additions only: lh_detect_features is declared, bound and exported; the ABI version stays 5; the ctypes
    structs have the header's layout."""
    hdr = open(os.path.join(ROOT, "include", "lego_ba.h")).read()
    assert "int lh_detect_features(lh_handle *h, const lh_detect_input *in, lh_detect_result *out);" in hdr
    assert "#define LH_ABI_VERSION 5" in hdr
    lib = lego_ba.ba_lib()
    assert "lh_detect_features" in lego_ba.ABI_SYMBOLS and hasattr(lib, "lh_detect_features")
    out = subprocess.run(["nm", "-D", "--defined-only", lego_ba.BA_LIB], capture_output=True, text=True).stdout
    assert " T lh_detect_features\n" in out
    src = open(os.path.join(ROOT, "lego-slam_amd", "csrc", "lh_gftt.hip")).read()
    for k in ("k_gftt_eig", "k_gftt_cand", "k_gftt_round", "k_gftt_rank"):
        assert k in src


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "lego_ba.h"
#define P(s, f) printf(#s "." #f " %zu\n", offsetof(s, f));
int main(void) {
  printf("lh_detect_input %zu\n", sizeof(lh_detect_input));
  printf("lh_detect_result %zu\n", sizeof(lh_detect_result));
  P(lh_detect_input, cols) P(lh_detect_input, rows) P(lh_detect_input, step) P(lh_detect_input, img)
  P(lh_detect_input, mask) P(lh_detect_input, mask_step) P(lh_detect_input, n_exclude) P(lh_detect_input, exclude_pt)
  P(lh_detect_input, exclude_half) P(lh_detect_input, max_corners) P(lh_detect_input, quality_level)
  P(lh_detect_input, min_distance)
  P(lh_detect_result, kp) P(lh_detect_result, kp_capacity) P(lh_detect_result, response) P(lh_detect_result, eig)
  P(lh_detect_result, n_corners) P(lh_detect_result, n_candidates) P(lh_detect_result, lambda_max)
  P(lh_detect_result, time_ms)
  return 0;
}
"""


def test_ctypes_struct_layout_matches_header(tmp_path):
    c = tmp_path / "layout.c"
    c.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    cls = {"lh_detect_input": lego_ba.LhDetectInput, "lh_detect_result": lego_ba.LhDetectResult}
    seen = 0
    for key, v in got.items():
        if "." in key:
            s, f = key.split(".")
            assert getattr(cls[s], f).offset == int(v), key
            seen += 1
        else:
            assert C.sizeof(cls[key]) == int(v), key
    assert seen == sum(len(k._fields_) for k in cls.values())
