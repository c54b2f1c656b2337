"""CPU tests of lh_insert_keyframe's boundary (include/lego_ba.h): the ctypes mirrors of its two structs
against a compiled C program, field by field, and tests/keyframe_ref.py's NumPy chain against a literal loop over the
conditions of Frontend::TriangulateNewPoints.  No GPU call is made here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import keyframe_ref as kf
import klt_ref
import lego_ba
import track_ref as tk
import triangulate_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"lh_keyframe_input": "LhKeyframeInput", "lh_keyframe_result": "LhKeyframeResult"}


def layout_program():
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "lego_ba.h"', "int main(void) {"]
    for c_name, py_name in STRUCTS.items():
        lines.append(f'  printf("{c_name} %zu\\n", sizeof({c_name}));')
        for field, _ in getattr(lego_ba, py_name)._fields_:
            lines.append(f'  printf("{c_name}.{field} %zu\\n", offsetof({c_name}, {field}));')
    return "\n".join(lines + ["  return 0;", "}", ""])


def test_ctypes_layout_matches_header(tmp_path):
    c = tmp_path / "layout.c"
    c.write_text(layout_program())
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    for c_name, py_name in STRUCTS.items():
        cls = getattr(lego_ba, py_name)
        assert got[c_name] == C.sizeof(cls), c_name
        assert len(cls._fields_) == sum(k.startswith(c_name + ".") for k in got)
        for field, _ in cls._fields_:
            assert getattr(cls, field).offset == got[f"{c_name}.{field}"], (c_name, field)
    # the header's fields, in its order, are the mirror's: none is missing from the mirror
    hdr = open(os.path.join(ROOT, "include", "lego_ba.h")).read()
    for c_name, py_name in STRUCTS.items():
        body = re.sub(r"/\*.*?\*/", "", hdr.split(f"typedef struct {c_name} {{")[1].split(f"}} {c_name};")[0], flags=re.S)
        names = []
        for decl in body.split(";")[:-1]:
            for part in decl.split(","):
                names.append(part.replace("*", " ").split("[")[0].split()[-1])
        assert names == [f for f, _ in getattr(lego_ba, py_name)._fields_], c_name


def test_symbol_and_flag():
    assert "lh_insert_keyframe" in lego_ba.ABI_SYMBOLS and hasattr(lego_ba.ba_lib(), "lh_insert_keyframe")
    assert lego_ba.LH_TRI_HAS_POINT == kf.F_HAS_POINT == 32
    assert lego_ba.LH_TRI_HAS_POINT & (tr.F_NONFINITE | tr.F_RATIO | tr.F_Y | tr.F_Z | tr.F_TRACK) == 0


def test_reference_flags_against_the_literal_loop():
    """reference() on the keyframe scene: every class of feature occurs, and its flags, points and counts are the
    feature-by-feature loop's over the tracker's and the triangulation's own references."""
    sc = kf.scene()
    r = kf.call(kf.reference, sc)
    nh, m = len(sc["have_kp"]), r["n_new"]
    assert (r["n_candidates"], m) == (259, 40) and r["kp_right"].shape == (nh + m, 2)
    assert kf.call(kf.reference, sc, max_corners=150)["n_new"] == 88                 # 40 is the cap
    hp = np.concatenate([sc["have_point"].astype(bool), np.zeros(m, bool)])
    assert set(np.unique(r["flags"])) >= {0, 2, 4, 6, 16, 32} and r["n_right"] == 74
    # the parts again, by hand
    kl = np.concatenate([sc["have_kp"], r["kp_new"]])
    X = np.concatenate([sc["have_pts_w"], np.zeros((m, 3))])
    g = tk.guess(X, hp, kl, sc["pose"], sc["cam_pose"][1], sc["cam_K"][1])
    assert np.array_equal(g[~hp], kl[~hp]) and not np.array_equal(g[hp], kl[hp])
    t = klt_ref.track(sc["img_left"], sc["img_right"], kl, kp2_init=g)
    assert np.array_equal(tk.bits(t["kp2"]), tk.bits(r["kp_right"])) and np.array_equal(t["success"], r["success"])
    xy = np.stack([kl.astype(np.float64), t["kp2"].astype(np.float64)], 1)
    every = tr.triangulate_ref(sc["cam_pose"], xy, K=sc["cam_K"], gate=sc["gate"])   # also the features nobody triangulates
    flags = kf.literal_flags(t["success"], hp, every["flags"])
    assert np.array_equal(flags, r["flags"])
    tri = flags < 16
    assert np.array_equal(tk.bits(r["pt"][tri]), tk.bits(every["pt"][tri])) and not r["pt"][~tri].any()
    assert r["n_accepted"] == int(np.sum(flags == 0)) > 0
    # a feature with a point carries bit 5 alone whether or not it tracked
    assert np.all(r["flags"][hp] == 32) and (r["success"] & hp).sum() > 0


def test_reference_edge_scenes():
    sc = kf.scene()
    none = dict(have_kp=None, have_pts_w=None, have_point=None)
    r = kf.call(kf.reference, sc, max_corners=150, **none)
    assert (r["n_candidates"], r["n_new"]) == (444, 127) and not (r["flags"] == 32).any()
    assert kf.call(kf.reference, sc, min_distance=20.0, **none)["n_new"] == 34
    assert kf.call(kf.reference, sc, min_distance=20.0)["n_new"] == 28               # below the cap of 40
    flat = np.full((kf.ROWS, kf.COLS), 77, np.uint8)
    r = kf.call(kf.reference, sc, img_left=flat, img_right=flat, **none)
    assert (r["n_new"], r["n_candidates"], r["lambda_max"], r["n_right"], r["n_accepted"]) == (0, 0, 0.0, 0, 0)
    assert r["kp_right"].shape == (0, 2) and r["flags"].shape == (0,)
