"""CPU test of the frontend's arena layouts (lego-slam_amd/csrc/lh_frontend_layout.h): tests/frontend_layout_probe.cpp,
built with plain g++, prints every offset of FramesLayout, TrackLayout, KeyframeLayout and TriOut; they must equal the
formulas the entry points computed inline before the layouts became structs (restated below as they stood, the
keyframe arena's unpadded segments included), and every segment must be aligned to its element type, end before its
successor begins and lie inside the arena.  No number here is measured."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = I64 = 8
F32 = I32 = 4

TRACK_N = [0, 1, 2, 3, 5, 63, 64, 65, 257]
KEYFRAME_LISTS = [(0, 7), (1, 7), (63, 7), (64, 7), (65, 7), (257, 7), (250, 40)]   # test_keyframe_gpu.py::test_list_sizes
FRAMES = [(F, O) for F in (1, 3) for O in (0, 1, 7, 40)]


def al(b):
    return (b + 15) & ~15


def frames_formulas(F, O, has_flag):
    """lh_estimate_pose's chains"""
    i_ptr = 0
    i_pose = al(I64 * (F + 1))
    i_pts = i_pose + al(F64 * 12 * F)
    i_uv = i_pts + al(F64 * 3 * O)
    i_flag = i_uv + al(F64 * 2 * O)
    i_end = i_flag + (al(O) if has_flag else 0)
    o_pose = 0
    o_rchi2 = al(F64 * 12 * F)
    o_iters = o_rchi2 + al(F64 * O)
    o_inl = o_iters + al(I32 * F)
    o_flag = o_inl + al(I32 * F)
    o_end = o_flag + al(O)
    return {k: v for k, v in locals().items() if k[:2] in ("i_", "o_")}


def track_formulas(N, _, has_point):
    """lh_track_frame's chains"""
    i_pose = 0
    i_pts = al(F64 * 12)
    i_kp1 = i_pts + al(F64 * 3 * N)
    i_hp = i_kp1 + al(F32 * 2 * N)
    i_end = i_hp + (al(N) if has_point else 0)
    o_pose = 0
    o_cnt = al(F64 * 12)
    o_kp2 = o_cnt + al(I32 * 4)
    o_succ = o_kp2 + al(F32 * 2 * N)
    o_idx = o_succ + al(N)
    o_flag = o_idx + al(I32 * N)
    o_chi = o_flag + al(N)
    o_end = o_chi + al(F64 * N)
    w_ptr = 0
    w_pts = al(I64 * 2)
    w_uv = w_pts + al(F64 * 3 * N)
    w_end = w_uv + al(F64 * 2 * N)
    return {k: v for k, v in locals().items() if k[:2] in ("i_", "o_", "w_")}


def keyframe_formulas(NH, mc, has_point):
    """lh_insert_keyframe's chains: i_K, i_pts, i_up and i_end are not padded; o_lam = 16, o_pt = 32"""
    CAP = NH + mc
    i_cam = 0
    i_K = F64 * 24
    i_pts = i_K + F64 * 8
    i_hp = i_pts + al(F64 * 3 * NH)
    i_kl = i_hp + (al(NH) if has_point else 0)
    i_up = i_kl + F32 * 2 * NH
    i_end = i_kl + F32 * 2 * CAP
    o_cnt = 0
    o_lam = I32 * 4
    o_pt = 32
    o_kpr = o_pt + al(F64 * 3 * CAP)
    o_new = o_kpr + al(F32 * 2 * CAP)
    o_succ = o_new + al(F32 * 2 * mc)
    o_flag = o_succ + al(CAP)
    o_end = o_flag + al(CAP)
    return {k: v for k, v in locals().items() if k[:2] in ("i_", "o_")}


def tri_formulas(n, _, __):
    """tri_outputs' chain; pt is the arena's head"""
    o_pt = 0
    o_ratio = F64 * 3 * n
    o_flag = o_ratio + F64 * n
    o_end = o_flag + n
    return {k: v for k, v in locals().items() if k[:2] == "o_"}


def frames_segments(F, O, has_flag):
    """per arena: its end's name, then (segment, bytes, element size) in order"""
    return [("i_end", [("i_ptr", I64 * (F + 1), I64), ("i_pose", F64 * 12 * F, F64), ("i_pts", F64 * 3 * O, F64),
                       ("i_uv", F64 * 2 * O, F64), ("i_flag", O if has_flag else 0, 1)]),
            ("o_end", [("o_pose", F64 * 12 * F, F64), ("o_rchi2", F64 * O, F64), ("o_iters", I32 * F, I32),
                       ("o_inl", I32 * F, I32), ("o_flag", O, 1)])]


def track_segments(N, _, has_point):
    return [("i_end", [("i_pose", F64 * 12, F64), ("i_pts", F64 * 3 * N, F64), ("i_kp1", F32 * 2 * N, F32),
                       ("i_hp", N if has_point else 0, 1)]),
            ("o_end", [("o_pose", F64 * 12, F64), ("o_cnt", I32 * 4, I32), ("o_kp2", F32 * 2 * N, F32), ("o_succ", N, 1),
                       ("o_idx", I32 * N, I32), ("o_flag", N, 1), ("o_chi", F64 * N, F64)]),
            ("w_end", [("w_ptr", I64 * 2, I64), ("w_pts", F64 * 3 * N, F64), ("w_uv", F64 * 2 * N, F64)])]


def keyframe_segments(NH, mc, has_point):
    CAP = NH + mc
    return [("i_end", [("i_cam", F64 * 24, F64), ("i_K", F64 * 8, F64), ("i_pts", F64 * 3 * NH, F64),
                       ("i_hp", NH if has_point else 0, 1), ("i_kl", F32 * 2 * CAP, F32)]),
            ("i_up", [("i_kl", F32 * 2 * NH, F32)]),          # the upload: up to the end of have_kp, the list's head
            ("o_end", [("o_cnt", I32 * 4, I32), ("o_lam", F64, F64), ("o_pt", F64 * 3 * CAP, F64),
                       ("o_kpr", F32 * 2 * CAP, F32), ("o_new", F32 * 2 * mc, F32), ("o_succ", CAP, 1), ("o_flag", CAP, 1)])]


def tri_segments(n, _, __):
    return [("o_end", [("o_pt", F64 * 3 * n, F64), ("o_ratio", F64 * n, F64), ("o_flag", n, 1)])]


KINDS = {"frames": (frames_formulas, frames_segments), "track": (track_formulas, track_segments),
         "keyframe": (keyframe_formulas, keyframe_segments), "tri": (tri_formulas, tri_segments)}


def build_probe(build_dir, *flags):
    exe = os.path.join(str(build_dir), "frontend_layout_probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I",
                           os.path.join(ROOT, "lego-slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "frontend_layout_probe.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """{(kind, count, count, flag): {name: offset}} as the probe prints them"""
    got = {}
    for line in subprocess.check_output([build_probe(tmp_path_factory.mktemp("layout"))], text=True).splitlines():
        kind, a, b, flag, *fields = line.split()
        got[(kind, int(a), int(b), int(flag))] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    return got


def test_probe_prints_every_case(printed):
    want = {("track", n, 0, f) for n in TRACK_N for f in (0, 1)}
    want |= {("keyframe", nh, mc, f) for nh, mc in KEYFRAME_LISTS for f in (0, 1)}
    want |= {("frames", F, O, f) for F, O in FRAMES for f in (0, 1)}
    want |= {("tri", n, 0, 0) for n in TRACK_N}
    assert set(printed) == want and len(want) == 18 + 14 + 16 + 9


def test_offsets_equal_the_inline_formulas(printed):
    n = 0
    for (kind, a, b, flag), got in printed.items():
        want = KINDS[kind][0](a, b, flag)
        assert got == want, (kind, a, b, flag)
        n += len(want)
    assert n == 18 * 17 + 14 * 15 + 16 * 12 + 9 * 4      # every offset of every struct


def test_segments_are_aligned_disjoint_and_inside(printed):
    for (kind, a, b, flag), got in printed.items():
        covered = set()
        for end, segs in KINDS[kind][1](a, b, flag):
            for (name, nbytes, elem), nxt in zip(segs, segs[1:] + [None]):
                at = got[name]
                assert at % elem == 0, (kind, a, b, flag, name)
                assert at + nbytes <= (got[nxt[0]] if nxt else got[end]), (kind, a, b, flag, name)
                covered.add(name)
            covered.add(end)
        assert covered == set(got), (kind, a, b, flag)        # no offset of the struct is left unchecked
