"""The windows of the reduced-system tests (tests/test_lin_ref_cpu.py, tests/test_lin_system_gpu.py): small
windows chosen for the planner shapes they reach (asserted from plan_window on the CPU) and for their conditioning."""
import numpy as np

import lego_ba
import windows


def _gen(fixed=(0,), cams=0, **kw):
    kw = dict(dict(windows.STABLE, outlier_frac=0.0), **kw)
    w = lego_ba.generate_window(**kw)
    if cams:
        w = windows.multi_camera(w, cams)
    f = np.zeros(w["n_poses"], np.uint8)
    f[list(fixed)] = 1
    w["pose_fixed"] = f
    return w


_ALLT = dict(P=16, L=96, k=2, k_max=16, pose_mode=1, seed=1)
_OUTL = dict(P=10, L=120, k=2, k_max=10, pose_mode=1, seed=2)

_ALLT_SHAPES = dict(T={1, 2, 3, 4, 5, 6}, U={2, 3, 5, 7, 8, 9, 10, 11, 12, 13, 15, 16}, lg={1, 2, 3, 4},
                    n_lm={1, 2, 3, 4}, sb={1, 2})
_OUTL_SHAPES = dict(T={1, 2, 3, 4}, U={2, 4, 5, 7, 8, 9, 10}, lg={1, 2, 3, 4}, n_lm={1, 2, 3, 4, 5, 6, 8},
                    sb={1, 2, 3, 4})

# id: (window, chunk_landmarks, solver options, the planner shapes the case claims: chunk T and U, sub-batch lg and
#      n_lm, sub-batches per chunk -- each the exact set plan_window gives).  What each is for:
#   allT      chunk T = 1..6, U 2..16, lane groups of 2..16, 1-2 sub-batches per chunk
#   manysb    7-8 sub-batches per chunk (every wave loops), 5 and 7 landmarks per sub-batch
#   fixedmid  a fixed pose inside chunk windows
#   outl      the Huber branch per lane (10 % outliers)
#   far       kappa(H_ll) = 6e6: the landmark Cholesky
#   cams4     rotated extrinsics, the per-(pose, camera) tables
#   p70       the block-sparse pair list, the second fixed_bits word (pose 66), the banded controller
#   nohuber   no robust kernel
#   tiny      U = 2, a one-landmark sub-batch
CASES = {
    "allT": (lambda: _gen(**_ALLT), 8, {}, _ALLT_SHAPES),
    "manysb": (lambda: _gen(**dict(_ALLT, L=200)), 32, {},
               dict(T={1, 2, 3, 4, 5, 6}, lg={1, 2, 3, 4}, n_lm={1, 2, 3, 4, 5, 7}, sb={1, 7, 8})),
    "fixedmid": (lambda: _gen(fixed=(0, 7), **_ALLT), 8, {}, _ALLT_SHAPES),
    "outl": (lambda: _gen(**dict(_OUTL, outlier_frac=0.1)), 16, {}, _OUTL_SHAPES),
    "far": (lambda: _gen(**dict(_OUTL, depth_max=300.0)), 16, {}, _OUTL_SHAPES),
    "cams4": (lambda: _gen(cams=4, P=8, L=64, k=8, seed=3), 8, {}, dict(T={3}, U={8}, lg={3}, n_lm={8}, sb={1})),
    "p70": (lambda: _gen(fixed=(0, 66), P=70, L=300, k=2, k_max=8, pose_mode=0, seed=1), 16, {},
            dict(T={3}, U={7, 8}, lg={3}, n_lm={1, 2, 3, 4, 5, 6, 7, 8}, sb={1, 2}, sparse=True, fixed_mask=1)),
    "nohuber": (lambda: _gen(**_ALLT), 8, dict(huber_delta=0.0), _ALLT_SHAPES),
    "tiny": (lambda: _gen(P=3, L=9, k=2, k_max=3, pose_mode=1, seed=1), 8, {},
             dict(T={1, 2}, U={2, 3}, lg={1, 2}, n_lm={1, 8}, sb={1})),
}

_cache = {}


def case(name):
    """(window, chunk_landmarks, solver options, claimed shapes) of case `name`; the window is built once."""
    if name not in _cache:
        make, chunk, opts, shapes = CASES[name]
        _cache[name] = (make(), chunk, dict(opts, gate_mode=1), shapes)
    return _cache[name]


def plan_shapes(w, chunk):
    """What plan_window gives for the case: the sets of chunk T and U, of sub-batch lg and n_lm, and of sub-batches
    per chunk; the pair list and whether it is block-sparse."""
    pw = lego_ba.plan_window(w, chunk)
    ch, sb = pw["chunks"], pw["sbs"]
    P = w["n_poses"]
    return dict(T=set(int(t) for t in ch["T"]), U=set(int(u) for u in ch["U"]), lg=set(int(x) for x in sb["lg"]),
                n_lm=set(int(x) for x in sb["n_lm"]), sb=set(int(x) for x in ch["sb_end"] - ch["sb_begin"]),
                pair_pq=pw["pair_pq"].astype(np.int64), sparse=len(pw["pair_pq"]) < P * (P + 1) // 2,
                fixed_mask=pw["fixed_mask"])


RS_LAD = 16   # LH_LAD


def rs_offsets(P, npairs):
    """lh_rs_make (lego-slam_amd/csrc/lh_common.h) restated: the packed reduced system's offsets."""
    off_bs = npairs * 36
    off_bp = off_bs + 6 * P
    off_hd = off_bp + 6 * P
    off_sc = off_hd + 6 * P
    off_bsc = off_sc + 8
    return dict(S=0, bs=off_bs, bp=off_bp, hd=off_hd, sc=off_sc, total=off_bsc + 2 * RS_LAD)


def decode_packed(v, P, pair_pq):
    """The packed vector as (S [6P, 6P] with both triangles filled from the blocks, bs, bp, hd, the four scalars).
    Block b holds S(6p + a, 6q + c) of its pair (p <= q) at 36 b + 6 a + c."""
    o = rs_offsets(P, len(pair_pq))
    assert len(v) == o["total"], (len(v), o["total"])
    S = np.zeros((6 * P, 6 * P))
    for b, (p, q) in enumerate(pair_pq):
        B = v[36 * b:36 * b + 36].reshape(6, 6)
        S[6 * p:6 * p + 6, 6 * q:6 * q + 6] = B
        if p != q:
            S[6 * q:6 * q + 6, 6 * p:6 * p + 6] = B.T
    n = 6 * P
    return S, v[o["bs"]:o["bs"] + n], v[o["bp"]:o["bp"] + n], v[o["hd"]:o["hd"] + n], v[o["sc"]:o["sc"] + 4]
