"""The planner's choice of k_lin's workgroup shape (lego-slam_amd/csrc/lh_plan.cpp, through liblego_plan.so).

Four waves per workgroup, two workgroups per compute unit, is the plan of every window that does not fill the GPU
and of every window with an explicit chunk size.  An auto-chunked window with more four-wave chunks than compute units
whose chunks are all T <= 3 gets eight waves per workgroup and at most one chunk per compute unit.

The rule the kernel implements for the eight-wave shape: sub-batch i of a chunk runs on wave i mod 8, and waves w
and w + 4 share a SIMD.  So a chunk of n sub-batches gives wave w  n // 8 + (w < n % 8)  of them, the four SIMD
pairs' loads differ by at most one, and two waves of one SIMD both carry the chunk's maximum only when n % 8 is 0 or
more than 4, that is, when every SIMD holds a wave with the maximum anyway (five or more long waves on four SIMDs).
A full chunk (26 sub-batches on C3: loads 7, 7, 6, 6) never has both waves of a SIMD long."""
import numpy as np
import pytest

import lego_ba
from test_plan_cpu import check_plan
from windows import window

N_CU = 256   # the planner's default where there is no device


def wave_counts(n, waves=8):
    """Sub-batches per wave of a chunk of n sub-batches: sub-batch i runs on wave i mod `waves` (k_lin's loop)."""
    return np.bincount(np.arange(n) % waves, minlength=waves)


@pytest.fixture(scope="module")
def c3():
    w = window("C3", seed=0, family="stable_noout")
    return w, lego_ba.plan_window(w, threads=4), lego_ba.plan_shape(w, threads=4)


def test_c3_window_gets_eight_waves_one_chunk_per_cu(c3):
    w, pl, sh = c3
    assert len(w["lm_xyz"]) == 50_000
    assert sh["waves"] == 8 and sh["n_cu"] == N_CU
    ch = pl["chunks"]
    assert sh["n_chunks"] == len(ch) <= N_CU
    assert len(ch) > N_CU // 2                                  # the GPU stays filled
    assert np.all(ch["T"] == 3)
    # every landmark exactly once (and every other invariant of a plan)
    lp = pl["lm_perm"]
    assert np.array_equal(np.sort(lp[lp >= 0]), np.arange(50_000))
    check_plan(w, pl)
    per_chunk = [int(pl["sbs"]["n_lm"][s:e].sum()) for s, e in zip(ch["sb_begin"], ch["sb_end"])]
    assert max(per_chunk) <= sh["chunk_lm"]


def test_long_waves_sit_on_distinct_simds(c3):
    _, pl, _ = c3
    ch = pl["chunks"]
    nsb = (ch["sb_end"] - ch["sb_begin"]).astype(int)
    full = np.bincount(nsb).argmax()
    assert full % 8 in (1, 2, 3, 4) and np.sum(nsb == full) > 0.9 * len(nsb)   # C3: 26 sub-batches
    for n in np.unique(nsb):
        c = wave_counts(int(n))
        assert c.sum() == n and c.max() - c.min() <= 1
        simd = c[:4] + c[4:]
        assert simd.max() - simd.min() <= 1
        both = [(c[w] == c.max() and c[w + 4] == c.max()) for w in range(4)]
        if any(both) and simd.min() < simd.max():
            # only where every SIMD holds a wave with the maximum anyway
            assert n % 8 > 4 and all(max(c[w], c[w + 4]) == c.max() for w in range(4)), n
        if n % 8 in (1, 2, 3, 4):
            assert not any(both), n
    assert sorted(wave_counts(26)[:4] + wave_counts(26)[4:], reverse=True) == [7, 7, 6, 6]
    assert sorted(wave_counts(25)[:4] + wave_counts(25)[4:], reverse=True) == [7, 6, 6, 6]


def test_the_chunk_count_follows_the_cu_count(c3):
    w, _, _ = c3
    sh = lego_ba.plan_shape(w, threads=4, n_cu=304)
    assert sh["waves"] == 8 and sh["n_chunks"] <= 304
    sh = lego_ba.plan_shape(w, threads=4, n_cu=160)             # past the four-wave plan's 256-landmark clamp
    assert sh["waves"] == 8 and sh["n_chunks"] <= 160 and 256 < sh["chunk_lm"] <= 512
    # fewer compute units than chunks of the largest size the shape allows (512 landmarks): four waves
    sh = lego_ba.plan_shape(w, threads=4, n_cu=64)
    assert sh["waves"] == 4 and sh["n_chunks"] == 488


def _same_plan(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("cfg,L,chunk_lm", [("small", 2000, 0), ("C3", 50_000, 104), ("C3", 50_000, 208),
                                            ("C2", 5000, 0), ("C2", 5000, 64)])
def test_other_windows_keep_the_four_wave_plan(cfg, L, chunk_lm, c3, monkeypatch):
    """A window that does not fill the GPU, and any window with chunk_landmarks set: byte-identical to the plan with
    the switch that forces four waves."""
    if cfg == "small":
        w = lego_ba.generate_window(P=10, L=2000, k=8, seed=1)
    elif cfg == "C3":
        w = c3[0]
    else:
        w = window(cfg, seed=1, family="stable_noout")
    assert len(w["lm_xyz"]) == L
    monkeypatch.delenv("LH_NO_LIN_WG8", raising=False)
    a, sa = lego_ba.plan_window(w, chunk_lm=chunk_lm, threads=3), lego_ba.plan_shape(w, chunk_lm=chunk_lm, threads=3)
    monkeypatch.setenv("LH_NO_LIN_WG8", "1")
    b, sb = lego_ba.plan_window(w, chunk_lm=chunk_lm, threads=3), lego_ba.plan_shape(w, chunk_lm=chunk_lm, threads=3)
    assert sa["waves"] == 4 and sa == sb
    _same_plan(a, b)


def test_the_switch_restores_the_four_wave_plan_on_c3(c3, monkeypatch):
    w, pl8, _ = c3
    monkeypatch.setenv("LH_NO_LIN_WG8", "1")
    sh = lego_ba.plan_shape(w, threads=4)
    pl4 = lego_ba.plan_window(w, threads=4)
    assert sh["waves"] == 4 and sh["chunk_lm"] == 104 and sh["n_chunks"] == len(pl4["chunks"]) == 488
    check_plan(w, pl4)
    assert len(pl8["chunks"]) < len(pl4["chunks"])


def test_the_test_knob_forces_eight_waves_on_a_small_window(monkeypatch):
    """LH_TEST_LIN_WG8=1 (the GPU tests' knob): eight waves on the chunking the window has anyway, if every chunk is
    T <= 3; LH_NO_LIN_WG8 wins over it; a window with a T > 3 chunk keeps four waves."""
    w = lego_ba.generate_window(P=8, L=600, k=8, seed=2)
    base = lego_ba.plan_window(w, chunk_lm=72, threads=2)
    assert lego_ba.plan_shape(w, chunk_lm=72)["waves"] == 4
    monkeypatch.setenv("LH_TEST_LIN_WG8", "1")
    assert lego_ba.plan_shape(w, chunk_lm=72)["waves"] == 8
    _same_plan(base, lego_ba.plan_window(w, chunk_lm=72, threads=2))
    wide = lego_ba.generate_window(P=16, L=96, k=2, k_max=16, pose_mode=1, seed=1)
    assert int(lego_ba.plan_window(wide, chunk_lm=8)["chunks"]["T"].max()) > 3
    assert lego_ba.plan_shape(wide, chunk_lm=8)["waves"] == 4
    monkeypatch.setenv("LH_NO_LIN_WG8", "1")
    assert lego_ba.plan_shape(w, chunk_lm=72)["waves"] == 4
