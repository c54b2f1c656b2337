"""CPU tests of a window's solve configuration (lego-slam_amd/csrc/lh_plan.cpp solve_config and
reduce_table, through liblego_plan.so): which controller an upload picks, whether k_ctrl_b runs narrow or
with its loaders as unit waves, the ladder and batch sizes, who decides and in which layout k_reduce hands
the system over, and k_reduce's block table.  lh_upload calls the same functions and the handle reports
what they returned, so the expectations here are the ones the GPU suite asserts through
Solver.controller(), band_narrow(), band_loader_units(), ladder() and batch() for the same windows."""
import functools

import numpy as np
import pytest

import lego_ba
from windows import STABLE, stable_window, window

LH_LAD = 16          # lh_common.h
PCG = lego_ba.LH_SOLVER_PCG
SWITCHES = ("LH_NO_BAND", "LH_NO_LADDER", "LH_NO_RED_SKIP", "LH_NO_NARROW", "LH_NO_BATCH", "LH_BATCH_MAX", "LH_ND",
            "LH_NO_EVO", "LH_NO_EVAL_FIRST", "LH_LADDER_LAZY", "LH_NO_BIMG", "LH_NO_IMG")


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@functools.lru_cache(maxsize=None)
def _stable(P, L, seed, mode=0):
    return stable_window(P, L, seed, **(dict(pose_mode=1, k_min=2, k_max=8) if mode else {}))


@functools.lru_cache(maxsize=None)
def _wide_band(k):
    w = lego_ba.generate_window(P=96, L=6000, k=k, seed=2, **dict(STABLE, outlier_frac=0.0))
    w["pose_fixed"] = np.eye(1, 96, dtype=np.uint8)[0]
    return w


@functools.lru_cache(maxsize=None)
def _c1():
    return window("C1", seed=1, family="stable")


def _p65(coupled_40_apart):
    """test_window_envelope_edges' windows: 65 keyframes, banded; and with 20 more landmarks that couple
    keyframes 0 and 40."""
    w = lego_ba.generate_window(P=65, L=500, k=8, seed=4)
    if not coupled_40_apart:
        return w
    L = len(w["lm_xyz"])
    wide = dict(w, lm_xyz=np.vstack([w["lm_xyz"], w["lm_xyz"][:20]]))
    wide["obs_pose"] = np.concatenate([w["obs_pose"], np.tile([0, 40], 20)]).astype(w["obs_pose"].dtype)
    wide["obs_lm"] = np.concatenate([w["obs_lm"], np.repeat(np.arange(L, L + 20), 2)]).astype(w["obs_lm"].dtype)
    wide["obs_cam"] = np.concatenate([w["obs_cam"], np.zeros(40, w["obs_cam"].dtype)])
    wide["obs_uv"] = np.vstack([w["obs_uv"], w["obs_uv"][:40]])
    return wide


# ---- the controller ----
@pytest.mark.parametrize("P,L,seed", [(22, 3000, 4), (32, 4000, 1), (64, 6000, 2), (96, 6000, 1), (128, 8000, 1)])
def test_sliding_windows_past_21_keyframes_run_banded(P, L, seed):
    assert lego_ba.solve_config(_stable(P, L, seed))["controller"] == "k_ctrl_b"


def test_random_keyframe_subsets_run_dense():
    assert lego_ba.solve_config(_stable(40, 3000, 3, mode=1))["controller"] == "k_ctrl_g"


def test_80_keyframes_banded_ldlt_and_block_sparse_pcg():
    w = _stable(80, 2000, 5)
    assert lego_ba.solve_config(w)["controller"] == "k_ctrl_b"
    assert lego_ba.solve_config(w, linear_solver=PCG)["controller"] == "k_ctrl_p"


def test_narrow_band(monkeypatch):
    w = _stable(128, 8000, 3)
    c = lego_ba.solve_config(w)
    assert c["controller"] == "k_ctrl_b" and c["band_narrow"]
    monkeypatch.setenv("LH_NO_NARROW", "1")
    c = lego_ba.solve_config(w)
    assert c["controller"] == "k_ctrl_b" and not c["band_narrow"]


@pytest.mark.parametrize("k", [11, 15])
def test_wide_band_loaders_take_units_at_15_keyframe_runs(k):
    c = lego_ba.solve_config(_wide_band(k))
    assert c["controller"] == "k_ctrl_b" and not c["band_narrow"] and c["band_loader_units"] == (k == 15)


def test_envelope_edges_past_64_keyframes():
    assert lego_ba.solve_config(_p65(False))["controller"] == "k_ctrl_b"
    wide = _p65(True)
    with pytest.raises(lego_ba.LhError) as e:
        lego_ba.solve_config(wide)
    assert e.value.status == lego_ba.LH_E_UNSUPPORTED
    assert lego_ba.solve_config(wide, linear_solver=PCG)["controller"] == "k_ctrl_p"


def test_no_band_switch(monkeypatch):
    monkeypatch.setenv("LH_NO_BAND", "1")
    assert lego_ba.solve_config(_stable(64, 6000, 2))["controller"] == "k_ctrl_g"


# ---- who decides, and the system's hand-over layout ----
def test_small_window_runs_k_ctrl_with_the_lds_image(monkeypatch):
    w = _c1()
    c = lego_ba.solve_config(w)
    assert c["controller"] == "k_ctrl" and c["img"] == 1 and c["dec_in_reduce"] == 1 and c["bimg"] == 0
    p = lego_ba.solve_config(w, linear_solver=PCG)
    assert p["controller"] == "k_ctrl" and p["img"] == 0
    monkeypatch.setenv("LH_NO_IMG", "1")
    assert lego_ba.solve_config(w)["img"] == 0


@pytest.mark.parametrize("rccl", [False, True])
def test_small_window_sharded_decides_in_the_controller(rccl):
    c = lego_ba.solve_config(_c1(), world_size=2, rccl=rccl)
    assert c["controller"] == "k_ctrl"
    assert (c["dec_in_reduce"], c["img"], c["bimg"]) == (0, 0, 0)


def test_two_chain_schedule_takes_no_lds_image(monkeypatch):
    """LH_ND=1: the two-chain schedule where lh_ctrl_nd_plan finds a split (C3, as the GPU suite's two-chain
    test; nd_steps is what lhp_ctrl_nd returns for the window's envelope), and then no LDS image.  C1's 5
    keyframes are below the planner's 12: no split there, the one-chain schedule and its image stay."""
    monkeypatch.setenv("LH_ND", "1")
    for w, splits in ((window("C3", seed=0, family="stable_noout"), True), (_c1(), False)):
        c = lego_ba.solve_config(w)
        assert c["controller"] == "k_ctrl"
        assert c["nd_steps"] == lego_ba.ctrl_nd(c["pf"])["nsteps"]
        assert (c["nd_steps"] > 0) == splits
        assert c["img"] == (0 if splits else 1)
        assert lego_ba.solve_config(w, linear_solver=PCG)["nd_steps"] == 0


def test_banded_window_on_one_rank_takes_the_band_image(monkeypatch):
    w = _stable(32, 4000, 1)
    c = lego_ba.solve_config(w)
    assert c["controller"] == "k_ctrl_b"
    assert (c["bimg"], c["commit_in_reduce"], c["dec_in_reduce"], c["img"]) == (1, 1, 1, 0)
    s = lego_ba.solve_config(w, world_size=2)
    assert s["controller"] == "k_ctrl_b" and (s["bimg"], s["commit_in_reduce"], s["dec_in_reduce"]) == (0, 1, 0)
    monkeypatch.setenv("LH_NO_BIMG", "1")
    c = lego_ba.solve_config(w)
    assert (c["bimg"], c["commit_in_reduce"]) == (0, 1)


# ---- ladder and batch ----
@pytest.mark.parametrize("max_trials", [1, 10, 16, 20])
def test_ladder_and_batch_sizes(max_trials, monkeypatch):
    w = _c1()
    rungs = min(max_trials, LH_LAD)
    c = lego_ba.solve_config(w, max_trials=max_trials)
    assert (c["ladder"], c["batch"]) == (rungs, rungs)
    with monkeypatch.context() as m:
        m.setenv("LH_BATCH_MAX", "4")
        c = lego_ba.solve_config(w, max_trials=max_trials)
        assert (c["ladder"], c["batch"]) == (rungs, min(rungs, 4))
    with monkeypatch.context() as m:
        m.setenv("LH_NO_BATCH", "1")
        c = lego_ba.solve_config(w, max_trials=max_trials)
        assert (c["ladder"], c["batch"]) == (rungs, 1)
    with monkeypatch.context() as m:
        m.setenv("LH_NO_LADDER", "1")
        c = lego_ba.solve_config(w, max_trials=max_trials)
        assert (c["ladder"], c["batch"]) == (1, 1)


# ---- k_reduce's block table ----
@pytest.mark.parametrize("P,L,seed", [(96, 6000, 1), (32, 4000, 1)])
def test_reduce_table_skips_uncoupled_pairs_on_one_rank(P, L, seed, monkeypatch):
    w = _stable(P, L, seed)
    pq = lego_ba.plan_window(w)["pair_pq"].astype(np.uint32)

    def check(rows, npairs, pair_ptr, blocks):
        assert np.array_equal(rows[-1], [npairs, 0, 0, 0])   # the scalar block's sentinel
        assert np.array_equal(rows[:-1, 0], blocks)
        assert np.array_equal(rows[:-1, 1], pair_ptr[blocks]) and np.array_equal(rows[:-1, 2], pair_ptr[blocks + 1])

    rows, npairs, pair_ptr = lego_ba.reduce_table(w)
    coupled = np.flatnonzero(pair_ptr[:-1] < pair_ptr[1:])
    check(rows, npairs, pair_ptr, coupled)
    assert np.array_equal(rows[:-1, 3], pq[coupled, 0] | pq[coupled, 1] << 16)
    if P <= 64:   # the dense layout lists every pair: most of a sliding window's are coupled by no chunk
        assert npairs == P * (P + 1) // 2 and len(coupled) < npairs
    rows2, npairs2, pair_ptr2 = lego_ba.reduce_table(w, world_size=2)   # (past 64 poses: the rank-invariant pair list)
    check(rows2, npairs2, pair_ptr2, np.arange(npairs2))
    monkeypatch.setenv("LH_NO_RED_SKIP", "1")
    rows, npairs, pair_ptr = lego_ba.reduce_table(w)
    check(rows, npairs, pair_ptr, np.arange(npairs))
