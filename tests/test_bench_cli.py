"""bench.py's command line: a plain run prints the timed line alone, --dump-outputs writes what the last
timed step computed (the same bytes from run to run), --full adds the per-kernel times and the roofline.
"""
import json
import os

import numpy as np
import pytest

import bench

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("kernels_ms_per_solve_event_bracketed", "roofline", "roofline_hbm", "host_buffer_path", "c4_1gpu",
             "live_config_c3", "pcg", "fp32_resid", "p64_window", "estimate_pose", "lk_optical_flow", "cpu_baseline")


def test_dump_budget_keeps_arrays_that_fit():
    a = {"x": np.arange(12.0).reshape(4, 3), "y": np.arange(5.0)}
    out = bench.fit_dump_budget(a, 10_000)
    assert list(out) == ["x", "y"] and all(out[k] is a[k] for k in a)


def test_dump_budget_samples_large_arrays_reproducibly():
    rng = np.random.default_rng(1)
    a = {"small": rng.standard_normal(7), "lm": rng.standard_normal((3001, 3)), "edges": rng.standard_normal(24007)}
    budget = 100_000        # lm 72 024 B + edges 192 056 B + small 56 B: over
    out = bench.fit_dump_budget(a, budget)
    assert list(out) == list(a)
    assert sum(v.nbytes for v in out.values()) <= budget
    assert out["small"] is a["small"]
    for k in ("lm", "edges"):
        full, part = a[k], out[k]
        assert part.shape[1:] == full.shape[1:] and 0 < len(part) < len(full)
        # rows of the array, in ascending order, none twice (the values are distinct)
        pos = {row.tobytes(): i for i, row in enumerate(full.reshape(len(full), -1))}
        idx = [pos[row.tobytes()] for row in part.reshape(len(part), -1)]
        assert idx == sorted(set(idx))
        # the budget is used, not merely respected
        assert len(part) >= int(0.9 * len(full) * budget / (a["lm"].nbytes + a["edges"].nbytes))
    again = bench.fit_dump_budget({k: v.copy() for k, v in a.items()}, budget)
    assert all(np.array_equal(out[k], again[k]) for k in a)


def _run(capsys, argv):
    capsys.readouterr()
    bench.main(argv)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    return [str(tmp_path_factory.mktemp(f"dump{i}")) for i in range(2)]


@pytest.mark.gpu
def test_plain_run_prints_the_timed_line_and_dumps_reproducible_outputs(capsys, dumps, monkeypatch):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    lines = [_run(capsys, ["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", d]) for d in dumps]
    for d in lines:
        assert all(k in d for k in HEADLINE)
        assert not any(k in d for k in FULL_ONLY)
        assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "LM iterations/s" and d["dtype"] == "f64"
        assert d["higher_is_better"] is True and d["ms_per_step"] > 0
        # value is LM iterations per second over the timed steps (both figures are rounded in the line)
        assert d["value"] == pytest.approx(d["iterations_per_solve"] / (d["ms_per_step"] * 1e-3), rel=1e-3)
    names = {"summary", "trace_chi2", "trace_lambda", "pose_Tcw", "lm_xyz", "edge_robust_chi2"}
    a, b = ({n[:-4]: np.load(os.path.join(d, n)) for n in os.listdir(d)} for d in dumps)
    assert set(a) == names and set(b) == names
    assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000
    for n in names:
        assert a[n].dtype == np.float64 and np.isfinite(a[n]).all(), n
        assert a[n].tobytes() == b[n].tobytes() and a[n].shape == b[n].shape, n
    c3 = bench.WORKLOADS["C3"]
    assert a["pose_Tcw"].shape == (c3["P"], 12) and a["lm_xyz"].shape == (c3["L"], 3)
    assert a["edge_robust_chi2"].shape == (c3["L"] * c3["k"],)
    s = dict(zip(bench.SUMMARY_FIELDS, a["summary"]))
    assert s["chi2_final"] == lines[0]["chi2_final"] and s["iterations"] == lines[0]["iterations_per_solve"]
    assert len(a["trace_chi2"]) == len(a["trace_lambda"]) > 0
    assert s["chi2_final"] < s["chi2_initial"]
    # the dumped per-edge robust chi2 is the state the summary describes: chi2 = sum / 2, to the worst-case
    # rounding of a 400 000-term fp64 sum in any order (n eps = 4.4e-11)
    assert 0.5 * a["edge_robust_chi2"].sum() == pytest.approx(s["chi2_final"], rel=1e-10)
    # the solve moved the landmarks it was given
    w = bench.make_window("C3", "stable_noout", 0, 0, 1)
    assert not np.array_equal(a["lm_xyz"], w["lm_xyz"])


@pytest.mark.gpu
def test_full_run_adds_kernel_times_and_roofline(capsys, monkeypatch):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    d = _run(capsys, ["--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--no-extras"])
    assert all(k in d for k in HEADLINE)
    assert set(d["kernels_ms_per_solve_event_bracketed"]) >= {"k_lin", "k_reduce", "k_ctrl"}
    assert d["roofline"]["kernel"] == "k_lin" and d["roofline"]["avg_launch_ms"] > 0
    assert d["roofline_hbm"]["bound"] == "hbm"
