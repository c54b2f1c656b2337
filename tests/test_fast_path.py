"""The array-free device-resident solve (lh_solve_resident with every output array NULL).

It returns as soon as the host sees the device's stop flag and reads the summary and the trace from
mapped host memory: the stop trial's controller copies them there from lh_ctrl on one thread and
raises done behind that thread's system-scope fence (publish_stop in lh_lm.h).  Nothing else
checks those words: bench.py replays one window, so a stale or torn summary would look like a correct
one there.  Here the array-free solve alternates between windows (and between handles whose solves
stop at different trials) and every scalar and trace entry must equal the synchronous path's (the
same upload solved again with arrays requested, which copies lh_ctrl after a stream synchronisation).
The kernels an array-free solve leaves draining are stream-ordered before the next upload, which is
then solved and checked too.
"""
import numpy as np
import pytest

import lego_ba
import windows

pytestmark = pytest.mark.gpu

FIELDS = ("iterations", "trials", "accepted", "chi2_initial", "chi2_final", "lambda_final", "pcg_iterations",
          "degenerate")


def _banded(P, L, seed):
    w = lego_ba.generate_window(P=P, L=L, k=8, seed=seed, **dict(windows.STABLE, outlier_frac=0.0))
    f = np.zeros(P, np.uint8)
    f[0] = 1
    w["pose_fixed"] = f
    return w


def _same(fast, full, what):
    for f in FIELDS:
        assert fast[f] == full[f], (what, f, fast[f], full[f])
    assert np.array_equal(fast["trace_chi2"], full["trace_chi2"]), what
    assert np.array_equal(fast["trace_lambda"], full["trace_lambda"]), what


def _check_window(s, w, what):
    s.upload(w)
    fast = s.solve_resident()                       # array-free: mapped summary
    full = s.solve_resident(want_states=True, want_edges=True)
    _same(fast, full, what)
    again = s.solve_resident()
    _same(again, full, what + " (repeat)")
    return fast


@pytest.mark.parametrize("kw,controller", [({}, "k_ctrl"), ({"linear_solver": lego_ba.LH_SOLVER_PCG}, "k_ctrl")])
def test_array_free_solves_alternating_windows(kw, controller):
    """k_ctrl (LDL^T and PCG): C2 and C3 windows, a survey-default one with rejections, alternated."""
    s = lego_ba.Solver(**kw)
    ws = [("C2 stable_noout", windows.window("C2", seed=0, family="stable_noout")),
          ("C3 stable_noout", windows.window("C3", seed=0, family="stable_noout")),
          ("C2 default", windows.window("C2", seed=1, family="default"))]
    first = {}
    for rnd in range(2):
        for name, w in ws:
            r = _check_window(s, w, name)
            assert s.controller() == controller
            if rnd == 0:
                first[name] = r
            else:
                _same(r, first[name], name + " (second round)")
    # the windows stop at different trials, so a stale summary would have been caught
    assert len({first[n]["trials"] for n, _ in ws}) > 1
    s.close()


def test_array_free_solves_alternating_stop_points():
    """Two handles on one window whose solves stop at different trials (max_iters 3 and 10), their
    array-free solves interleaved."""
    w = windows.window("C3", seed=0, family="stable_noout")
    a, b = lego_ba.Solver(max_iters=3), lego_ba.Solver()
    a.upload(w)
    b.upload(w)
    ra = [a.solve_resident() for _ in range(1)]
    rb = [b.solve_resident() for _ in range(1)]
    for _ in range(3):
        ra.append(a.solve_resident())
        rb.append(b.solve_resident())
    fa = a.solve_resident(want_states=True)
    fb = b.solve_resident(want_states=True)
    assert fa["iterations"] == 3 and fb["iterations"] > 3
    for r in ra:
        _same(r, fa, "max_iters 3")
    for r in rb:
        _same(r, fb, "max_iters 10")
    a.close()
    b.close()


def test_array_free_solves_banded_controller():
    """k_ctrl_b (128 keyframes): its stop trial publishes the summary the same way."""
    s = lego_ba.Solver()
    w1, w2 = _banded(128, 8000, 1), _banded(96, 6000, 1)
    r1 = _check_window(s, w1, "P128")
    assert s.controller() == "k_ctrl_b"
    r2 = _check_window(s, w2, "P96")
    assert s.controller() == "k_ctrl_b"
    _same(_check_window(s, w1, "P128 again"), r1, "P128 after P96")
    assert r1["trials"] != r2["trials"] or r1["chi2_final"] != r2["chi2_final"]
    s.close()
