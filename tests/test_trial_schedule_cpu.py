"""CPU tests of a solve's trial schedule (lego-slam_amd/csrc/lh_plan.cpp trial_schedule, may_enqueue and
topup_target, through liblego_plan.so): the functions against the expressions they replaced in lh_host.cpp,
restated here, over a grid of options; then, by simulation, the invariant a sharded solve depends on: whatever
the lag at which each rank sees the device's progress word, no rank enqueues more than the top-up target of the
stop chain, so every rank ends the solve with the same number of exchanges, and none past max_total."""
import itertools

import numpy as np
import pytest

import lego_ba

MAX_ITERS = (0, 1, 8)
MAX_TRIALS = (0, 1, 10)
EVAL_FIRST = (0, 1)
TRIALS_PER_SYNC = (0, 1, 2, 5, 40)
HOST = (False, True)
GRID = list(itertools.product(MAX_ITERS, MAX_TRIALS, EVAL_FIRST, TRIALS_PER_SYNC, HOST))


# ---- the expressions of solve_resident_impl before the schedule moved into the planner ----
def ref_max_total(max_iters, max_trials, eval_first):
    return max_iters * (max(1, max_trials) + (1 if eval_first else 0)) if max_iters > 0 else 0


def ref_depth(trials_per_sync, host):
    return 1 if host else (min(trials_per_sync, 32) if trials_per_sync > 0 else 2)


def ref_may_enqueue(depth, pw, enq):
    last = -1 if pw < 0 else pw >> 1
    return enq - last < (1 if (pw >= 0 and (pw & 1)) else depth)


def ref_target(max_total, depth, stop_chain):
    return min(stop_chain + depth, max_total)


def _schedules():
    """every (max_total, depth) of the grid, once"""
    return sorted({(ref_max_total(mi, mt, ef), ref_depth(tps, host)) for mi, mt, ef, tps, host in GRID})


def test_schedule_matches_the_parent_expressions():
    for mi, mt, ef, tps, host in GRID:
        assert lego_ba.trial_schedule(mi, mt, ef, tps, host) == (ref_max_total(mi, mt, ef), ref_depth(tps, host)), \
            (mi, mt, ef, tps, host)


def test_enqueue_test_and_target_match_the_parent_expressions():
    for max_total, depth in _schedules():
        for s in range(max_total + 1):
            assert lego_ba.topup_target(max_total, depth, s) == ref_target(max_total, depth, s), (max_total, depth, s)
        for pw in range(-1, 2 * max_total + 2):
            for enq in range(max_total + 1):
                assert lego_ba.may_enqueue(max_total, depth, pw, enq) == ref_may_enqueue(depth, pw, enq), \
                    (max_total, depth, pw, enq)


def _simulate(rng, max_total, depth, s):
    """Two ranks and one device.  Chain 0 is the initial linearisation (enqueued by both ranks before the loop),
    chain k >= 1 is trial k.  The device decides chain k once both ranks have enqueued it (its exchange needs
    both), writes the progress word 2 k + near_k, and stops on chain s: the word never passes 2 s + 1.  Each rank
    runs the enqueue loop of solve_resident_impl on its own, lagging view of the word and of done.  Returns the
    ranks' counts at the end of their loops; asserts the bound after every enqueue."""
    near = rng.integers(0, 2, size=s + 1)
    target = lego_ba.topup_target(max_total, depth, s)
    dev = -1                       # the last chain decided
    view = [-1, -1]                # the progress word each rank last read
    done_seen = [False, False]
    enq = [0, 0]
    p_dev = rng.uniform(0.1, 0.9)
    p_look = rng.uniform(0.05, 0.95, size=2)   # how often each rank's read is fresh: the ranks' lags
    running = lambda r: not done_seen[r] and enq[r] < max_total   # noqa: E731  (the loop's condition)
    steps = 0
    while running(0) or running(1):
        steps += 1
        assert steps < 4000 * (max_total + 2), "the simulated solve does not end"
        if dev < s and dev + 1 <= min(enq) and rng.random() < p_dev:
            dev += 1
        for r in rng.permutation(2):
            if not running(r):
                continue
            if rng.random() < p_look[r]:
                # a read anywhere between the last one and the device's latest word; done only once it is raised
                seen = -1 if view[r] < 0 else view[r] >> 1
                k = int(rng.integers(seen, dev + 1))
                view[r] = -1 if k < 0 else 2 * k + int(near[k])
                done_seen[r] = dev == s and rng.random() < 0.5
                if done_seen[r]:
                    continue
            assert view[r] <= 2 * s + 1
            if lego_ba.may_enqueue(max_total, depth, view[r], enq[r]):
                enq[r] += 1
                assert enq[r] <= target, (max_total, depth, s, r, view[r], enq[r], target)
    return enq, target


def test_every_rank_issues_the_same_number_of_exchanges():
    rng = np.random.default_rng(20240607)
    for max_total, depth in _schedules():
        for s in range(max_total + 1):
            enq, target = _simulate(rng, max_total, depth, s)
            final = []
            for e in enq:   # the top-up loop as the host runs it: for (; enq < target; ++enq); it never takes back
                while e < target:
                    e += 1
                final.append(e)
            assert final[0] == final[1] == target, (max_total, depth, s, enq, target)
            assert max(final) <= max_total, (max_total, depth, s, final)


@pytest.mark.parametrize("depth", [1, 2, 5, 32])
def test_the_near_bit_allows_one_ahead(depth):
    """one iteration from max_iters the host keeps a single trial ahead, whatever the depth"""
    for last in range(4):
        assert lego_ba.may_enqueue(100, depth, 2 * last + 1, last)
        assert not lego_ba.may_enqueue(100, depth, 2 * last + 1, last + 1)
        assert lego_ba.may_enqueue(100, depth, 2 * last, last + depth - 1)
        assert not lego_ba.may_enqueue(100, depth, 2 * last, last + depth)
