// trial_schedule_check.cpp — the planner's trial schedule (lh_plan.h trial_schedule, may_enqueue, topup_target)
// over the grid of tests/test_trial_schedule_cpu.py, as a stand-alone program for the sanitizer build
// (make -C lego-slam_amd san-schedule): the functions against the expressions they replaced in lh_host.cpp, and two
// simulated ranks that see the progress word at different lags never pass the top-up target of the stop chain.
#include <algorithm>
#include <cstdio>
#include <random>

#include "../csrc/lh_plan.h"

static int fails = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c) && ++fails < 20) std::printf("line %d: %s\n", __LINE__, #c); \
    } while (0)

static void simulate(std::mt19937& rng, const lh::TrialSchedule& ts, int s) {
    const int target = lh::topup_target(ts, s);
    std::vector<int> near(s + 1);
    for (int& b : near) b = (int)(rng() & 1);
    int dev = -1, view[2] = {-1, -1}, enq[2] = {0, 0};
    bool done[2] = {false, false};
    auto running = [&](int r) { return !done[r] && enq[r] < ts.max_total; };
    for (long step = 0; running(0) || running(1); ++step) {
        CHECK(step < 4000L * (ts.max_total + 2));
        if (step >= 4000L * (ts.max_total + 2)) return;
        if (dev < s && dev + 1 <= std::min(enq[0], enq[1]) && (rng() & 1)) ++dev;
        for (int r = 0; r < 2; ++r) {
            if (!running(r)) continue;
            if (rng() % 4 <= (unsigned)(r + 1)) {   // rank 1 reads fresh words more often than rank 0
                const int seen = view[r] < 0 ? -1 : view[r] >> 1;
                const int k = seen + (int)(rng() % (unsigned)(dev - seen + 1));
                view[r] = k < 0 ? -1 : 2 * k + near[k];
                done[r] = dev == s && (rng() & 1);
                if (done[r]) continue;
            }
            CHECK(view[r] <= 2 * s + 1);
            if (lh::may_enqueue(ts, view[r], enq[r])) CHECK(++enq[r] <= target);
        }
    }
    for (int r = 0; r < 2; ++r)
        for (; enq[r] < target; ++enq[r]) {}   // the top-up loop as the host runs it
    CHECK(enq[0] == target && enq[1] == target && target <= ts.max_total);
}

int main() {
    const int iters[] = {0, 1, 8}, trials[] = {0, 1, 10}, tps[] = {0, 1, 2, 5, 40};
    std::mt19937 rng(20240607);
    long cases = 0;
    for (int mi : iters) for (int mt : trials) for (int ef = 0; ef < 2; ++ef) for (int t : tps) for (int host = 0; host < 2; ++host) {
        const lh::TrialSchedule ts = lh::trial_schedule(mi, mt, ef, t, host != 0);
        const int max_total = mi > 0 ? mi * (std::max(1, mt) + (ef ? 1 : 0)) : 0;
        const int depth = host ? 1 : (t > 0 ? std::min(t, 32) : 2);
        CHECK(ts.max_total == max_total && ts.depth == depth);
        for (int s = 0; s <= max_total; ++s) {
            CHECK(lh::topup_target(ts, s) == std::min(s + depth, max_total));
            simulate(rng, ts, s);
            ++cases;
        }
        for (int pw = -1; pw < 2 * max_total + 2; ++pw)
            for (int enq = 0; enq <= max_total; ++enq) {
                const int last = pw < 0 ? -1 : (pw >> 1);
                CHECK(lh::may_enqueue(ts, pw, enq) == (enq - last < ((pw >= 0 && (pw & 1)) ? 1 : depth)));
            }
    }
    std::printf("trial_schedule_check: %ld simulated solves, %d failures\n", cases, fails);
    return fails ? 1 : 0;
}
