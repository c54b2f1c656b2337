"""Diagnostic: where k_lin's waves sit and when each finishes its sub-batches, from the -DLH_STAMPS build (set LH_LIB
to lib/liblego_ba_stamps.so).  For the last full trial launch of a solve of the C3 window, in k_lin's default shape
and with LH_NO_LIN_WG8=1: per compute unit the waves on each SIMD (HW_ID), the waves that run the extra sub-batch
("long"), whether a long wave's SIMD-mate is long too, and the duration of each round (a wave's r-th sub-batch) by
how many waves of its SIMD were in a sub-batch of the same index.  The stamps perturb the kernel: shares and
placement only, never this build's run time.
usage: LH_LIB=lego-slam_amd/lib/liblego_ba_stamps.so python scripts/lin_wave_stamps.py [CFG]"""
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lego-slam_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lego_ba  # noqa: E402
from windows import window  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "C3"
w = window(cfg, seed=0, family="stable_noout")


def measure(no_wg8):
    if no_wg8:
        os.environ["LH_NO_LIN_WG8"] = "1"
    else:
        os.environ.pop("LH_NO_LIN_WG8", None)
    s = lego_ba.Solver(device=0)
    s.upload(w)
    s.solve_resident()
    lego_ba.debug_lin_stamps()
    r = s.solve_resident()
    st = lego_ba.debug_lin_stamps()
    nw, nchunks, chunk_lm = s.lin_shape()
    s.close()
    return st, nw, nchunks, chunk_lm, r


def report(st, nw, nchunks, chunk_lm, r):
    valid = np.flatnonzero((st[:, 0] >> np.uint64(40)) & np.uint64(1))
    print(f"== {cfg}: {nw} waves per workgroup, {nchunks} chunks of at most {chunk_lm} landmarks; "
          f"{r['iterations']} iterations, {r['trials']} trials; {len(valid)} wave records")
    if len(valid) == 0:
        print("no records: not the LH_STAMPS build")
        return
    hw = st[valid, 0].astype(np.int64)
    wg, wave = valid // nw, valid % nw
    simd, cu = (hw >> 4) & 3, ((hw >> 32) & 0xF) * 256 + ((hw >> 8) & 0xFF)
    t = st[valid, 1:].astype(np.int64)
    rounds = (t[:, 1:] != 0).sum(1)
    if nw == 8:
        same = 0
        for g in np.unique(wg):
            m = wg == g
            sd = dict(zip(wave[m], simd[m]))
            same += all(sd.get(k) == sd.get(k + 4) for k in range(4) if k in sd and k + 4 in sd)
        print(f"workgroups whose waves w and w + 4 share a SIMD: {same} of {len(np.unique(wg))}")
    per_cu = collections.Counter(cu.tolist())
    wgs_cu = {c: len(set(wg[cu == c].tolist())) for c in per_cu}
    print("workgroups per compute unit:", sorted(collections.Counter(wgs_cu.values()).items()))
    print("waves per (compute unit, SIMD):", sorted(collections.Counter(
        collections.Counter(zip(cu.tolist(), simd.tolist())).values()).items()))
    # long waves: the most rounds on their compute unit; beside = a SIMD-mate is long too
    dur = np.diff(t, axis=1)                         # dur[:, r]: round r
    stats = collections.defaultdict(list)
    beside = alone = 0
    for c in per_cu:
        m = np.flatnonzero(cu == c)
        rmax = rounds[m].max()
        if rmax < 2 or (rounds[m] == rmax).all():
            continue
        for i in m:
            mates = [j for j in m if j != i and simd[j] == simd[i]]
            for rr in range(rounds[i]):
                # SIMD-mates inside a sub-batch during this round: overlap of the two intervals
                a, b = t[i, rr], t[i, rr + 1]
                busy = 0
                for j in mates:
                    for q in range(rounds[j]):
                        busy += max(0, min(b, t[j, q + 1]) - max(a, t[j, q]))
                share = busy / max(b - a, 1)
                stats["shared" if share > 0.5 else "solo"].append(dur[i, rr])
            if rounds[i] == rmax:
                if any(rounds[j] == rmax for j in mates):
                    beside += 1
                else:
                    alone += 1
                stats["last round of a long wave, mate long" if any(rounds[j] == rmax for j in mates)
                      else "last round of a long wave, mate short or none"].append(dur[i, rmax - 1])
    print(f"long waves (an extra sub-batch): {beside} beside a long wave of their SIMD, {alone} not")
    for k in sorted(stats):
        v = np.array(stats[k])
        print(f"  {k:48s} n {len(v):5d}  mean {v.mean():8.1f} ticks  median {np.median(v):8.1f}")
    # the waves of three compute units
    for c in list(per_cu)[:3]:
        m = np.flatnonzero(cu == c)
        m = m[np.lexsort((wave[m], wg[m], simd[m]))]
        t0 = t[m, 0].min()   # (the clock is per XCD: comparable within a compute unit only)
        print(f"  compute unit {c:#06x}:  simd wg wave rounds | start, end of each round (ticks from the compute unit's first)")
        for i in m:
            ends = " ".join(f"{x - t0:6d}" for x in t[i, 1:1 + rounds[i]])
            print(f"    {simd[i]:4d} {wg[i]:4d} {wave[i]:3d} {rounds[i]:5d} | {t[i, 0] - t0:6d}  {ends}")


for no_wg8 in (False, True):
    report(*measure(no_wg8))
