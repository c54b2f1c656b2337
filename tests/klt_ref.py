"""NumPy restatement of lh_klt_track's definition (include/lego_ba.h): the pyramidal KLT tracker of
cv::calcOpticalFlowPyrLK's scalar path with an 11 x 11 window on 8-bit images, in arithmetic that leaves nothing
to a compiler: integer pyramid, Scharr derivatives and window sums, and float32 steps of one rounding each.

Written from the definition, not from lego-slam_amd/csrc/lh_klt.h: the CPU suite holds the host build of that header
against this file bit for bit, and the GPU suite holds the kernels against it.  Beside kp2 and success it reports, per
point and level, the exit taken, the iterations run, minEig and the distance moved: the tests' coverage assertions
rest on these alone.  OpenCV is not available here: parity with cv::calcOpticalFlowPyrLK itself is not tested."""
import os

import numpy as np

F = np.float32
HALF = 5            # (11 - 1) / 2
WIN = 11
PAD = 11            # a window reaches 11 pixels past an edge
EXITS = ("range_p", "min_eig", "range_q", "eps", "osc", "max_iters")
X_RANGE_P, X_MIN_EIG, X_RANGE_Q, X_EPS, X_OSC, X_MAX_ITERS = range(6)
W5 = np.array([1, 4, 6, 4, 1], np.int64)
FLT_EPSILON = F(2.0 ** -23)


def reflect(i, n):
    """BORDER_REFLECT_101: ... 2 1 | 0 1 2 ... n-2 n-1 | n-2 n-3 ..., one fold (|offset| < n)."""
    i = np.abs(np.asarray(i, np.int64))
    return np.where(i >= n, 2 * (n - 1) - i, i)


def pyr_down(src):
    rows, cols = src.shape
    dr, dc = (rows + 1) // 2, (cols + 1) // 2
    s = src.astype(np.int64)
    taps = np.arange(-2, 3)
    xi = reflect(2 * np.arange(dc)[:, None] + taps, cols)          # [dc, 5]
    yi = reflect(2 * np.arange(dr)[:, None] + taps, rows)          # [dr, 5]
    h = (s[:, xi] * W5).sum(-1)                                    # [rows, dc]
    v = (h[yi, :] * W5[None, :, None]).sum(1)                      # [dr, dc]
    return ((v + 128) >> 8).astype(np.uint8)


def pyramid(img, max_level=3):
    """Level 0 is the image; level l + 1 exists while l < max_level and both its sizes are > 11."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    levels = [np.ascontiguousarray(img)]
    while len(levels) - 1 < max_level:
        rows, cols = levels[-1].shape
        if (rows + 1) // 2 <= WIN or (cols + 1) // 2 <= WIN:
            break
        levels.append(pyr_down(levels[-1]))
    return levels


def scharr(img):
    """Ix, Iy of an 8-bit image, REFLECT_101 neighbours at its edge (int64; |.| <= 4080)."""
    p = np.pad(img.astype(np.int64), 1, mode="reflect")
    t0 = 3 * (p[:-2, :] + p[2:, :]) + 10 * p[1:-1, :]              # [rows, cols + 2]
    ix = t0[:, 2:] - t0[:, :-2]
    t1 = p[2:, :] - p[:-2, :]
    iy = 3 * (t1[:, :-2] + t1[:, 2:]) + 10 * t1[:, 1:-1]
    return ix, iy


def _in_range(ix, iy, cols, rows):
    """The range test on the floored position, in float: NaN and huge values fail."""
    return bool(ix >= F(-PAD) and ix < F(cols) and iy >= F(-PAD) and iy < F(rows))


def _weights(px, ipx, py, ipy):
    a, b = F(px - ipx), F(py - ipy)
    one, s = F(1), F(16384)
    w00 = int(np.rint(F(F(F(one - a) * F(one - b)) * s)))
    w01 = int(np.rint(F(F(a * F(one - b)) * s)))
    w10 = int(np.rint(F(F(F(one - a) * b) * s)))
    return w00, w01, w10, 16384 - w00 - w01 - w10


def _bil(padded, ix, iy, w):
    """The 11 x 11 bilinear sums at the integer corner (ix, iy) of an image padded by PAD, exact (int64)."""
    t = padded[iy + PAD:iy + PAD + WIN + 1, ix + PAD:ix + PAD + WIN + 1]
    return t[:-1, :-1] * w[0] + t[:-1, 1:] * w[1] + t[1:, :-1] * w[2] + t[1:, 1:] * w[3]


def _to_float(s):
    """(float)(double)S * 2^-20"""
    return F(F(np.float64(int(s))) * F(2.0 ** -20))


def track(img1, img2, kp1, kp2_init=None, max_level=3, max_iters=30, epsilon=0.01, min_eig=1e-4):
    """Returns dict(kp2 [n, 2] float32, success [n] bool, levels, exits [n, levels] (index into EXITS), iters
    [n, levels], min_eig [n, levels] (NaN where step 4 was not reached), moved [n, levels] (the largest distance
    along an axis between a level's first and any later q, in that level's pixels))."""
    if min(np.shape(img1)) <= WIN:
        raise ValueError("cols, rows >= 12 is required")
    P1, P2 = pyramid(img1, max_level), pyramid(img2, max_level)
    L = len(P1) - 1
    lv = []
    for a, b in zip(P1, P2):
        gx, gy = scharr(a)
        lv.append(dict(rows=a.shape[0], cols=a.shape[1],
                       I=np.pad(a.astype(np.int64), PAD, mode="reflect"), J=np.pad(b.astype(np.int64), PAD, mode="reflect"),
                       Ix=np.pad(gx, PAD), Iy=np.pad(gy, PAD)))     # a derivative outside the image is 0
    k1 = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
    n = len(k1)
    guess = k1 if kp2_init is None else np.ascontiguousarray(kp2_init, np.float32).reshape(-1, 2)
    out = dict(kp2=np.zeros((n, 2), np.float32), success=np.zeros(n, bool), levels=L + 1,
               exits=np.full((n, L + 1), -1, np.int32), iters=np.zeros((n, L + 1), np.int32),
               min_eig=np.full((n, L + 1), np.nan), moved=np.zeros((n, L + 1)))
    eps2 = float(epsilon) * float(epsilon)
    with np.errstate(all="ignore"):
        for i in range(n):
            k2x, k2y, status = guess[i, 0], guess[i, 1], 1
            for l in range(L, -1, -1):
                v = lv[l]
                sc = F(1.0 / (1 << l))
                px, py = F(k1[i, 0] * sc), F(k1[i, 1] * sc)
                if l == L:
                    qx, qy = F(k2x * sc), F(k2y * sc)
                else:
                    qx, qy = F(F(2) * k2x), F(F(2) * k2y)
                k2x, k2y = qx, qy
                # 1
                px, py = F(px - F(HALF)), F(py - F(HALF))
                ipx, ipy = np.floor(px), np.floor(py)
                if not _in_range(ipx, ipy, v["cols"], v["rows"]):
                    out["exits"][i, l] = X_RANGE_P
                    status = 0 if l == 0 else status
                    continue
                # 2, 3
                w = _weights(px, ipx, py, ipy)
                ix0, iy0 = int(ipx), int(ipy)
                Iw = (_bil(v["I"], ix0, iy0, w) + 256) >> 9
                dx = (_bil(v["Ix"], ix0, iy0, w) + 8192) >> 14
                dy = (_bil(v["Iy"], ix0, iy0, w) + 8192) >> 14
                # 4
                A11, A12, A22 = _to_float((dx * dx).sum()), _to_float((dx * dy).sum()), _to_float((dy * dy).sum())
                D = F(F(A11 * A22) - F(A12 * A12))
                d = F(A11 - A22)
                me = F(F(F(A22 + A11) - np.sqrt(F(F(d * d) + F(F(F(4) * A12) * A12)))) / F(242))
                out["min_eig"][i, l] = float(me)
                if float(me) < min_eig or D < FLT_EPSILON:
                    out["exits"][i, l] = X_MIN_EIG
                    status = 0 if l == 0 else status
                    continue
                D = F(F(1) / D)
                # 5
                qx, qy = F(qx - F(HALF)), F(qy - F(HALF))
                q0x, q0y = float(qx), float(qy)
                pdx = pdy = F(0)
                ex = X_MAX_ITERS
                for j in range(max_iters):
                    iqx, iqy = np.floor(qx), np.floor(qy)
                    if not _in_range(iqx, iqy, v["cols"], v["rows"]):
                        ex = X_RANGE_Q
                        status = 0 if l == 0 else status
                        break
                    out["iters"][i, l] = j + 1
                    wq = _weights(qx, iqx, qy, iqy)
                    diff = ((_bil(v["J"], int(iqx), int(iqy), wq) + 256) >> 9) - Iw
                    b1, b2 = _to_float((diff * dx).sum()), _to_float((diff * dy).sum())
                    ddx = F(F(F(A12 * b2) - F(A22 * b1)) * D)
                    ddy = F(F(F(A12 * b1) - F(A11 * b2)) * D)
                    qx, qy = F(qx + ddx), F(qy + ddy)
                    k2x, k2y = F(qx + F(HALF)), F(qy + F(HALF))
                    out["moved"][i, l] = max(out["moved"][i, l], abs(float(qx) - q0x), abs(float(qy) - q0y))
                    if float(ddx) * float(ddx) + float(ddy) * float(ddy) <= eps2:
                        ex = X_EPS
                        break
                    if j > 0 and abs(float(F(ddx + pdx))) < 0.01 and abs(float(F(ddy + pdy))) < 0.01:
                        k2x, k2y = F(k2x - F(F(0.5) * ddx)), F(k2y - F(F(0.5) * ddy))
                        ex = X_OSC
                        break
                    pdx, pdy = ddx, ddy
                out["exits"][i, l] = ex
            out["kp2"][i] = (k2x, k2y)
            out["success"][i] = bool(status)
    return out


def count(r, exit_code, level=None):
    """How many points took the exit (at one level, or at any)."""
    e = r["exits"] if level is None else r["exits"][:, level]
    return int(np.sum(e == exit_code))


def min_eig_clear(r, threshold):
    """No point's minEig lies within 1e-3 relative of the threshold: no case hangs on step 4's rounding."""
    me = r["min_eig"][np.isfinite(r["min_eig"])]
    return bool(np.all(np.abs(me - threshold) > 1e-3 * threshold)) if threshold > 0 else True


# ---- the host build of lego-slam_amd/csrc/lh_klt.h (tests/klt_probe.cpp) ----
def host_library(build_dir):
    import ctypes as C
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    so = os.path.join(str(build_dir), "libklt_probe.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-I",
                           os.path.join(os.path.dirname(here), "lego-slam_amd", "csrc"),
                           os.path.join(here, "klt_probe.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.klt_track.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]
    lib.klt_pyr_down.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p]
    lib.klt_pyr_down.restype = None
    lib.klt_level_count.argtypes = [C.c_int, C.c_int, C.c_int]
    return lib


def host_track(lib, img1, img2, kp1, kp2_init=None, max_level=3, max_iters=30, epsilon=0.01, min_eig=1e-4):
    """img1, img2: 2-D uint8 of one shape, rows strides[0] bytes apart."""
    assert img1.shape == img2.shape and img1.strides == img2.strides and img1.strides[1] == 1
    k1 = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
    n = len(k1)
    k2 = np.zeros((n, 2), np.float32) if kp2_init is None else np.array(kp2_init, np.float32, copy=True).reshape(-1, 2)
    ok = np.zeros(n, np.uint8)
    rc = lib.klt_track(img1.ctypes.data, img2.ctypes.data, img1.shape[1], img1.shape[0], img1.strides[0], n,
                       k1.ctypes.data, k2.ctypes.data, ok.ctypes.data, int(kp2_init is not None), max_level, max_iters,
                       epsilon, min_eig)
    assert rc == 0
    return dict(kp2=k2, success=ok.astype(bool))


def host_pyr_down(lib, img):
    rows, cols = img.shape
    out = np.zeros(((rows + 1) // 2, (cols + 1) // 2), np.uint8)
    lib.klt_pyr_down(img.ctypes.data, cols, rows, img.strides[0], out.ctypes.data)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
