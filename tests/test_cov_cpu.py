"""CPU tests of lh_covariance's boundary and of its reference (include/lego_ba.h): the ctypes mirrors
of its two structs against a compiled C program; tests/cov_ref.py's formula against the blocks of the inverse of the
assembled full Hessian; the free gauge (singular without an anchor, regular with one); and lh_cov.h's plain-C++
landmark arithmetic, compiled with g++, against the reference.  No GPU call is made here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import cov_ref
import lego_ba
import lin_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"lh_cov_input": "LhCovInput", "lh_cov_result": "LhCovResult"}
LD = cov_ref.LD


def test_ctypes_layout_matches_header(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "lego_ba.h"', "int main(void) {"]
    for c_name, py_name in STRUCTS.items():
        lines.append(f'  printf("{c_name} %zu\\n", sizeof({c_name}));')
        for field, _ in getattr(lego_ba, py_name)._fields_:
            lines.append(f'  printf("{c_name}.{field} %zu\\n", offsetof({c_name}, {field}));')
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    hdr = open(os.path.join(ROOT, "include", "lego_ba.h")).read()
    for c_name, py_name in STRUCTS.items():
        cls = getattr(lego_ba, py_name)
        assert got[c_name] == C.sizeof(cls), c_name
        for field, _ in cls._fields_:
            assert getattr(cls, field).offset == got[f"{c_name}.{field}"], (c_name, field)
        # the header's fields, in its order, are the mirror's
        body = re.sub(r"/\*.*?\*/", "", hdr.split(f"typedef struct {c_name} {{")[1].split(f"}} {c_name};")[0], flags=re.S)
        names = [part.replace("*", " ").split("[")[0].split()[-1] for decl in body.split(";")[:-1] for part in decl.split(",")]
        assert names == [f for f, _ in cls._fields_], c_name


def test_symbol_status_and_message():
    lib = lego_ba.ba_lib()
    assert "lh_covariance" in lego_ba.ABI_SYMBOLS and hasattr(lib, "lh_covariance")
    assert lego_ba.LH_E_SINGULAR == 7 and b"singular" in lib.lh_strerror(lego_ba.LH_E_SINGULAR)
    assert re.search(r"LH_E_SINGULAR\s*=\s*7\b", open(os.path.join(ROOT, "include", "lego_ba.h")).read())


def test_formula_against_the_full_hessian_inverse():
    """tiny: Sigma_pp and every Sigma_l are the corresponding blocks of the inverse of the full (6 P_free + 3 L)^2
    Gauss-Newton Hessian [[H_pp, H_pl], [H_lp, H_ll]] (H_pp = S + H_pl H_ll^-1 H_lp, assembled from the
    linearisation's per-edge blocks), to 1e-11 of the block's largest entry."""
    w, _, opts, _ = lin_cases.case("tiny")
    cv = cov_ref.covariance(w, huber_delta=opts.get("huber_delta", 5.991))
    R, free = cv["R"], cv["free"]
    P, L = w["n_poses"], len(w["lm_xyz"])
    Hpl = np.zeros((6 * P, 3 * L), LD)
    for e, (p, l) in enumerate(zip(R["op"], R["ol"])):
        Hpl[6 * p:6 * p + 6, 3 * l:3 * l + 3] += R["Hpl"][e]
    Hll = np.zeros((3 * L, 3 * L), LD)
    Hli = np.zeros((3 * L, 3 * L), LD)
    for l in range(L):
        Hll[3 * l:3 * l + 3, 3 * l:3 * l + 3] = R["Hll"][l]
        Hli[3 * l:3 * l + 3, 3 * l:3 * l + 3] = R["Hinv"][l]
    Hpp = R["S"] + Hpl @ Hli @ Hpl.T
    nf = len(free)
    H = np.zeros((nf + 3 * L, nf + 3 * L), LD)
    H[:nf, :nf] = Hpp[np.ix_(free, free)]
    H[:nf, nf:] = Hpl[free]
    H[nf:, :nf] = Hpl[free].T
    H[nf:, nf:] = Hll
    d = 1 / np.sqrt(np.diag(H))   # (inverted scaled: the raw H spans twelve decades)
    Hi = cov_ref.invert(H * d[:, None] * d[None, :]) * d[:, None] * d[None, :]
    A, B = cv["pose_full"][np.ix_(free, free)], Hi[:nf, :nf]
    rel = float(np.abs(A - B).max() / np.abs(B).max())
    assert rel <= 1e-11, f"Sigma_pp: {rel:.2e}"
    worst = 0.0
    for l in range(L):
        B = Hi[nf + 3 * l:nf + 3 * l + 3, nf + 3 * l:nf + 3 * l + 3]
        worst = max(worst, float(np.abs(cv["lm"][l] - B).max() / np.abs(B).max()))
    print(f"tiny: Sigma_pp {rel:.2e}, Sigma_l {worst:.2e} of the full inverse's blocks")
    assert worst <= 1e-11, f"Sigma_l: {worst:.2e}"


def test_free_gauge_is_singular_and_an_anchor_regularises_it():
    """allT without its fixed pose: the scaled S has an eigenvalue below 1e-12 of its largest (what the GPU must
    report as LH_E_SINGULAR); with anchor = 5 the scaled S[f, f] has kappa < 1e4."""
    import lin_ref
    w, _, opts, _ = lin_cases.case("allT")
    w = dict(w, pose_fixed=None)
    R = lin_ref.linearise(w, huber_delta=opts.get("huber_delta", 5.991))
    _, lo, hi = cov_ref.scaled_kappa(R["S"])
    assert lo < 1e-12 * hi, (lo, hi)
    free = np.flatnonzero(np.repeat(~cov_ref.held_poses(w, 5), 6))
    kappa = cov_ref.scaled_kappa(R["S"][np.ix_(free, free)])[0]
    print(f"allT free gauge: lambda_min / lambda_max {lo / hi:.1e}; anchor 5: kappa_scaled {kappa:.1e}")
    assert len(free) == 90 and kappa < 1e4


PROBE = r"""
#include "lh_cov.h"
extern "C" void finish(int n, const double* cl, const double* m, double* out) {
    for (int i = 0; i < n; ++i) lh_cov_lm_finish(cl + 6 * i, m + 6 * i, out + 9 * i);
}
"""


def test_landmark_finish_compiled_for_the_host(tmp_path):
    """lh_cov.h's lh_cov_lm_finish (Sigma_l from the record's Cholesky factor and M) compiled with g++, contraction
    off, on `tiny` and `far` (kappa(H_ll) = 6e6): the factor and M are formed here in double (M from the double
    evaluation's Sigma_pp), and the result is held to the reference at the GPU's bound, max(8 e(double, ref),
    64 eps kappa_scaled)."""
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE)
    so = tmp_path / "probe.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                           os.path.join(ROOT, "lego-slam_amd", "csrc"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.finish.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    for name in ("tiny", "far"):
        w, _, opts, _ = lin_cases.case(name)
        hub = opts.get("huber_delta", 5.991)
        ref = cov_ref.covariance(w, huber_delta=hub)
        dbl = cov_ref.covariance(w, huber_delta=hub, dtype=np.float64)
        R = dbl["R"]
        L, P = len(w["lm_xyz"]), w["n_poses"]
        Cf = np.linalg.cholesky(R["Hll"])
        cl = np.stack([1 / Cf[:, 0, 0], Cf[:, 1, 0], 1 / Cf[:, 1, 1], Cf[:, 2, 0], Cf[:, 2, 1], 1 / Cf[:, 2, 2]], 1)
        # Sigma_pp symmetrised, as the kernels' is (one triangle, mirrored): np.linalg.inv's error is mostly
        # antisymmetric, and the upper triangle of an M formed from it alone carries ten times the error of M's
        # symmetric part (measured on tiny, landmark 3: 5.1e-11 against 3.6e-12)
        F4 = (0.5 * (dbl["pose_full"] + dbl["pose_full"].T)).reshape(P, 6, P, 6)
        m = np.zeros((L, 6))
        iu = np.triu_indices(3)
        for l in range(L):
            idx = np.flatnonzero(R["ol"] == l)
            G = R["Hpl"][idx]
            M = np.einsum("eac,eafb,fbd->cd", G, F4[R["op"][idx]][:, :, R["op"][idx], :], G)
            m[l] = M[iu]
        out = np.zeros((L, 3, 3))
        cl, m = np.ascontiguousarray(cl), np.ascontiguousarray(m)
        lib.finish(L, cl.ctypes.data, m.ctypes.data, out.ctypes.data)
        assert np.array_equal(out, out.transpose(0, 2, 1)), "not exactly symmetric"
        e, l = cov_ref.lm_error(out, ref["lm"])
        e_d, _ = cov_ref.lm_error(dbl["lm"], ref["lm"])
        tol = cov_ref.tolerance(e_d, ref["kappa"])
        print(f"{name}: lh_cov_lm_finish e {e:.2e} (landmark {l}), double evaluation {e_d:.2e}, bound {tol:.2e}")
        assert e <= tol, f"{name}: landmark {l}: e = {e:.3e} > {tol:.3e}"
