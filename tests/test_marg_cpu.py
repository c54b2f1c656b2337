"""CPU tests of lh_marginalize's boundary and of its reference (include/lego_ba.h): the ctypes mirrors
of its two structs against a compiled C program; the symbol; lh_marg.h's plain-C++ elimination, compiled with g++,
against NumPy; and tests/marg_ref.py's own consistency (marginalising is taking the covariance's sub-block; an earlier
prior against the dense computation; the landmark sets).  No GPU call is made here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import cov_ref
import lego_ba
import lin_cases
import marg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"lh_marg_input": "LhMargInput", "lh_marg_result": "LhMargResult"}
LD = marg_ref.LD


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


def test_symbol_is_declared_bound_and_exported():
    lib = lego_ba.ba_lib()
    hdr = open(os.path.join(ROOT, "include", "lego_ba.h")).read()
    assert "lh_marginalize" in lego_ba.ABI_SYMBOLS and hasattr(lib, "lh_marginalize")
    assert re.search(r"\bint\s+lh_marginalize\s*\(\s*lh_handle\s*\*", hdr)
    assert lib.lh_marginalize.argtypes is not None and hasattr(lego_ba.Solver, "marginalize")
    assert re.search(r"#define\s+LH_ABI_VERSION\s+5\b", hdr) and lego_ba.LH_ABI_VERSION == 5


PROBE = r"""
#include "lh_marg.h"
// H [n][n] and g [n] from the symmetric A [n][n] (lower triangle read), b [n] and the block at rows 6 m: the route of
// k_marg_assemble and k_marg_schur.  Returns lh_marg_chol6's status; piv: min and max pivot.
extern "C" int eliminate(int n, int m, const double* A, const double* b, double* Y, double* H, double* g, double* piv) {
    double a[36], c[36], y[6];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            const int r = 6 * m + (i > j ? i : j), s = 6 * m + (i > j ? j : i);
            a[6 * i + j] = A[(long)r * n + s];
        }
    const int bad = lh_marg_chol6(a, c, piv, piv + 1);
    if (bad >= 0) return bad;
    for (int col = 0; col < n; ++col) {
        for (int k = 0; k < 6; ++k) {
            const int r = 6 * m + k;
            Y[(long)k * n + col] = r > col ? A[(long)r * n + col] : A[(long)col * n + r];
        }
        lh_marg_fwd6(c, Y + col, n);
    }
    for (int k = 0; k < 6; ++k) y[k] = b[6 * m + k];
    lh_marg_fwd6(c, y, 1);
    for (int r = 0; r < n; ++r) {
        const bool rm = r / 6 == m;
        g[r] = rm ? 0.0 : lh_marg_update(b[r], Y + r, y, n, 1);
        for (int s = 0; s < n; ++s) {
            const double av = r > s ? A[(long)r * n + s] : A[(long)s * n + r];
            H[(long)r * n + s] = (rm || s / 6 == m) ? 0.0 : lh_marg_update(av, Y + r, Y + s, n, n);
        }
    }
    return -1;
}
"""


def _probe(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE)
    so = tmp_path / "probe.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                           os.path.join(ROOT, "lego-slam_amd", "csrc"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.eliminate.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 6
    return lib


def test_elimination_compiled_for_the_host(tmp_path):
    """lh_marg.h's factor, forward substitution and update, compiled with g++, on random SPD systems of 2..9 poses with
    the block condition number up to 1e6: H and g against the long-double Schur complement within 64 eps kappa of
    the eliminated block (scaled error); H equals its transpose by bits; m's rows are +0.0; a block whose third pivot is
    not positive is reported at row 2."""
    lib = _probe(tmp_path)
    rng = np.random.default_rng(7)
    for trial in range(12):
        P = int(rng.integers(2, 10))
        n, m = 6 * P, int(rng.integers(0, P))
        Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
        A = (Q * np.logspace(0, rng.uniform(1, 6), n)) @ Q.T
        A = np.tril(A) + np.tril(A, -1).T
        b = rng.standard_normal(n)
        Al = np.tril(A) + np.triu(rng.standard_normal((n, n)), 1)   # (the upper triangle is not read)
        Y, H, g, piv = np.zeros((6, n)), np.full((n, n), -7.0), np.full(n, -7.0), np.zeros(2)
        assert lib.eliminate(n, m, Al.ctypes.data, b.ctypes.data, Y.ctypes.data, H.ctypes.data, g.ctypes.data, piv.ctypes.data) == -1
        mm = np.arange(6 * m, 6 * m + 6)
        r = np.setdiff1d(np.arange(n), mm)
        Ai = cov_ref.invert(A[np.ix_(mm, mm)])
        Ar = A.astype(LD)
        Href = Ar[np.ix_(r, r)] - Ar[np.ix_(r, mm)] @ Ai @ Ar[np.ix_(mm, r)]
        gref = b[r] - Ar[np.ix_(r, mm)] @ (Ai @ b[mm])
        kappa = cov_ref.scaled_kappa(A[np.ix_(mm, mm)])[0]
        d = np.sqrt(np.diag(Href).astype(np.float64))
        # (the entries of A[r, r] before the cancellation set the scale of the rounding: sqrt(A_ii A_jj))
        da = np.sqrt(np.diag(A)[r])
        e = float((np.abs((H[np.ix_(r, r)] - Href).astype(np.float64)) / da[:, None] / da[None, :]).max())
        eg = float((np.abs((g[r] - gref).astype(np.float64)) / da).max() / (np.abs(b).max() / da.min()))
        assert e <= 64 * marg_ref.EPS * kappa and eg <= 64 * marg_ref.EPS * kappa, (trial, e, eg, kappa)
        assert (d > 0).all()
        assert np.array_equal(H.view(np.uint64), H.T.copy().view(np.uint64)), "H is not its transpose by bits"
        assert not H[mm].view(np.uint64).any() and not H[:, mm].view(np.uint64).any() and not g[mm].view(np.uint64).any()
        assert 0 < piv[0] <= piv[1]
    # an indefinite block: the pivot of row 2 is not > 0
    n, m = 12, 1
    A = np.eye(n)
    A[8, 8] = -1.0
    out = [np.zeros((6, n)), np.zeros((n, n)), np.zeros(n), np.zeros(2)]
    assert lib.eliminate(n, m, A.ctypes.data, np.zeros(n).ctypes.data, *[a.ctypes.data for a in out]) == 2


def test_marginalising_is_the_covariance_sub_block():
    """Where every landmark is in M and another pose is fixed (cams4 m = 1, tiny m = 1), the inverse of H_prior over
    its non-zero rows is cov_ref.covariance's Sigma_pp on those rows, to 1e-11 in the scaled error."""
    for name, m in (("cams4", 1), ("tiny", 1)):
        w, _, opts, _ = lin_cases.case(name)
        hub = opts.get("huber_delta", 5.991)
        ref = marg_ref.marginalize(w, m, huber_delta=hub)
        assert ref["in_M"].all() and ref["n_degenerate"] == 0 and ref["n_edges"] == len(w["obs_pose"]), name
        cv = cov_ref.covariance(w, huber_delta=hub)
        rows = ref["rows"]
        assert np.array_equal(rows, np.setdiff1d(cv["free"], np.arange(6 * m, 6 * m + 6))), name
        X = cov_ref.invert(ref["H"][np.ix_(rows, rows)])
        full = np.zeros_like(cv["pose_full"])
        full[np.ix_(rows, rows)] = X
        e, pq = cov_ref.pose_error(full, cv["pose_full"], rows)
        print(f"{name}: inv(H_prior) against Sigma_pp[r, r]: e = {e:.2e} (poses {pq})")
        assert e <= 1e-11, (name, e, pq)


def test_strict_subsets_and_layout():
    """allT m = 1 and outl m = 9 marginalise strict subsets of the landmarks; the rows of m, of the fixed poses and of
    the poses that share no landmark with m are exactly zero, every other diagonal is positive."""
    for name, m in (("allT", 1), ("outl", 9), ("fixedmid", 7)):
        w, _, opts, _ = lin_cases.case(name)
        ref = marg_ref.marginalize(w, m, huber_delta=opts.get("huber_delta", 5.991), dtype=np.float64)
        L, P = len(w["lm_xyz"]), w["n_poses"]
        assert 0 < ref["n_landmarks"] < L, (name, ref["n_landmarks"], L)
        op, ol = np.asarray(w["obs_pose"], np.int64), np.asarray(w["obs_lm"], np.int64)
        involved = np.zeros(P, bool)
        involved[op[ref["in_M"][ol]]] = True
        involved &= ~ref["fixed"]
        involved[m] = False
        print(f"{name} m={m}: {ref['n_landmarks']} of {L} landmarks, {ref['n_edges']} edges, {int(involved.sum())} poses involved, "
              f"kappa {ref['kappa']:.1e}")
        assert np.array_equal(ref["rows"], np.flatnonzero(np.repeat(involved, 6))), name
        assert (np.diag(ref["H"])[ref["rows"]] > 0).all()
        out = np.repeat(~involved, 6)
        assert not ref["H"][out].any() and not ref["H"][:, out].any() and not ref["b"][out].any()


def test_earlier_prior_against_the_dense_computation():
    """With a random SPD prior_H (scaled to A's diagonal) and a random prior_b, the result is the Schur complement of
    the dense sum A_M + prior, the fixed pose's rows and columns of the prior zeroed first."""
    w, _, opts, _ = lin_cases.case("allT")
    m, hub = 1, opts.get("huber_delta", 5.991)
    P = w["n_poses"]
    A0, b0, info = marg_ref.system(w, m, huber_delta=hub)
    H0, g0 = marg_ref.random_prior(P, A0, b0, seed=3)
    ref = marg_ref.marginalize(w, m, huber_delta=hub, prior=(H0, g0))
    live = np.repeat(~info["fixed"], 6)
    A = A0 + np.where(live[:, None] & live[None, :], H0, 0).astype(LD)
    b = b0 + np.where(live, g0, 0).astype(LD)
    mm = np.arange(6 * m, 6 * m + 6)
    r = np.setdiff1d(np.arange(6 * P), mm)
    # the dense route: the block of the inverse, inverted back (over the live rows)
    lr = np.flatnonzero(live)
    Ainv = np.zeros_like(A)
    Ainv[np.ix_(lr, lr)] = cov_ref.invert(A[np.ix_(lr, lr)])
    keep = np.setdiff1d(lr, mm)
    Hd = cov_ref.invert(Ainv[np.ix_(keep, keep)])
    assert np.array_equal(ref["rows"], keep)   # (the prior reaches every live pose)
    d = np.sqrt(np.diag(Hd).astype(np.float64))
    e = float((np.abs((ref["H"][np.ix_(keep, keep)] - Hd).astype(np.float64)) / d[:, None] / d[None, :]).max())
    gd = Hd @ (Ainv[np.ix_(keep, lr)] @ b[lr])
    eg = float((np.abs((ref["b"][keep] - gd).astype(np.float64)) / d).max() / marg_ref.rhs_scale(ref))
    print(f"allT m=1 with an earlier prior: H {e:.2e}, b {eg:.2e} from the dense computation")
    assert e <= 1e-10 and eg <= 1e-10, (e, eg)
    assert not ref["H"][~live].any() and not ref["H"][:, ~live].any()
