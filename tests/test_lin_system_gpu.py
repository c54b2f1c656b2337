"""k_lin + k_reduce's reduced pose system, block by block, against the long-double linearisation (tests/lin_ref.py).

The staged system (lh_rs_layout: the 6x6 blocks of S = H_pp - H_pl H_ll^-1 H_lp, b_s, b_p, diag H_pp, the chunk
scalars) is read back through lh_debug_reduced_system and decoded here with lh_rs_make's offsets and the planner's
pair list.  The cases and what each reaches: tests/lin_cases.py (their planner shapes are asserted on the CPU,
tests/test_lin_ref_cpu.py).  Every case runs in both layouts k_reduce writes S in: `packed` (LH_NO_IMG, LH_NO_BIMG:
the blocks of the packed buffer) and `image` (the default of these windows: k_ctrl's LDS image or k_ctrl_b's band
image, hook buffer 3; b_s, b_p, diag H_pp and the scalars are in the packed buffer either way).

Test A  the initial linearisation (k_lin<T, false>, k_reduce mode 0): max_iters = 0.
Test B  a trial's re-linearisation (k_lin<T, true>): LH_NO_EVO, LH_NO_LADDER, LH_NO_BATCH, max_iters = max_trials = 1,
        the trial accepted.  With LH_NO_EVO ctrl_lm_step leaves evo 0, so the trial's k_lin linearises the candidate
        in full and k_reduce (mode 1, evo 0) writes that system to the staged side; the decision stops the loop, so
        the controller returns before anything copies or overwrites it (k_ctrl: `if (done || skip) return`), and the
        chain the host may have enqueued past it exits on ctrl->done.  The staged buffer (hook buffer 0, not 1) is
        therefore the linearisation at the candidate, and the candidate is the state the solve returns: the reference
        and the oracle yardstick are evaluated at the GPU's returned poses and landmarks.
Test C  the same run's candidate: the pending pose step dx_p (hook buffer 2) is the step the trial applied (a stopped
        controller solves no new one).  From the INPUT state in long double, X' = X + H_ll^-1 (b_l - H_lp dx_p) and
        T' = exp(dx_p) T; the returned landmarks are held to 32 eps kappa_2(H_ll) (|d| + |H_ll^-1| (|b_l| +
        sum_e |H_lp,e dx_p|)) + 4 eps |X| each, the poses to 64 eps per rotation entry and 64 eps (1 + |t|) per
        translation entry.

Tolerance of S and b_s (A and B): MARGIN = 8 x the largest distance of the double-precision oracle from the same
reference over 1, 2 and 8 threads, on that case and state, computed at run time; floor 64 eps.  b_p, diag H_pp and
sum rho0: the a-priori summation bound (n + 16) eps sum |terms| (lin_ref.linearise; why the terms count both
operands of r = uv - proj: tests/test_lin_ref_cpu.py).  max |diag H_ll|: 16 eps relative.  Rank-deficient landmarks:
exactly 0.  Rows and columns of fixed poses: k_lin adds nothing for a fixed pose (lin_blocks returns early), so every
entry k_reduce writes there is an exact zero, which the controllers rely on (a zero row takes lambda alone on its
diagonal and yields a zero step): asserted as exact zeros.  A failing block is named by its pose pair.

Measured e_GPU / e_oracle, S | b_s (MI355X; both layouts give the same bits; also DESIGN.md 4.5).  Worst 2.83 (far:
the landmark Cholesky against the oracle's LU inverse at kappa(H_ll) = 6e6), so MARGIN stays 8:

    case       A: initial     B: trial       e_oracle(S) at A
    allT       1.01 | 0.96    1.58 | 1.00    9.5e-15
    manysb     0.67 | 0.91    1.39 | 1.00    6.9e-15
    fixedmid   1.01 | 0.96    2.11 | 1.00    9.5e-15
    outl       0.47 | 1.02    0.12 | 0.06    7.4e-15
    far        2.83 | 2.43    0.86 | 0.27    3.2e-13
    cams4      0.81 | 1.10    0.57 | 0.99    2.7e-15
    p70        1.57 | 1.09    0.73 | 0.41    7.5e-14
    nohuber    1.01 | 0.96    0.77 | 1.00    9.5e-15
    tiny       0.47 | 0.18    0.75 | 0.67    1.5e-13

Test C: rotations within 0.2 eps, translations within 2.5 eps (1 + |t|), landmarks within 0.5 % of their bound.
The first run of Test A found max |diag H_ll| of `tiny` at a third of its value: wave_max's lane ^ 4 step
(lego-slam_amd/csrc/lh_dev.h), fixed with it.
"""
import numpy as np
import pytest

import lego_ba
import lin_cases
import lin_ref
import oracle_bind as ob

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
MARGIN = 8.0
THREADS = (1, 2, 8)
IMG_AS, IMG_NPAD = 130, 128      # LH_IMG_AS, LH_NPAD (lego-slam_amd/csrc/lh_common.h)
BIMG_TR = 16 * 128               # LH_BIMG_TR

CASES = list(lin_cases.CASES)
LAYOUTS = ("packed", "image")

_ref0 = {}


def huber(opts):
    return opts.get("huber_delta", 5.991)


def reference0(name):
    """The long-double linearisation at the case's input state and the oracle's distances from it: once per case."""
    if name not in _ref0:
        w, _, opts, _ = lin_cases.case(name)
        R = lin_ref.linearise(w, huber_delta=huber(opts))
        _ref0[name] = (R, oracle_distance(w, opts, R))
    return _ref0[name]


def oracle_distance(w, opts, R):
    es, eb = [], []
    for t in THREADS:
        S, bs, _ = ob.reduced_system(w, n_threads=t, **opts)
        es.append(lin_ref.block_error(S, R["S"], R["fixed"])[0])
        eb.append(lin_ref.rhs_error(bs, R)[0])
    return max(es), max(eb)


def set_layout(monkeypatch, layout):
    for v in ("LH_NO_IMG", "LH_NO_BIMG"):
        if layout == "packed":
            monkeypatch.setenv(v, "1")
        else:
            monkeypatch.delenv(v, raising=False)


def decode_image(img, P, S_ref):
    """S (both triangles) from the staged half of k_reduce's image: k_ctrl's LDS layout (S(r, c), r >= c, at
    r LH_IMG_AS + c; b_s in row LH_NPAD) or k_ctrl_b's band image (lh_bimg_idx).  An entry outside k_ctrl_b's band has
    no slot: the reference must hold an exact zero there, which it then keeps."""
    n = 6 * P
    S = np.zeros((n, n))
    r, c = np.tril_indices(n)
    if len(img) == (IMG_NPAD + 1) * IMG_AS:
        S[r, c] = img[r * IMG_AS + c]
        bs = img[IMG_NPAD * IMG_AS:IMG_NPAD * IMG_AS + n].copy()
    else:
        assert len(img) == ((n + 15) >> 4) * BIMG_TR, len(img)
        o = c - 16 * ((r >> 4) - 7)
        inb = (o >= 0) & (o < 128)
        S[r[inb], c[inb]] = img[(r[inb] >> 4) * BIMG_TR + (r[inb] & 15) * 128 + o[inb]]
        assert not S_ref[r[~inb], c[~inb]].any(), "the reference has a nonzero outside k_ctrl_b's band"
        bs = None
    S = S + np.tril(S, -1).T
    return S, bs


def read_system(s, w, chunk, layout, R):
    """The staged system of solver `s` as (S, bs, bp, hd, scalars), S from the layout under test."""
    P = w["n_poses"]
    pair_pq = lin_cases.plan_shapes(w, chunk)["pair_pq"]
    v, npairs = s.reduced_system(0)
    assert npairs == len(pair_pq), (npairs, len(pair_pq))
    S, bs, bp, hd, sc = lin_cases.decode_packed(v, P, pair_pq)
    # a pose pair the planner lists no block for must be an exact zero of the reference
    listed = np.zeros((P, P), bool)
    listed[pair_pq[:, 0], pair_pq[:, 1]] = listed[pair_pq[:, 1], pair_pq[:, 0]] = True
    Rb = np.abs(R["S"]).reshape(P, 6, P, 6).max((1, 3))
    assert not Rb[~listed].any(), "the planner's pair list misses a coupled pose pair"
    img, _ = s.reduced_system(3)
    if layout == "packed":
        assert len(img) == 0, "LH_NO_IMG / LH_NO_BIMG: no image expected"
    else:
        assert len(img) > 0, "the case's controller reads no image: nothing to test in this layout"
        S, bs_img = decode_image(img, P, np.asarray(R["S"], np.float64))
        if bs_img is not None:
            assert np.array_equal(bs_img, bs), "the image's rhs row differs from the packed b_s"
    return S, bs, bp, hd, sc


def check_system(tag, name, got, R, orc):
    """Every quantity of the staged system against reference R; orc: the oracle's (e(S), e(b_s)) at the same state."""
    S, bs, bp, hd, sc = got
    e_orc, eb_orc = orc
    fx = np.repeat(R["fixed"], 6)
    assert not S[fx].any() and not S[:, fx].any(), f"{name}: a fixed pose's row or column of S is not exactly zero"
    assert not bs[fx].any() and not bp[fx].any() and not hd[fx].any(), f"{name}: a fixed pose's b_s, b_p or diag H_pp"
    e, pq = lin_ref.block_error(S, R["S"], R["fixed"])
    eb, row = lin_ref.rhs_error(bs, R)
    tol, tolb = max(MARGIN * e_orc, 64 * EPS), max(MARGIN * eb_orc, 64 * EPS)
    print(f"RATIO {tag} {name}: S e_gpu {e:.2e} e_oracle {e_orc:.2e} ratio {e / e_orc:.2f} (pair {pq}) | "
          f"b_s e_gpu {eb:.2e} e_oracle {eb_orc:.2e} ratio {eb / eb_orc:.2f} (row {row})")
    d_bp = np.abs((bp - R["bp"]).astype(np.float64))
    d_hd = np.abs((hd - R["hd"]).astype(np.float64))
    d_chi = abs(float(sc[0] - R["chi2"]))
    d_maxd = abs(float(sc[3] - R["maxd"])) / float(R["maxd"])
    live = ~fx
    print(f"      b_p {np.max(d_bp[live] / R['bp_bound'][live]):.3f} diag H_pp {np.max(d_hd[live] / R['hd_bound'][live]):.3f} "
          f"sum rho0 {d_chi / R['chi2_bound']:.3f} of their bounds; max |diag H_ll| {d_maxd / EPS:.1f} eps; ndeg {sc[2]}")
    assert e <= tol, (f"{name}: S block of pose pair {pq}: e = {e:.3e} > {tol:.3e} "
                      f"({e / e_orc:.1f} x the oracle's {e_orc:.2e})")
    assert eb <= tolb, f"{name}: b_s row {row} (pose {row // 6}): e = {eb:.3e} > {tolb:.3e}"
    bad = np.flatnonzero(d_bp > R["bp_bound"])
    assert len(bad) == 0, f"{name}: b_p rows {bad} (poses {np.unique(bad // 6)}) past (n_p + 16) eps sum |terms|"
    bad = np.flatnonzero(d_hd > R["hd_bound"])
    assert len(bad) == 0, f"{name}: diag H_pp rows {bad} (poses {np.unique(bad // 6)}) past (n_p + 16) eps sum |terms|"
    assert d_chi <= R["chi2_bound"], f"{name}: sum rho0 off by {d_chi:.3e} > {R['chi2_bound']:.3e}"
    assert d_maxd <= 16 * EPS, f"{name}: max |diag H_ll| off by {d_maxd / EPS:.1f} eps"
    assert sc[2] == 0.0, f"{name}: {sc[2]} rank-deficient landmarks"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", CASES)
def test_initial_linearisation(name, layout, monkeypatch):
    """Test A."""
    w, chunk, opts, _ = lin_cases.case(name)
    R, orc = reference0(name)
    set_layout(monkeypatch, layout)
    s = lego_ba.Solver(max_iters=0, chunk_landmarks=chunk, **opts)
    try:
        g = s.solve(w)
        assert g["degenerate"] == 0 and g["trials"] == 0
        got = read_system(s, w, chunk, layout, R)
    finally:
        s.close()
    check_system("A/" + layout, name, got, R, orc)


def test_hook_arguments():
    """LH_E_BADARG without an uploaded window, for a buffer that does not exist and for too small a capacity."""
    import ctypes as C
    w, chunk, opts, _ = lin_cases.case("tiny")
    s = lego_ba.Solver(max_iters=0, chunk_landmarks=chunk, **opts)
    try:
        with pytest.raises(lego_ba.LhError) as ei:
            s.reduced_system(0)
        assert ei.value.status == lego_ba.LH_E_BADARG
        s.solve(w)
        v, npairs = s.reduced_system(0)
        assert npairs == 6 and len(v) == lin_cases.rs_offsets(3, 6)["total"]
        assert len(s.reduced_system(1)[0]) == len(v) and len(s.reduced_system(2)[0]) == 18
        n, npo = C.c_int64(0), C.c_int32(0)
        small = np.full(len(v), -7.0)
        f = lego_ba.ba_lib().lh_debug_reduced_system
        assert f(s.h, 0, small.ctypes.data, len(v) - 1, C.byref(n), C.byref(npo)) == lego_ba.LH_E_BADARG
        assert n.value == len(v) and (small == -7.0).all()   # the size is reported, nothing is written
        assert f(s.h, 4, small.ctypes.data, len(v), C.byref(n), C.byref(npo)) == lego_ba.LH_E_BADARG
    finally:
        s.close()


_trial = {}


def trial_run(name, layout, monkeypatch):
    """One accepted trial under LH_NO_EVO, LH_NO_LADDER, LH_NO_BATCH: (result, staged system, dx_p); once per
    (case, layout), shared by tests B and C."""
    if (name, layout) not in _trial:
        w, chunk, opts, _ = lin_cases.case(name)
        set_layout(monkeypatch, layout)
        for v in ("LH_NO_EVO", "LH_NO_LADDER", "LH_NO_BATCH"):
            monkeypatch.setenv(v, "1")
        s = lego_ba.Solver(max_iters=1, max_trials=1, chunk_landmarks=chunk, **opts)
        try:
            g = s.solve(w)
            assert g["accepted"] == 1 and g["trials"] == 1, (g["accepted"], g["trials"])   # the precondition
            R1 = lin_ref.linearise(w, pose=g["pose_Tcw"], lm=g["lm_xyz"], huber_delta=huber(opts))
            got = read_system(s, w, chunk, layout, R1)
            dxp, _ = s.reduced_system(2)
        finally:
            s.close()
        _trial[(name, layout)] = (g, got, dxp, R1)
    return _trial[(name, layout)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", CASES)
def test_trial_linearisation(name, layout, monkeypatch):
    """Test B.  (Every case's first trial is accepted by the oracle, ob.solve(w, max_iters=1, max_trials=1).)"""
    w, _, opts, _ = lin_cases.case(name)
    g, got, _, R1 = trial_run(name, layout, monkeypatch)
    orc = oracle_distance(dict(w, pose_Tcw=g["pose_Tcw"], lm_xyz=g["lm_xyz"]), opts, R1)
    check_system("B/" + layout, name, got, R1, orc)


@pytest.mark.parametrize("name", CASES)
def test_trial_candidate(name, monkeypatch):
    """Test C."""
    w, _, opts, _ = lin_cases.case(name)
    g, _, dxp, _ = trial_run(name, "image", monkeypatch)
    R0, _ = reference0(name)
    P, L = w["n_poses"], len(w["lm_xyz"])
    assert len(dxp) == 6 * P
    dx = np.asarray(dxp, lin_ref.LD).reshape(P, 6)
    assert not dx[R0["fixed"]].any(), "a fixed pose has a step"
    # poses: T' = exp(dx_p) T
    T1 = lin_ref.left_update(dx, w["pose_Tcw"]).reshape(P, 3, 4)
    G = np.asarray(g["pose_Tcw"]).reshape(P, 3, 4)
    dR = np.abs((G[:, :, :3] - T1[:, :, :3]).astype(np.float64))
    dt = np.abs((G[:, :, 3] - T1[:, :, 3]).astype(np.float64))
    tn = np.sqrt((T1[:, :, 3].astype(np.float64) ** 2).sum(1))
    print(f"CAND {name}: rotation {dR.max() / EPS:.1f} eps, translation {np.max(dt / (1 + tn)[:, None]) / EPS:.1f} eps (1 + |t|)")
    p = int(np.argmax(dR.max((1, 2))))
    assert dR.max() <= 64 * EPS, f"{name}: pose {p} rotation off by {dR.max() / EPS:.1f} eps"
    p = int(np.argmax((dt / (1 + tn)[:, None]).max(1)))
    assert (dt <= 64 * EPS * (1 + tn)[:, None]).all(), f"{name}: pose {p} translation past 64 eps (1 + |t|)"
    # landmarks: X' = X + H_ll^-1 (b_l - H_lp dx_p), H_lp,e = H_pl,e^T
    ol, op = R0["ol"], R0["op"]
    hd = np.einsum("oak,oa->ok", R0["Hpl"], dx[op])
    t = R0["bl"].copy()
    np.add.at(t, ol, -hd)
    d = np.einsum("lij,lj->li", R0["Hinv"], t)
    X0 = np.asarray(w["lm_xyz"], lin_ref.LD)
    X1 = X0 + d
    nrm = lambda a: np.sqrt((np.asarray(a, np.float64) ** 2).sum(-1))
    shd = np.zeros(L)
    np.add.at(shd, ol, nrm(hd))
    bound = 32 * EPS * R0["kappa"] * (nrm(d) + R0["hinv_norm"] * (nrm(R0["bl"]) + shd)) + 4 * EPS * nrm(X0)
    err = nrm(np.asarray(g["lm_xyz"]) - X1)
    l = int(np.argmax(err / bound))
    print(f"CAND {name}: landmarks at most {np.max(err / bound):.3f} of their bound (landmark {l}, kappa {R0['kappa'][l]:.1e})")
    assert (err <= bound).all(), f"{name}: landmark {l}: |dX| = {err[l]:.3e} > {bound[l]:.3e} (kappa {R0['kappa'][l]:.1e})"
