"""CPU tests of the C-ABI boundary (include/lego_ba.h): the shared library
loads and exports every declared symbol, the ctypes structs match the C
layout, option defaults mirror the reference constants, and the host-only
Backend::Optimize outlier pass (backend_lego.cpp:163-194) is exact.
No compute call is made here (no GPU in this container)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lego_ba

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lego_ba.h")


def declared_functions():
    txt = open(HDR).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(lh_\w+)\s*\(", txt, re.M)))


def test_library_loads_and_exports_every_header_symbol():
    lib = lego_ba.ba_lib()
    decl = declared_functions()
    assert len(decl) >= 12
    assert set(lego_ba.ABI_SYMBOLS) <= set(decl)
    for name in decl:
        assert hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", lego_ba.BA_LIB], capture_output=True, text=True).stdout
    for name in decl:
        assert re.search(rf"\bT {name}\b", out), name


def test_no_hipify_or_dual_paths_in_sources():
    src = os.path.join(ROOT, "lego-slam_amd", "csrc")
    for f in os.listdir(src):
        txt = open(os.path.join(src, f)).read()
        assert "__HIP_PLATFORM_AMD__" not in txt and "cuda" not in txt.lower(), f


# the fields the hand-written layout program checked before it was generated: the generated one covers at least these
EARLIER_FIELDS = {
    "lh_frames": "obs_ptr is_outlier K", "lh_frames_result": "iterations time_ms",
    "lh_options": "huber_delta linear_solver comm_id profile pcg_max_iters pcg_tol gate_mode chunk_landmarks comm_mode "
                  "host_threads allreduce allreduce_user precision",
    "lh_window": "n_obs K cam_ext",
    "lh_result": "trace_cap chi2_initial time_ms pcg_iterations degenerate time_prep_ms time_upload_ms time_download_ms "
                 "is_outlier outlier_chi2_th outlier_th n_inlier n_outlier",
}


def mirrored_structs():
    """{C name: class} of every ctypes.Structure lego_ba mirrors from include/lego_ba.h: LhFooBar is lh_foo_bar.
    (LhwParams mirrors the window generator's header, not this one.)"""
    return {re.sub(r"(?<!^)([A-Z])", r"_\1", name).lower(): c for name, c in vars(lego_ba).items()
            if isinstance(c, type) and issubclass(c, C.Structure) and c is not C.Structure and name != "LhwParams"}


def test_ctypes_struct_layout_matches_header(tmp_path):
    """sizeof of every mirrored struct and offsetof of every field, as a C compiler sees the header.  On a mismatch the
    header is right."""
    structs = mirrored_structs()
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "lego_ba.h"', "int main(void) {"]
    for s, c in structs.items():
        lines.append(f'  printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'  printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f, *_ in c._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    fields = {key for key in got if "." in key}
    assert len(got) - len(fields) == len(structs) >= 22
    assert len(fields) == sum(len(c._fields_) for c in structs.values())
    assert {f"{s}.{f}" for s, names in EARLIER_FIELDS.items() for f in names.split()} <= fields
    assert len(fields) >= 36
    assert {"lh_options", "lh_window", "lh_result", "lh_kernel_stats", "lh_frames", "lh_frames_result"} <= set(structs)
    for key, v in got.items():
        if "." in key:
            s, f = key.split(".")
            assert getattr(structs[s], f).offset == v, key
        else:
            assert C.sizeof(structs[key]) == v, key


def test_default_options_are_keyed_on_the_callers_abi():
    """A binary built against the ABI-4 header calls the plain symbol lh_default_options: it gets abi_version 4, so
    the library never reads the ABI-5 lh_result fields its smaller struct lacks.  The header maps
    lh_default_options(&o) to lh_default_options_v(&o, LH_ABI_VERSION), the caller's compile-time version."""
    lib = lego_ba.ba_lib()
    o = lego_ba.LhOptions()
    o.abi_version = 99
    lib.lh_default_options(C.byref(o))
    assert o.abi_version == 4 and o.max_iters == 10 and o.huber_delta == 5.991
    lib.lh_default_options_v(C.byref(o), 5)
    assert o.abi_version == 5 and o.max_iters == 10
    hdr = open(os.path.join(ROOT, "include", "lego_ba.h")).read()
    assert "#define lh_default_options(opt) lh_default_options_v((opt), LH_ABI_VERSION)" in hdr


def test_default_options_mirror_reference_constants():
    o = lego_ba.default_options()
    assert o.abi_version == lego_ba.LH_ABI_VERSION == 5
    assert o.precision == lego_ba.LH_PREC_FP64          # double throughout: the residual mirrors the reference
    assert o.gate_mode == 0 and o.degenerate_guard == 0   # the reference's Huber gate and LU semantics
    assert o.comm_mode == lego_ba.LH_COMM_RCCL and o.chunk_landmarks == 0 and not o.allreduce
    assert o.linear_solver == lego_ba.LH_SOLVER_LDLT   # Eigen LDLT     problem.cpp:420
    assert o.pcg_tol == 1e-6 and o.pcg_max_iters <= 0   # PCGSolver stop rule / cap  problem.cpp:597, :422
    assert o.max_iters == 10          # problem.solve(10)      backend_lego.cpp:161
    assert o.max_trials == 10         # false_cnt_threshold    problem.cpp:178
    assert o.huber_delta == 5.991     # HuberCost(chi2_th)     backend_lego.cpp:92-94
    assert o.stop_dchi2 == 1e-5       # diffChiThreshold_      problem.h:165
    assert o.tau == 1e-5 and o.lambda_cap == 5e10   # problem.cpp:494-495
    assert o.lambda_init < 0 and o.strategy == 0 and o.world_size == 1


def test_strerror():
    lib = lego_ba.ba_lib()
    for st in range(7):
        assert lib.lh_strerror(st)
    assert b"empty" in lib.lh_strerror(lego_ba.LH_E_EMPTY)


def reference_outlier_pass(rchi2, chi2_th):
    """Python transcription of backend_lego.cpp:163-194."""
    cnt_out = cnt_in = 0
    iteration = 0
    while iteration < 5:
        cnt_out = int(np.sum(rchi2 > chi2_th))
        cnt_in = len(rchi2) - cnt_out
        ratio = cnt_in / float(cnt_in + cnt_out) if (cnt_in + cnt_out) else float("nan")
        if ratio > 0.5:
            break
        chi2_th *= 2
        iteration += 1
    return rchi2 > chi2_th, chi2_th, cnt_in, cnt_out


@pytest.mark.parametrize("frac", [0.0, 0.3, 0.6, 0.9, 1.0])
def test_classify_outliers_matches_backend(frac):
    rng = np.random.default_rng(int(frac * 10))
    n = 1000
    r = rng.uniform(0, 5.0, n)
    m = rng.random(n) < frac
    r[m] = rng.uniform(6.0, 400.0, m.sum())
    flags, th, ni, no = lego_ba.classify_outliers(r)
    rf, rth, rni, rno = reference_outlier_pass(r, 5.991)
    assert np.array_equal(flags, rf) and th == rth and (ni, no) == (rni, rno)


def test_classify_outliers_empty():
    flags, th, ni, no = lego_ba.classify_outliers(np.zeros(0))
    assert th == 5.991 * 32 and ni == 0 and no == 0
