// lh_host.cpp — C ABI (include/lego_ba.h) of the MI355X BA solver: the handle's life (lh_handle.h), the upload of
// a window (lh_plan.cpp preprocessing into pinned staging, one async copy per array), the LM launch loop, the per-trial
// exchange of a landmark-sharded solve, the download of the results.  (The frontend entry points: lh_frontend.cpp and
// lh_frame.cpp; lh_covariance: lh_cov_host.cpp.)
//
// Per solve nothing but kernel launches happens on the host: the whole LM loop (accept/reject,
// lambda schedule, stop rule) runs on the device, and the host keeps `depth` trials enqueued ahead
// of the device's progress word.  With >1 rank each trial carries one all-reduce of the packed
// reduced pose system; every rank issues exactly the same number of them (lh_plan.h, the trial schedule).
#include <sched.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>

#include "lh_frontend_layout.h"
#include "lh_handle.h"
#include "lh_launch.h"

using namespace lh;

hipEvent_t lh::next_event(lh_handle* h) {
    if (h->event_next == h->event_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        h->event_pool.push_back(e);
    }
    return h->event_pool[h->event_next++];
}

void lh::par_copy(lh_handle* h, const ByteSeg* seg, int nseg) {
    const size_t blk = 262144;
    size_t total = 0;
    for (int k = 0; k < nseg; ++k) total += (seg[k].dst && seg[k].src) ? seg[k].n : 0;
    if (total < 4 * blk) {   // waking the pool costs more than copying a small call's bytes
        for (int k = 0; k < nseg; ++k)
            if (seg[k].dst && seg[k].src && seg[k].n) std::memcpy(seg[k].dst, seg[k].src, seg[k].n);
        return;
    }
    std::vector<std::pair<int, size_t>> jobs;
    for (int k = 0; k < nseg; ++k)
        if (seg[k].dst && seg[k].src)
            for (size_t o = 0; o < seg[k].n; o += blk) jobs.emplace_back(k, o);
    auto job = [&](int j) {
        const ByteSeg& g = seg[jobs[j].first];
        const size_t o = jobs[j].second, c = std::min(blk, g.n - o);
        std::memcpy((uint8_t*)g.dst + o, (const uint8_t*)g.src + o, c);
    };
    if (h->pool && jobs.size() > 1) h->pool->run((int)jobs.size(), job);
    else for (int j = 0; j < (int)jobs.size(); ++j) job(j);
}

namespace {

const char* kKernelNames[KC_N] = {"k_lin", "k_reduce", "k_ctrl", "allreduce", "k_lin_init", "", "", ""};

// ---- Eigen quaternion <-> matrix (host copies of the formulas the kernels use) ----
void q_from_R(const double* R, double q[4]) {
#define M(i, j) R[3 * (i) + (j)]
    double t = M(0, 0) + M(1, 1) + M(2, 2);
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (M(2, 1) - M(1, 2)) * t;
        q[2] = (M(0, 2) - M(2, 0)) * t;
        q[3] = (M(1, 0) - M(0, 1)) * t;
    } else {
        int i = 0;
        if (M(1, 1) > M(0, 0)) i = 1;
        if (M(2, 2) > M(i, i)) i = 2;
        int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(M(i, i) - M(j, j) - M(k, k) + 1.0);
        double c[3];
        c[i] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (M(k, j) - M(j, k)) * t;
        c[j] = (M(j, i) + M(i, j)) * t;
        c[k] = (M(k, i) + M(i, k)) * t;
        q[1] = c[0]; q[2] = c[1]; q[3] = c[2];
    }
#undef M
}

void R_from_q(const double q[4], double R[9]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;          R[2] = txz + twy;
    R[3] = txy + twz;          R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;          R[7] = tyz + twx;          R[8] = 1.0 - (txx + tyy);
}

void cross3(const double a[3], const double b[3], double c[3]) {
    const double c0 = a[1] * b[2] - a[2] * b[1], c1 = a[2] * b[0] - a[0] * b[2], c2 = a[0] * b[1] - a[1] * b[0];
    c[0] = c0; c[1] = c1; c[2] = c2;
}

void q_rotate(const double* q, const double v[3], double o[3]) {
    double uv[3], uv2[3];
    cross3(q + 1, v, uv);
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    cross3(q + 1, uv, uv2);
    for (int i = 0; i < 3; ++i) o[i] = v[i] + q[0] * uv[i] + uv2[i];
}

void q_mul(const double* a, const double* b, double o[4]) {
    double w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    double x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    double y = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
    double z = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
    const double sq = w * w + x * x + y * y + z * z;
    if (sq != 1.0) {
        const double sc = 2.0 / (1.0 + sq);
        w *= sc; x *= sc; y *= sc; z *= sc;
    }
    o[0] = w; o[1] = x; o[2] = y; o[3] = z;
}

// host mirror of d_pose_table (lh_edge.h): estimate_ -> (q_T, t_T, ext*T, R_T)
void pose_table(const double* T12, const double* e, double* pt) {
    const double R[9] = {T12[0], T12[1], T12[2], T12[4], T12[5], T12[6], T12[8], T12[9], T12[10]};
    double q[4];
    q_from_R(R, q);
    const double t[3] = {T12[3], T12[7], T12[11]};
    for (int i = 0; i < 4; ++i) pt[LH_PT_QT + i] = q[i];
    for (int i = 0; i < 3; ++i) pt[LH_PT_TT + i] = t[i];
    double qet[4], rt[3];
    q_mul(e, q, qet);
    q_rotate(e, t, rt);
    for (int i = 0; i < 4; ++i) pt[LH_PT_QET + i] = qet[i];
    for (int i = 0; i < 3; ++i) pt[LH_PT_TET + i] = e[4 + i] + rt[i];
    double Rt[9];
    R_from_q(q, Rt);
    for (int i = 0; i < 9; ++i) pt[LH_PT_RT + i] = Rt[i];
    pt[23] = 0.0;
}

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Planner threads: the CPUs this process may use (affinity mask, capped by a cgroup v2 CPU quota:
// a GPU box exposes every host core but grants a share of them), at most 16.
int auto_host_threads() {
    cpu_set_t set;
    int n = 8;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0};
        long per = 0;
        if (std::fscanf(f, "%31s %ld", q, &per) == 2 && std::strcmp(q, "max") != 0 && per > 0) {
            const long quota = std::atol(q);
            if (quota > 0) n = std::min<long>(n, (quota + per - 1) / per);
        }
        std::fclose(f);
    }
    // the planner's passes are memory-bound and their pool meets at a barrier per pass; its workers are
    // pinned to the caller's last-level cache (lh_plan.cpp Pool), which has 8 cores on an EPYC 9575F.
    // C3 lh_solve on such a box with a 16-CPU quota: 2.12 ms at 8 threads, 2.18 at 12, 2.16 at 16
    // (unpinned: 3.55, 3.45, 2.69)
    return std::max(1, std::min(8, n));
}

// What other sites ask of the transport: is the solve sharded; does it exchange one trial at a time on the host
// (every rank reading the device's stop flag at the same point); has it failed (P2P: a peer's tag did not arrive)
bool sharded(const lh_handle* h) { return h->transport != TR_NONE; }
bool exchange_synchronous(const lh_handle* h) { return h->transport == TR_HOST; }
bool transport_failed(const lh_handle* h) { return h->transport == TR_P2P && *h->p2p.h_xerr; }

struct Prof {
    lh_handle* h;
    int kc;
    hipEvent_t a = nullptr, b = nullptr;
    Prof(lh_handle* hh, int k) : h(hh), kc(k) {
        if (h->opt.profile) {
            a = next_event(h);
            b = next_event(h);
            if (a) (void)hipEventRecord(a, h->stream);
        }
    }
    ~Prof() {
        if (a && b) {
            (void)hipEventRecord(b, h->stream);
            h->pending.push_back({kc, h->cur_trial, a, b});
        }
    }
};

// Launches enqueued for trials past the device's stop (trial > trials_run) exit at their first
// instruction; they are not counted as kernel work.
void collect_profile(lh_handle* h, int trials_run) {
    for (auto& pe : h->pending) {
        float ms = 0.f;
        if (pe.trial > trials_run) continue;
        if (hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess) {
            h->launches[pe.kc] += 1;
            h->total_ms[pe.kc] += ms;
        }
    }
    h->pending.clear();
    h->event_next = 0;
}

// the planner's slot batches go to the device as soon as they are final (plan_fill's on_slots), so
// the copies of the largest arrays overlap the rest of the fill
struct SlotCopy {
    lh_handle* h;
    hipError_t err;
};
void copy_slots(void* user, int64_t s0, int64_t s1) {
    SlotCopy* c = static_cast<SlotCopy*>(user);
    lh_handle* h = c->h;
    if (c->err != hipSuccess || s1 <= s0) return;
    const size_t n = (size_t)(s1 - s0);
    hipStream_t st = h->stream;
    hipError_t e = hipMemcpyAsync(h->d_meta.p + s0, h->s_meta.p + s0, n * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(h->d_uv.p + 2 * s0, h->s_uv.p + 2 * s0, 2 * n * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(h->d_obs_perm.p + s0, h->s_obs_perm.p + s0, n * sizeof(int32_t), hipMemcpyHostToDevice, st);
    c->err = e;
}

// Wait for an event by polling it: hipEventSynchronize measured ~2 ms for lh_upload's copies that the
// solve path (which polls) sees finish within ~0.3 ms of the planner: the runtime's blocking wait
// wakes the thread late.
hipError_t spin_wait(hipEvent_t ev) {
    for (;;) {
        const hipError_t q = hipEventQuery(ev);
        if (q != hipErrorNotReady) return q;
        for (int i = 0; i < 64; ++i) __builtin_ia32_pause();
    }
}

// sync: return only once the copies are done (lh_upload); lh_solve leaves them queued ahead of its
// kernels on the same stream.  Either way the next upload waits for them before it rewrites the staging.
int upload_body(lh_handle* h, const lh_window* w, bool sync);
int rank_max(lh_handle* h, double* buf, int n);
int p2p_setup(lh_handle* h);

// Every exit after the first copy out of the pinned staging is queued must leave ev_staging recorded
// behind it, or the next upload could rewrite (or reallocate) the staging while that DMA still reads
// it: the error returns (LH_E_UNSUPPORTED envelope checks, a failed HIP call) record it here.
//
// A sharded upload holds one collective, the MAX all-reduce of the envelope of S (envelope_collective).  A rank that fails before it (a bad pixel, an unsupported window, an allocation)
// still joins it, contributing its status in word 0 and nothing to the envelope, so the healthy ranks
// are not left blocked in it: every rank then returns the largest status of any rank.
//
// A rank can also fail after that collective (the controllers' buffers, the image initialisation, the arena
// copy), when its peers have already passed it: so every rank that passed it (all of them, or none: the
// collective's status word is shared) closes the upload with a second MAX all-reduce of its final status, and
// a rank whose tail failed takes the others down with it instead of leaving them in the first trial's exchange.
int upload_impl(lh_handle* h, const lh_window* w, bool sync) {
    h->upload_joined = false;
    h->upload_tail = false;
    int st = upload_body(h, w, sync);
    if (st != LH_OK && sharded(h) && !h->upload_joined && w && w->n_poses > 0 && w->n_poses <= LH_PMAX_ANY) {
        std::vector<double> buf(1 + (size_t)w->n_poses, -1e300);
        buf[0] = (double)st;
        rank_max(h, buf.data(), 1 + w->n_poses);
    }
    if (sharded(h) && h->upload_tail) {
        double fs = (double)st;
        const int st_r = rank_max(h, &fs, 1);
        if (st == LH_OK) st = (st_r != LH_OK) ? st_r : (int)fs;
        if (st != LH_OK) h->uploaded = false;
    }
    // the peer-write exchange's buffers (P2P only) once every rank's upload is through (its collectives run on all ranks)
    if (st == LH_OK && (st = p2p_setup(h)) != LH_OK) h->uploaded = false;
    if (st != LH_OK && !h->staging_pending && h->ev_staging) {
        if (hipEventRecord(h->ev_staging, h->stream) == hipSuccess) h->staging_pending = true;
    }
    return st;
}

// ---- the stages of an upload, in upload_body's order.  None of them decides how the window is solved:
//      that is lh::solve_config (lh_plan.h), whose result the handle keeps (h->cfg). ----
// the previous upload's copies out of the pinned staging
int wait_staging(lh_handle* h) {
    if (h->staging_pending) {
        HIPCHK(spin_wait(h->ev_staging));
        h->staging_pending = false;
    }
    return LH_OK;
}

// the landmark positions need no plan: they go out first and cross the link while the planner runs
int send_landmarks(lh_handle* h, const lh_window* w) {
    if (w && w->n_landmarks > 0 && w->lm_xyz) {
        const size_t nl = 3 * (size_t)w->n_landmarks;
        HIPCHK(h->d_lm_in.ensure(nl));
        HIPCHK(h->s_lm.ensure(nl));
        const ByteSeg seg{h->s_lm.p, w->lm_xyz, nl * sizeof(double)};
        par_copy(h, &seg, 1);
        HIPCHK(hipMemcpyAsync(h->d_lm_in.p, h->s_lm.p, nl * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    return LH_OK;
}

int plan_window(lh_handle* h, const lh_window* w, const lh::Switches& sw) {
    lh::PlanCfg cfg;
    cfg.chunk_lm = h->opt.chunk_landmarks;
    cfg.rank_invariant_pairs = h->opt.world_size > 1;
    cfg.n_cu = h->n_cu;
    cfg.lin_smem = lh_lin_smem;
    cfg.lds_limit = (size_t)h->lds_limit;
    lh::apply_switches(cfg, sw);
    const int st = lh::plan_structure(w, cfg, h->opt.world_size > 1, h->plan, h->pool);
    if (st != LH_OK) {
        HIPCHK(hipEventRecord(h->ev_staging, h->stream));
        h->staging_pending = true;
    }
    return st;
}

// what this rank's share of the window must fit, whatever the other ranks hold
int rank_local_limits(lh_handle* h) {
    const lh::Plan& pl = h->plan;
    // k_lin's write-through record stores address both record buffers through one buffer descriptor
    // (32-bit byte offsets): up to ~8.3 M landmarks per rank
    if ((size_t)2 * pl.n_rec * LH_REC * sizeof(double) > (size_t)INT32_MAX) return LH_E_UNSUPPORTED;
    // a chunk window must fit one CU's LDS
    for (int T = 1; T <= LH_TMAX; ++T)
        if (pl.tgroup_begin[T + 1] > pl.tgroup_begin[T] && lh_lin_smem(T, pl.ncam, pl.lin_waves) > (size_t)h->lds_limit)
            return LH_E_UNSUPPORTED;
    return LH_OK;
}

// The per-window tables (all but the observation slots and the positions) live in one arena, on the
// device and in pinned staging, at the same offsets: they cross the link as one copy.  Each
// hipMemcpyAsync costs ~10 us of DMA-engine turnaround beside its transfer (rocprofv3 memory-copy
// trace of lh_upload), and the 13 small copies these were made most of the upload's tail.
// band_possible: the window may run banded (decided after the envelope collective), so k_ctrl_b's
// tables are reserved.
int bind_arena(lh_handle* h, bool band_possible) {
    const lh::Plan& pl = h->plan;
    const int P = pl.P, ncam = pl.ncam;
    h->P = P; h->L = pl.L; h->O = pl.O; h->ncam = ncam;
    h->n_rec = pl.n_rec;
    h->n_slots = pl.n_slots;
    h->LY = lh_rs_make(P, pl.npairs);
    const size_t PT = (size_t)P * ncam * LH_PT;
    Arena ar;   // 256-byte aligned segments
    const size_t o_chunks = ar.take(pl.n_chunks * sizeof(lh_chunk), 256);
    const size_t o_sbs = ar.take((size_t)pl.n_sb * sizeof(lh_subbatch), 256);
    const size_t o_lmp = ar.take((size_t)pl.n_rec * sizeof(int32_t), 256);
    const size_t o_pptr = ar.take(((size_t)pl.npairs + 1) * sizeof(uint32_t), 256);
    const size_t o_items = ar.take((size_t)pl.n_items * sizeof(uint32_t), 256);
    const size_t o_ppq = ar.take(2 * (size_t)pl.npairs * sizeof(uint16_t), 256);
    const size_t o_rsmap = ar.take((size_t)pl.npairs * 36 * sizeof(uint32_t), 256);
    const size_t o_ptab = ar.take(2 * PT * sizeof(double), 256);
    const size_t o_qt = ar.take(24 * (size_t)std::max(P, 1) * sizeof(double), 256);
    const size_t o_ext = ar.take(LH_EXT * (size_t)ncam * sizeof(double), 256);
    const size_t o_fix = ar.take(pl.fixed_bits.size() * sizeof(uint64_t), 256);
    const size_t o_bptr = ar.take(pl.brow_ptr.size() * sizeof(int32_t), 256);
    const size_t o_bent = ar.take(pl.brow_ent.size() * sizeof(uint32_t), 256);
    const size_t o_units = ar.take(16 * LH_NSTEP * sizeof(uint16_t), 256);
    const size_t n_bunits = band_possible ? 16 * (size_t)lh::kBandSteps : 0, n_bblk = band_possible ? (size_t)P * 64 : 0;
    const size_t o_bunits = ar.take(n_bunits * sizeof(uint16_t), 256);
    const size_t o_bblk = ar.take(n_bblk * sizeof(int32_t), 256);
    const size_t o_red = ar.take(4 * ((size_t)pl.npairs + 1) * sizeof(uint32_t), 256);
    HIPCHK(h->d_arena.ensure(ar.end));
    HIPCHK(h->s_arena.ensure(ar.end));
    h->arena_bytes = ar.end;
    auto bind = [](auto& d, auto& st, uint8_t* dbase, uint8_t* sbase, size_t off, size_t count) {
        using T = std::remove_pointer_t<decltype(d.p)>;
        d.p = reinterpret_cast<T*>(dbase + off); d.n = count;
        st.p = reinterpret_cast<T*>(sbase + off); st.n = count;
    };
    uint8_t* db = h->d_arena.p;
    uint8_t* sb = h->s_arena.p;
    bind(h->d_chunks, h->s_chunks, db, sb, o_chunks, pl.n_chunks);
    bind(h->d_sbs, h->s_sbs, db, sb, o_sbs, pl.n_sb);
    bind(h->d_lm_perm, h->s_lm_perm, db, sb, o_lmp, pl.n_rec);
    bind(h->d_pair_ptr, h->s_pair_ptr, db, sb, o_pptr, pl.npairs + 1);
    bind(h->d_items, h->s_items, db, sb, o_items, pl.n_items);
    bind(h->d_pair_pq, h->s_pair_pq, db, sb, o_ppq, 2 * (size_t)pl.npairs);
    bind(h->d_rsmap, h->s_rsmap, db, sb, o_rsmap, (size_t)pl.npairs * 36);
    bind(h->d_ptab_init, h->s_ptab, db, sb, o_ptab, 2 * PT);
    bind(h->d_qt_init, h->s_qt, db, sb, o_qt, 24 * (size_t)std::max(P, 1));
    bind(h->d_ext, h->s_ext, db, sb, o_ext, LH_EXT * (size_t)ncam);
    bind(h->d_fixed, h->s_fixed, db, sb, o_fix, pl.fixed_bits.size());
    bind(h->d_brow_ptr, h->s_brow_ptr, db, sb, o_bptr, pl.brow_ptr.size());
    bind(h->d_brow_ent, h->s_brow_ent, db, sb, o_bent, pl.brow_ent.size());
    bind(h->d_units, h->s_units, db, sb, o_units, 16 * LH_NSTEP);
    bind(h->d_bunits, h->s_bunits, db, sb, o_bunits, n_bunits);
    bind(h->d_bblk, h->s_bblk, db, sb, o_bblk, n_bblk);
    bind(h->d_red, h->s_red, db, sb, o_red, 4 * ((size_t)pl.npairs + 1));
    return LH_OK;
}

// the device buffers sized by the window alone (before the fill: its slot batches are copied as they
// complete); ladder: one pending step per lambda-ladder rung
int window_buffers(lh_handle* h, int ladder) {
    const lh::Plan& pl = h->plan;
    const int P = pl.P;
    const size_t PT = (size_t)P * pl.ncam * LH_PT;
    HIPCHK(h->d_meta.ensure(pl.n_slots));
    HIPCHK(h->d_uv.ensure(2 * pl.n_slots));
    HIPCHK(h->d_obs_perm.ensure(pl.n_slots));
    HIPCHK(h->d_lm_in.ensure(3 * (size_t)pl.L));
    HIPCHK(h->d_rec.ensure(2 * (size_t)pl.n_rec * LH_REC));
    HIPCHK(h->d_ptab.ensure(2 * PT));
    HIPCHK(h->d_qt.ensure(24 * (size_t)P));
    HIPCHK(h->d_wflag.ensure(2 * (size_t)pl.n_slots));
    HIPCHK(h->d_rows.ensure((size_t)pl.n_items * LH_ROW));
    HIPCHK(h->d_rs_stage.ensure(h->LY.total));
    HIPCHK(h->d_rs_commit.ensure(h->LY.total));
    HIPCHK(h->d_maxd.ensure(1));
    HIPCHK(h->d_dxp.ensure((size_t)ladder * 6 * (size_t)std::max(P, 1)));
    HIPCHK(h->d_ctrl.ensure(1));
    HIPCHK(h->d_out_xyz.ensure(3 * (size_t)pl.L));
    HIPCHK(h->d_out_rho.ensure(pl.O));
    if (exchange_synchronous(h)) HIPCHK(h->s_rs.ensure(h->LY.total + 1));   // its pinned copy of the reduced system
    return LH_OK;
}

// the planner's fill into the staging (the observation slots go out as they complete), k_reduce's
// block table, and the plan's small tables
int fill_staging(lh_handle* h, const lh_window* w, const lh::Switches& sw) {
    const lh::Plan& pl = h->plan;
    HIPCHK(h->s_meta.ensure(pl.n_slots));
    HIPCHK(h->s_uv.ensure(2 * pl.n_slots));
    HIPCHK(h->s_obs_perm.ensure(pl.n_slots));
    lh::PlanOut po{h->s_chunks.p, h->s_sbs.p, h->s_meta.p, h->s_uv.p, h->s_obs_perm.p, h->s_lm_perm.p,
                   h->s_items.p, h->s_pair_pq.p, h->s_rsmap.p, nullptr};   // positions: copied out above
    SlotCopy sc{h, hipSuccess};
    const int batches = pl.n_slots >= (1 << 16) ? 8 : 1;
    const int fs = lh::plan_fill(w, pl, po, h->pool, copy_slots, &sc, batches);
    HIPCHK(sc.err);
    if (fs != LH_OK) {   // a pixel that is not a float value; the slot copies already issued read the staging
        HIPCHK(hipEventRecord(h->ev_staging, h->stream));
        h->staging_pending = true;
        return fs;
    }
    std::memcpy(h->s_pair_ptr.p, pl.pair_ptr.data(), pl.pair_ptr.size() * sizeof(uint32_t));
    const bool skip = lh::reduce_skip(h->opt.world_size, sw);
    h->n_red = lh::reduce_table(pl, skip, h->s_red.p);
    if (skip) {   // the skipped pairs' blocks (and every buffer slot k_reduce never writes) read as zero
        HIPCHK(hipMemsetAsync(h->d_rs_stage.p, 0, h->LY.total * sizeof(double), h->stream));
        HIPCHK(hipMemsetAsync(h->d_rs_commit.p, 0, h->LY.total * sizeof(double), h->stream));
    }
    std::memcpy(h->s_fixed.p, pl.fixed_bits.data(), pl.fixed_bits.size() * sizeof(uint64_t));
    std::memcpy(h->s_brow_ptr.p, pl.brow_ptr.data(), pl.brow_ptr.size() * sizeof(int32_t));
    std::memcpy(h->s_brow_ent.p, pl.brow_ent.data(), pl.brow_ent.size() * sizeof(uint32_t));
    return LH_OK;
}

// camera extrinsics (Sophus SE3 of Camera::pose_) and the initial pose tables into the staging
struct ExtFlags {
    int identity = 0, rot_identity = 0;   // bit c: camera c's extrinsic (its rotation) is exactly the identity
};
ExtFlags pose_tables(lh_handle* h, const lh_window* w) {
    const int P = h->P, ncam = h->ncam;
    double* ext = h->s_ext.p;
    ExtFlags fl;
    for (int c = 0; c < ncam; ++c) {
        static const double I12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        const double* E = (w->n_cams > 0) ? w->cam_ext + 12 * c : I12;
        const double R[9] = {E[0], E[1], E[2], E[4], E[5], E[6], E[8], E[9], E[10]};
        double q[4], Rq[9];
        q_from_R(R, q);
        R_from_q(q, Rq);
        double* e = ext + LH_EXT * (size_t)c;
        for (int i = 0; i < 4; ++i) e[i] = q[i];
        e[4] = E[3]; e[5] = E[7]; e[6] = E[11];
        for (int i = 0; i < 9; ++i) e[7 + i] = Rq[i];
        if (q[0] == 1.0 && q[1] == 0.0 && q[2] == 0.0 && q[3] == 0.0) {
            fl.rot_identity |= 1 << c;
            if (e[4] == 0.0 && e[5] == 0.0 && e[6] == 0.0) fl.identity |= 1 << c;
        }
    }
    for (int p = 0; p < P; ++p) {
        const double* T = w->pose_Tcw + 12 * p;
        for (int s = 0; s < 2; ++s) {
            std::memcpy(h->s_qt.p + 12 * ((size_t)s * P + p), T, 12 * sizeof(double));
            for (int c = 0; c < ncam; ++c)
                pose_table(T, ext + LH_EXT * (size_t)c, h->s_ptab.p + ((size_t)s * P * ncam + (size_t)p * ncam + c) * LH_PT);
        }
    }
    return fl;
}

// The sharded upload's envelope collective.  Word 0 carries the largest status of any rank (a rank
// that failed earlier joins from upload_impl with its own), then -pf per pose: the union envelope.
// Everything after it is decided on data identical on every rank; a rank-local failure after it
// (allocations, the image initialisation, the copies) is shared by upload_impl's closing status
// all-reduce.
int envelope_collective(lh_handle* h, std::vector<int>& pf) {
    if (!sharded(h)) return LH_OK;
    const int P = h->P;
    std::vector<double> neg(1 + (size_t)P);
    neg[0] = 0.0;
    for (int p = 0; p < P; ++p) neg[1 + p] = -(double)pf[p];
    h->upload_joined = true;
    const int st_r = rank_max(h, neg.data(), 1 + P);
    if (st_r != LH_OK) return st_r;
    if (neg[0] > 0.0) return (int)neg[0];
    for (int p = 0; p < P; ++p) pf[p] = (int)(-neg[1 + p]);
    h->upload_tail = true;
    // (test hook) this rank fails after the collective, as a failed allocation in the tail would
    const char* fail_env = getenv("LH_TEST_FAIL_AFTER_ENVELOPE");
    if (fail_env && atoi(fail_env) == h->opt.rank) return LH_E_HIP;
    return LH_OK;
}

int configure(lh_handle* h, const std::vector<int>& pf, const lh::Switches& sw) {
    lh::SolveIn in;
    in.P = h->P;
    in.n_brow_ent = h->plan.brow_ent.size();
    in.lin_waves = h->plan.lin_waves;
    in.pf = pf.data();
    in.linear_solver = h->opt.linear_solver;
    in.max_trials = h->opt.max_trials;
    in.world_size = h->opt.world_size;
    in.rccl = h->transport == TR_RCCL;
    in.sw = sw;
    return lh::solve_config(in, h->cfg);
}

// the buffers the configuration sizes, and what of them is cleared per window
int controller_buffers(lh_handle* h) {
    const lh::SolveConfig& c = h->cfg;
    const lh::Plan& pl = h->plan;
    // per batch rung a per-edge rho0 and the chunk scalars
    HIPCHK(h->d_rho.ensure((size_t)c.batch * pl.n_slots));
    HIPCHK(h->d_csc.ensure((size_t)c.batch * pl.n_chunks * 4));
    if (c.kind == LH_CTRL_BAND) {   // k_ctrl_b's L rows and ND blocks; L entries outside the envelope are never written: zero
        const size_t nb = (size_t)c.ladder * c.n_band;
        HIPCHK(h->d_band.ensure(nb));
        HIPCHK(hipMemsetAsync(h->d_band.p, 0, nb * sizeof(double), h->stream));
    } else if (c.kind == LH_CTRL_PCG) {
        HIPCHK(h->d_gA.ensure(c.n_gA));
    } else if (c.kind == LH_CTRL_DENSE) {   // k_ctrl_g's systems and k_dense's S: zeroed once, when grown
        const bool fresh = h->d_gA.n < c.n_gA;
        HIPCHK(h->d_gA.ensure(c.n_gA));
        if (fresh) HIPCHK(hipMemsetAsync(h->d_gA.p, 0, h->d_gA.n * sizeof(double), h->stream));
        const bool fresh_s = h->d_gS.n < c.n_gS;
        HIPCHK(h->d_gS.ensure(c.n_gS));
        if (fresh_s) HIPCHK(hipMemsetAsync(h->d_gS.p, 0, h->d_gS.n * sizeof(double), h->stream));
    }
    if (c.bimg) {   // entries no pair block writes stay zero: cleared per window
        HIPCHK(h->d_img.ensure(c.n_img));
        HIPCHK(hipMemsetAsync(h->d_img.p, 0, c.n_img * sizeof(double), h->stream));
    }
    if (c.img) {
        HIPCHK(h->d_img.ensure(c.n_img));
        HIPCHK(lh_launch_img_init(h->stream, h->d_img.p, 6 * h->P));
    }
    return LH_OK;
}

// the controller's work units, and k_ctrl_b's pair -> block table, into the staging
void stage_tables(lh_handle* h) {
    const lh::SolveConfig& c = h->cfg;
    if (c.kind == LH_CTRL_LDS) std::memcpy(h->s_units.p, c.units.data(), c.units.size() * sizeof(uint16_t));
    if (c.kind == LH_CTRL_BAND) {
        std::memcpy(h->s_bunits.p, c.units.data(), c.units.size() * sizeof(uint16_t));
        lh::band_block_table(h->plan, h->s_bblk.p);
    }
}

void set_params(lh_handle* h, const lh_window* w, const ExtFlags& ext) {
    const lh::SolveConfig& c = h->cfg;
    lh_params& prm = h->prm;
    prm.P = h->P;
    prm.npairs = h->plan.npairs;
    prm.n = 6 * h->P;
    prm.ncam = h->ncam;
    prm.max_iters = h->opt.max_iters;
    prm.max_trials = h->opt.max_trials;
    prm.strategy = h->opt.strategy;
    prm.guard = h->opt.degenerate_guard;
    prm.gate_mode = h->opt.gate_mode;
    prm.precision = h->opt.precision;
    prm.lambda_given = h->opt.lambda_init >= 0.0;
    prm.ext_identity = ext.identity;
    prm.ext_rot_identity = ext.rot_identity;
    prm.huber_delta = h->opt.huber_delta;
    prm.stop_dchi2 = h->opt.stop_dchi2;
    prm.tau = h->opt.tau;
    prm.lambda_cap = h->opt.lambda_cap;
    prm.lambda_init = h->opt.lambda_init;
    prm.solver = h->opt.linear_solver;
    prm.pcg_tol = h->opt.pcg_tol;
    prm.pcg_max_it = h->opt.pcg_max_iters;
    prm.no_evo = c.no_evo;
    prm.eval_first = c.eval_first;
    prm.dec_in_reduce = c.dec_in_reduce;
    prm.batch = c.batch;
    prm.n_chunks = (int32_t)h->plan.n_chunks;
    prm.commit_in_reduce = c.commit_in_reduce;
    prm.ladder = c.ladder;
    prm.lad_stride = (int32_t)c.lad_stride;
    prm.ladder_eager = c.ladder_eager;
    prm.band_narrow = c.band_narrow ? 1 : 0;
    prm.band_lu = c.band_lu ? 1 : 0;
    prm.bimg = c.bimg;
    prm.img = c.img;
    prm.nd_steps = c.nd.nsteps;
    prm.nd_a = c.nd.a;
    prm.nd_s = c.nd.s;
    prm.nd_long_first = c.nd.long_first;
    for (int i = 0; i < 4; ++i) prm.K[i] = w->K[i];
}

// every per-window table in one copy, and the event the next upload waits for
int send_arena(lh_handle* h, bool sync) {
    hipStream_t s = h->stream;
    if (h->arena_bytes)
        HIPCHK(hipMemcpyAsync(h->d_arena.p, h->s_arena.p, h->arena_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(h->ev_staging, s));
    h->staging_pending = true;
    if (sync) {
        HIPCHK(spin_wait(h->ev_staging));
        h->staging_pending = false;
    }
    return LH_OK;
}

int upload_body(lh_handle* h, const lh_window* w, bool sync) {
    const double t0 = now_ms();
    h->uploaded = false;
    h->solved = false;
    const lh::Switches sw = lh::read_switches();
    STAGE(wait_staging(h));
    STAGE(send_landmarks(h, w));
    STAGE(plan_window(h, w, sw));
    std::vector<int> pf = lh::plan_envelope(h->plan);   // this rank's; the collective below unites the ranks'
    STAGE(rank_local_limits(h));
    STAGE(bind_arena(h, lh::band_possible(h->plan.P, h->opt.linear_solver, sw)));
    STAGE(window_buffers(h, lh::ladder_rungs(h->opt.max_trials, sw)));
    STAGE(fill_staging(h, w, sw));
    const ExtFlags ext = pose_tables(h, w);
    STAGE(envelope_collective(h, pf));
    STAGE(configure(h, pf, sw));
    STAGE(controller_buffers(h));
    stage_tables(h);
    set_params(h, w, ext);
    const double t1 = now_ms();
    STAGE(send_arena(h, sync));
    h->last_prep_ms = t1 - t0;
    h->last_upload_ms = now_ms() - t0;
    h->uploaded = true;
    return LH_OK;
}

#define DBGSYNC(name)                                                                                   \
    do {                                                                                                \
        if (g_debug) {                                                                                  \
            hipError_t e_ = hipStreamSynchronize(s);                                                    \
            if (e_ == hipSuccess) e_ = hipGetLastError();                                               \
            if (e_ != hipSuccess) {                                                                     \
                fprintf(stderr, "lego_ba: %s failed: %s\n", name, hipGetErrorString(e_));               \
                return LH_E_HIP;                                                                        \
            }                                                                                           \
        }                                                                                               \
    } while (0)

// One k_lin launch per tile count present.  In a trial, block 0 of the first launch (of a T = 1 launch
// with no chunks when the window has none) stores the trial's candidate poses and pose tables.
int launch_lin(lh_handle* h, int trial) {
    hipStream_t s = h->stream;
    // block 0 of the first launch: a trial's candidate poses and tables, or (the initial linearisation) the
    // restart of the solve from the uploaded window
    int writer = 1;
    const int P = h->P;
    const lh_reset_args rst{h->d_lm_perm.p, h->d_lm_in.p, h->d_qt_init.p, h->d_ptab_init.p, 24 * P,
                            (int)(2 * (size_t)P * h->ncam * LH_PT), 6 * std::max(P, 1)};
    for (int T = 1; T <= LH_TMAX; ++T) {
        const int c0 = h->plan.tgroup_begin[T], c1 = h->plan.tgroup_begin[T + 1];
        const bool last = T == LH_TMAX;
        if (c1 == c0 && !(writer && last)) continue;
        HIPCHK(lh_launch_lin(T, h->plan.lin_waves, trial, c1 - c0, c0, s, h->d_chunks.p, h->d_sbs.p, h->d_uv.p, h->d_meta.p, h->d_rec.p,
                             h->d_ptab.p, h->d_ext.p, h->d_ctrl.p, h->d_dxp.p, h->d_rho.p, h->d_rows.p,
                             h->d_csc.p, h->d_items.p, h->d_wflag.p, (long)h->n_slots, h->prm, h->n_rec,
                             h->d_fixed.p, h->d_qt.p, writer, rst));
        writer = 0;
        DBGSYNC("k_lin");
    }
    return LH_OK;
}

// host-transport exchange: the reduced system (and at the initial linearisation max|diag H_ll|)
// through the caller's all-reduce, synchronously
int host_exchange(lh_handle* h, int mode) {
    hipStream_t s = h->stream;
    const size_t n = (size_t)h->LY.total;
    HIPCHK(hipMemcpyAsync(h->s_rs.p, h->d_rs_stage.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (mode == 0) HIPCHK(hipMemcpyAsync(h->s_rs.p + n, h->d_maxd.p, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (mode == 0 && h->opt.allreduce(h->opt.allreduce_user, h->s_rs.p + n, 1, 1) != 0) return LH_E_RCCL;
    if (h->opt.allreduce(h->opt.allreduce_user, h->s_rs.p, (int64_t)n, 0) != 0) return LH_E_RCCL;
    ++h->n_coll;
    HIPCHK(hipMemcpyAsync(h->d_rs_stage.p, h->s_rs.p, n * sizeof(double), hipMemcpyHostToDevice, s));
    if (mode == 0) HIPCHK(hipMemcpyAsync(h->d_maxd.p, h->s_rs.p + n, sizeof(double), hipMemcpyHostToDevice, s));
    return LH_OK;
}

lh_band_args band_args(lh_handle* h) {
    if (h->cfg.kind != LH_CTRL_BAND) return lh_band_args{nullptr, nullptr, nullptr, nullptr};
    return lh_band_args{h->d_bblk.p, h->d_bunits.p, h->d_band.p, h->d_band.p + lh::band_scratch(h->P).nd_off};
}

// RCCL, P2P: one exchange (mode 0: and max|diag H_ll|) on the stream; next_chain: a top-up, P2P's chain numbers go on
int exchange_on_stream(lh_handle* h, int mode, bool next_chain) {
    if (h->transport == TR_P2P) {   // lh_launch_p2p; tags carry the solve count, so no stale tag ever matches
        const P2pState& x = h->p2p;
        const int seq = next_chain ? ++h->cur_trial : h->cur_trial;
        const unsigned long long tag = ((unsigned long long)x.solve_gen << 32) | (unsigned long long)(seq + 1);
        ++h->n_coll;
        HIPCHK(lh_launch_p2p(h->stream, h->d_rs_stage.p, h->d_maxd.p, h->LY.total, x.peers, h->opt.rank,
                             h->opt.world_size, seq & 1, tag, x.xchg_slot, mode, x.d_xerr));
        return LH_OK;
    }
    if (mode == 0) NCCLCHK(ncclAllReduce(h->d_maxd.p, h->d_maxd.p, 1, ncclFloat64, ncclMax, h->comm, h->stream));
    NCCLCHK(ncclAllReduce(h->d_rs_stage.p, h->d_rs_stage.p, (size_t)h->LY.total, ncclFloat64, ncclSum, h->comm, h->stream));
    ++h->n_coll;
    return LH_OK;
}

// the per-chain exchange of a trial (mode 1) or of the initial linearisation (mode 0); *stopped as in enqueue_trial
int exchange_chain(lh_handle* h, int mode, bool* stopped) {
    switch (h->transport) {
        case TR_NONE: break;
        case TR_RCCL: case TR_P2P: { Prof pr(h, KC_ALLREDUCE); return exchange_on_stream(h, mode, false); }
        case TR_HOST:
            HIPCHK(hipStreamSynchronize(h->stream));
            *stopped = mode != 0 && h->h_done[0];   // device-determined, identical on every rank
            return *stopped ? LH_OK : host_exchange(h, mode);
    }
    return LH_OK;
}

// One LM trial (mode 1) or the initial linearisation (mode 0).  *stopped is set (host transport
// only) when the device had already stopped: no exchange and no k_ctrl were issued.
int enqueue_trial(lh_handle* h, int mode, bool* stopped) {
    hipStream_t s = h->stream;
    h->cur_trial = (mode == 0) ? 0 : h->cur_trial + 1;
    {
        Prof pr(h, mode == 0 ? KC_INIT : KC_LIN);
        int st = launch_lin(h, mode);
        if (st != LH_OK) return st;
    }
    {
        Prof pr(h, KC_REDUCE);
        HIPCHK(lh_launch_reduce(s, h->d_rows.p, h->d_csc.p, h->d_red.p, h->n_red, h->d_ctrl.p,
                                h->d_rs_stage.p, h->d_rs_commit.p, h->d_maxd.p, h->prm, h->plan.n_chunks, mode, h->d_done,
                                h->cur_trial, h->d_img.p));
        DBGSYNC("k_reduce");
    }
    STAGE(exchange_chain(h, mode, stopped));
    if (*stopped) return LH_OK;
    {
        Prof pr(h, KC_CTRL);
        if (h->cfg.kind == LH_CTRL_DENSE)
            HIPCHK(lh_launch_dense(s, h->d_rs_stage.p, h->d_pair_pq.p, h->d_ctrl.p, h->d_gS.p, h->P));
        HIPCHK(lh_launch_ctrl(s, h->d_ctrl.p, h->d_rs_commit.p, h->d_rs_stage.p, h->d_maxd.p, h->d_rsmap.p, h->d_pair_pq.p,
                              h->d_dxp.p, h->prm, mode, h->d_done, h->cur_trial, h->d_gA.p, h->d_gS.p, h->d_brow_ptr.p,
                              h->d_brow_ent.p, h->d_units.p, band_args(h), h->d_img.p, h->cfg.kind));
        DBGSYNC("k_ctrl");
    }
    return LH_OK;
}

// Results into the caller's buffers: device -> pinned staging in one stream (poses, landmark
// positions gathered into window order, per-edge rho0), then the staging is copied out on the
// planner's threads (a pageable device-to-host copy runs at a fraction of the link).
// the ABI-5 outlier flags were asked for (lh_result.is_outlier; read only at ABI 5)
bool wants_outliers(const lh_handle* h, const lh_result* out) {
    return out && h->opt.abi_version >= 5 && out->is_outlier != nullptr;
}

// the outlier pass's three result scalars lie behind the flags (one copy brings both)
size_t outlier_scalars_off(const lh_handle* h) { return ((size_t)h->O + 15) & ~(size_t)15; }
void read_outlier_scalars(const lh_handle* h, lh_result* out) {
    double r3[3];
    std::memcpy(r3, h->s_oflag.p + outlier_scalars_off(h), sizeof(r3));
    out->outlier_th = r3[0]; out->n_inlier = (int64_t)r3[1]; out->n_outlier = (int64_t)r3[2];
}

// Backend::Optimize's outlier pass on the device (backend_lego.cpp:163-194): flags + 3 scalars, into the pinned staging.
// A sharded window: the reference counts the whole window's edges, so each rank counts its own, the five counts and the
// edge counts are summed over the ranks (one 6-double exchange: every rank of the handle asks for the flags alike, as
// it solves alike), and each rank flags its edges at the threshold the totals give.
int outlier_pass(lh_handle* h, const lh_result* out) {
    hipStream_t s = h->stream;
    const size_t bytes = outlier_scalars_off(h) + 3 * sizeof(double);
    const double* rho = h->d_rho.p + h->rho_off;
    const long nslots = (long)h->n_slots, n_obs = (long)h->O;
    const double th = out->outlier_chi2_th;
    HIPCHK(h->d_ocnt.ensure(5 * 256));
    HIPCHK(h->d_oflag.ensure(bytes));
    HIPCHK(h->s_oflag.ensure(bytes));
    switch (h->transport) {
        case TR_P2P:   // ADVICE.md, first finding: each rank thresholds on its own shard's counts.  The fix moves
                       // this label down to the sharded cases (the sum through the caller's all-reduce).
        case TR_NONE:
            HIPCHK(lh_launch_outliers(s, rho, h->d_obs_perm.p, nslots, n_obs, th, h->d_ocnt.p, h->d_oflag.p));
            break;
        case TR_RCCL: case TR_HOST:
            HIPCHK(h->d_otot.ensure(6));
            HIPCHK(lh_launch_outlier_counts(s, rho, h->d_obs_perm.p, nslots, n_obs, th, h->d_ocnt.p, h->d_otot.p));
            if (h->transport == TR_RCCL) {
                NCCLCHK(ncclAllReduce(h->d_otot.p, h->d_otot.p, 6, ncclFloat64, ncclSum, h->comm, s));
            } else {
                double t6[6];
                HIPCHK(hipMemcpyAsync(t6, h->d_otot.p, sizeof(t6), hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                if (h->opt.allreduce(h->opt.allreduce_user, t6, 6, 0) != 0) return LH_E_RCCL;
                HIPCHK(hipMemcpyAsync(h->d_otot.p, t6, sizeof(t6), hipMemcpyHostToDevice, s));
                HIPCHK(hipStreamSynchronize(s));   // (t6 is on this stack frame)
            }
            HIPCHK(lh_launch_outlier_flags(s, rho, h->d_obs_perm.p, nslots, n_obs, th, h->d_otot.p, h->d_oflag.p));
            break;
    }
    HIPCHK(hipMemcpyAsync(h->s_oflag.p, h->d_oflag.p, bytes, hipMemcpyDeviceToHost, s));
    return LH_OK;
}

int download(lh_handle* h, lh_result* out, int cur) {
    hipStream_t s = h->stream;
    const int P = h->P;
    const double t0 = now_ms();
    const size_t np = out->pose_Tcw ? 12 * (size_t)P : 0;
    const size_t nl = (out->lm_xyz && h->L) ? 3 * (size_t)h->L : 0;
    const size_t ne = (out->edge_robust_chi2 && h->O) ? (size_t)h->O : 0;
    const bool fl = wants_outliers(h, out);
    if (fl) STAGE(outlier_pass(h, out));
    if (np + nl + ne == 0 && !fl) {
        out->time_download_ms = 0.0;
        return LH_OK;
    }
    if (np + nl + ne == 0) {
        HIPCHK(hipStreamSynchronize(s));
        read_outlier_scalars(h, out);
        const ByteSeg seg_f = {out->is_outlier, h->s_oflag.p, (size_t)h->O};
        par_copy(h, &seg_f, 1);
        out->time_download_ms = now_ms() - t0;
        return LH_OK;
    }
    HIPCHK(h->s_out.ensure(np + nl + ne));
    double* st = h->s_out.p;
    if (np)   // estimate_ of every VertexPose (backend_lego.cpp:198-213)
        HIPCHK(hipMemcpyAsync(st, h->d_qt.p + 12 * (size_t)cur * P, np * sizeof(double), hipMemcpyDeviceToHost, s));
    if (nl || ne) {
        // landmarks without an edge are not vertices (backend_lego.cpp:126): they keep their input
        if (nl) HIPCHK(hipMemcpyAsync(h->d_out_xyz.p, h->d_lm_in.p, nl * sizeof(double), hipMemcpyDeviceToDevice, s));
        HIPCHK(lh_launch_gather(s, h->d_ctrl.p, h->d_rec.p, h->d_lm_perm.p, nl ? h->n_rec : 0, h->d_rho.p + h->rho_off,
                                h->d_obs_perm.p, ne ? (long)h->n_slots : 0L, h->d_out_xyz.p, h->d_out_rho.p));
        if (nl) HIPCHK(hipMemcpyAsync(st + np, h->d_out_xyz.p, nl * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    // poses and landmarks are copied out of the staging while the per-edge chi2 is still in flight
    hipEvent_t e_first = next_event(h);
    if (!e_first) return LH_E_HIP;
    HIPCHK(hipEventRecord(e_first, s));
    if (ne) HIPCHK(hipMemcpyAsync(st + np + nl, h->d_out_rho.p, ne * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(spin_wait(e_first));
    const ByteSeg seg[2] = {{out->pose_Tcw, st, np * sizeof(double)}, {out->lm_xyz, st + np, nl * sizeof(double)}};
    par_copy(h, seg, 2);
    HIPCHK(hipStreamSynchronize(s));
    const ByteSeg seg_e[2] = {{out->edge_robust_chi2, st + np + nl, ne * sizeof(double)},
                              {fl ? out->is_outlier : nullptr, fl ? h->s_oflag.p : nullptr, fl ? (size_t)h->O : 0}};
    par_copy(h, seg_e, 2);
    if (fl) read_outlier_scalars(h, out);
    out->time_download_ms = now_ms() - t0;
    return LH_OK;
}

// ---- the stages of a resident solve.  Its start: the mapped words' reset, P2P's tag generation (every rank solves
//      the same number of times); an exchange that failed earlier fails every later solve ----
int begin_solve(lh_handle* h) {
    volatile int* hd = h->h_done;   // [0] done, [1] progress word (ctrl_lm_step)
    hd[0] = 0; hd[1] = -1;
    h->n_coll = 0;
    if (h->transport == TR_P2P) ++h->p2p.solve_gen;
    return transport_failed(h) ? LH_E_RCCL : LH_OK;
}

// One turn of a host spin loop: every 4096th, and at most every 50 ms unless `often`, hipStreamQuery turns a device fault
// or the transport's failure into an error return (a query delays the next launch by ~6 us).  idle: it found nothing queued.
struct Watchdog { bool often = false, idle = false; unsigned spin = 0; double t_query = now_ms(); };
int watchdog_turn(lh_handle* h, Watchdog& wd) {
    wd.idle = false;
    if ((++wd.spin & 4095) == 0 && (wd.often || now_ms() - wd.t_query > 50.0)) {
        const hipError_t q = hipStreamQuery(h->stream);
        if (q != hipSuccess && q != hipErrorNotReady) return LH_E_HIP;
        if (transport_failed(h)) {
            (void)hipStreamSynchronize(h->stream);
            return LH_E_RCCL;
        }
        wd.idle = q == hipSuccess;
        wd.t_query = now_ms();
    }
    __builtin_ia32_pause();
    return LH_OK;
}

// The initial chain (its block 0 restarts the solve: controller, poses, tables, step; launch_lin), then the trials;
// *enq: how many of those were enqueued.
int enqueue_chains(lh_handle* h, const lh::TrialSchedule& ts, int* enq) {
    volatile int* hd = h->h_done;
    bool stopped = false;
    STAGE(enqueue_trial(h, 0, &stopped));
    if (exchange_synchronous(h)) {
        // each trial's exchange waits for the previous k_ctrl, whose stop flag every rank reads at the same point
        while (*enq < ts.max_total && !stopped) {
            STAGE(enqueue_trial(h, 1, &stopped));
            if (!stopped) ++*enq;
        }
        return LH_OK;
    }
    // k_ctrl writes each live trial it has decided into the mapped progress word; the host keeps ts.depth trials
    // enqueued past it (one when the next iteration reaches max_iters: lh::may_enqueue) until the device raises done
    static const bool query_often = getenv("LH_QUERY_OFTEN") != nullptr;   // diagnostic A/B switch (timing only)
    Watchdog wd{query_often};
    while (!hd[0] && *enq < ts.max_total) {
        if (lh::may_enqueue(ts, hd[1], *enq)) {
            STAGE(enqueue_trial(h, 1, &stopped));
            ++*enq;
        } else {
            STAGE(watchdog_turn(h, wd));
        }
    }
    return LH_OK;
}

// The top-up after the stop, to equal collective counts: no rank enqueued more than the schedule's target for the
// stop chain and every rank tops up to it (lh_plan.h); nobody reads what these exchanges carry
int exchange_top_up(lh_handle* h, const lh::TrialSchedule& ts, int enq, int stop_chain) {
    if (!sharded(h) || exchange_synchronous(h)) return LH_OK;   // (synchronous: none was enqueued past the stop)
    const int target = lh::topup_target(ts, stop_chain);
    if (enq > target) return LH_E_STATE;   // cannot happen: the schedule's bound
    for (; enq < target; ++enq) STAGE(exchange_on_stream(h, 1, true));
    HIPCHK(hipStreamSynchronize(h->stream));
    return transport_failed(h) ? LH_E_RCCL : LH_OK;
}

// the solve's summary from the controller's words (lh_ctrl, or the mapped lh_host_words)
template <typename W>
void write_summary(const lh_handle* h, const W& w, double time_ms, lh_result* out) {
    out->time_ms = time_ms;
    out->iterations = w.iter; out->trials = w.trials; out->accepted = w.accepted;
    out->chi2_initial = w.chi2_initial; out->chi2_final = w.chi; out->lambda_final = w.lambda;
    out->pcg_iterations = w.pcg_iters; out->degenerate = w.nonpd;
    out->trace_len = std::min((int)w.trace_len, std::min(out->trace_cap, LH_TRACE));
    for (int i = 0; i < out->trace_len; ++i) {
        if (out->trace_chi2) out->trace_chi2[i] = w.trace_chi[i];
        if (out->trace_lambda) out->trace_lambda[i] = w.trace_lambda[i];
    }
    out->time_prep_ms = h->last_prep_ms; out->time_upload_ms = h->last_upload_ms; out->time_download_ms = 0.0;
}

int solve_resident_impl(lh_handle* h, lh_result* out) {
    if (!h->uploaded) return LH_E_STATE;
    hipStream_t s = h->stream;
    hipEvent_t e0 = next_event(h), e1 = next_event(h);
    if (!e0 || !e1) return LH_E_HIP;
    // No arrays wanted (and no collectives, profiling or printout): the summary comes with done in the
    // mapped words, and the solve returns when the host sees it; later work on this handle is stream-
    // ordered behind the solve's kernels (lh_destroy synchronises)
    const bool fast = out && !out->pose_Tcw && !out->lm_xyz && !out->edge_robust_chi2 && !wants_outliers(h, out) &&
                      !sharded(h) && !h->opt.profile && !h->opt.verbose;
    const lh::TrialSchedule ts = lh::trial_schedule(h->opt.max_iters, h->opt.max_trials, h->prm.eval_first,
                                                    h->opt.trials_per_sync, exchange_synchronous(h));
    const double t_start = now_ms();
    STAGE(begin_solve(h));
    if (!fast) HIPCHK(hipEventRecord(e0, s));   // (the array-free solve times itself on the host clock)
    int enq = 0;
    STAGE(enqueue_chains(h, ts, &enq));
    if (fast) {
        // the wait: every trial is enqueued and done comes with the last; a fault, or an idle stream without it, ends it
        volatile int* hd = h->h_done;
        for (Watchdog wd; !hd[0];) {
            STAGE(watchdog_turn(h, wd));
            if (wd.idle && !hd[0]) return LH_E_STATE;
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        const double ms = now_ms() - t_start;   // host clock: enqueue of the first kernel to done seen
        write_summary(h, *reinterpret_cast<const volatile lh_host_words*>(h->h_done), ms, out);
        h->event_next = 0; h->last_chains = h->last_lskips = -1;   // (the chain counts are not in the host words)
        return LH_OK;
    }
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipMemcpyAsync(h->h_ctrl, h->d_ctrl.p, sizeof(lh_ctrl), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const lh_ctrl& c = *h->h_ctrl;
    STAGE(exchange_top_up(h, ts, enq, c.seq_last));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    h->rho_off = (size_t)c.rho_sel * h->n_slots;
    h->last_batches = c.nbatches; h->last_retrials[0] = c.nretrials[0]; h->last_retrials[1] = c.nretrials[1];
    h->last_chains = c.seq_last; h->last_lskips = c.lskips;
    if (out) {
        write_summary(h, c, ms, out);
        STAGE(download(h, out, c.cur));
    }
    if (h->opt.verbose) {
        printf("==========LEGO OPTIMIZER (MI355X)==========\n");
        for (int i = 0; i < std::min(c.trace_len, LH_TRACE); ++i)
            printf("Iteration = %d,\tChi = %g,\tLambda = %g\n", i, c.trace_chi[i], c.trace_lambda[i]);
        printf("\nInfo: \nTimeCost(SolveProblem) = %g ms\n", (double)ms);
    }
    if (h->opt.profile) collect_profile(h, c.seq_last);
    else h->event_next = 0;
    return LH_OK;
}

// Every rank must run the same controller with the same options: the LM decisions are taken on
// identical all-reduced sums, and the number of collectives a solve issues is a function of the stop
// trial, the enqueue depth and max_iters x max_trials (lh_plan.h trial_schedule).  Ranks whose options
// differ would issue different collective counts and hang, so lh_create compares them once: each
// rank contributes (v, -v) per option to a MAX all-reduce, and any rank whose v differs from the
// maximum or minimum sees a mismatch (every rank returns LH_E_BADARG).
// MAX over the ranks of buf[0..n), in place; a no-op on one rank
int rank_max(lh_handle* h, double* buf, int n) {
    switch (h->transport) {
        case TR_NONE: return LH_OK;
        case TR_HOST: case TR_P2P: return h->opt.allreduce(h->opt.allreduce_user, buf, n, 1) != 0 ? LH_E_RCCL : LH_OK;
        case TR_RCCL: break;
    }
    DevBuf<double> d;
    HIPCHK(d.ensure(n));
    HIPCHK(hipMemcpyAsync(d.p, buf, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    NCCLCHK(ncclAllReduce(d.p, d.p, n, ncclFloat64, ncclMax, h->comm, h->stream));
    HIPCHK(hipMemcpyAsync(buf, d.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return LH_OK;
}

// every peer's mapping closed (this rank's own entry is its buffer, not a mapping)
void p2p_close_peers(P2pState& x) {
    for (int r = 0; r < LH_P2P_MAX; ++r)
        if (x.peers.p[r] && x.peers.p[r] != x.d_xchg.p) (void)hipIpcCloseMemHandle(x.peers.p[r]);
    x.peers = lh_peers{};
}

// P2P: this rank's exchange buffer (2 parities x world slots of the packed reduced system + max|diag H_ll|, then
// the arrival tags), exported over IPC, and every peer's opened here.  Collective: every rank calls it at the same
// upload (the buffer size follows from the reduced system's layout, identical on every rank); its handles travel
// through the caller's all-reduce (a sum of byte values, exact), and a MAX all-reduce of the status ends it, so a
// rank that cannot map a peer takes every rank's upload down with it.  The other transports have no such buffers.
int p2p_setup(lh_handle* h) {
    if (h->transport != TR_P2P) return LH_OK;
    P2pState& x = h->p2p;
    const int world = h->opt.world_size, rank = h->opt.rank;
    const long slot = (h->LY.total + 1 + 63) & ~63L;
    const size_t need = (size_t)2 * world * slot + 2 * (size_t)world;   // (a tag is one 8-byte word)
    if (x.d_xchg.n >= need && x.xchg_slot == slot) return LH_OK;
    int st = LH_OK;
    p2p_close_peers(x);
    x.d_xchg.release();
    hipIpcMemHandle_t mine{};
    if (x.d_xchg.ensure(need) != hipSuccess ||
        hipMemsetAsync(x.d_xchg.p, 0, need * sizeof(double), h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess || hipIpcGetMemHandle(&mine, x.d_xchg.p) != hipSuccess)
        st = LH_E_HIP;
    static_assert(sizeof(hipIpcMemHandle_t) <= 64, "an IPC handle in 64 byte values");
    std::vector<double> hb((size_t)world * 64, 0.0);
    const uint8_t* mb = reinterpret_cast<const uint8_t*>(&mine);
    for (size_t i = 0; i < sizeof(mine); ++i) hb[(size_t)rank * 64 + i] = (double)mb[i];
    if (h->opt.allreduce(h->opt.allreduce_user, hb.data(), (int64_t)hb.size(), 0) != 0) return LH_E_RCCL;
    x.peers.p[rank] = x.d_xchg.p;
    for (int r = 0; r < world && st == LH_OK; ++r) {
        if (r == rank) continue;
        hipIpcMemHandle_t ph{};
        uint8_t* pb = reinterpret_cast<uint8_t*>(&ph);
        for (size_t i = 0; i < sizeof(ph); ++i) pb[i] = (uint8_t)hb[(size_t)r * 64 + i];
        void* p = nullptr;
        if (hipIpcOpenMemHandle(&p, ph, hipIpcMemLazyEnablePeerAccess) != hipSuccess || !p) {
            if (getenv("LH_DEBUG_P2P")) fprintf(stderr, "lego_ba: rank %d cannot map rank %d's exchange buffer\n", rank, r);
            st = LH_E_UNSUPPORTED;
        } else {
            x.peers.p[r] = static_cast<double*>(p);
        }
    }
    double fs = (double)st;
    const int st_r = rank_max(h, &fs, 1);
    if (st_r != LH_OK) return st_r;
    if (fs > 0.0) return (int)fs;
    x.xchg_slot = slot;
    return LH_OK;
}

int check_rank_options(lh_handle* h) {
    const lh_options& o = h->opt;
    const int depth = lh::trial_schedule(o.max_iters, o.max_trials, 0, o.trials_per_sync, exchange_synchronous(h)).depth;
    const double v[] = {(double)o.max_iters, (double)o.max_trials, (double)o.strategy, o.huber_delta, o.stop_dchi2,
                        o.tau, o.lambda_cap, o.lambda_init, (double)o.linear_solver, (double)o.world_size,
                        (double)o.degenerate_guard, (double)depth, (double)o.pcg_max_iters, o.pcg_tol,
                        (double)o.gate_mode, (double)o.chunk_landmarks > 0 ? 1.0 : 0.0, (double)o.comm_mode,
                        (double)o.precision};
    constexpr int n = (int)(sizeof(v) / sizeof(v[0]));
    double buf[2 * n];
    for (int i = 0; i < n; ++i) { buf[i] = v[i]; buf[n + i] = -v[i]; }
    if (!sharded(h)) return LH_OK;
    const int st = rank_max(h, buf, 2 * n);
    if (st != LH_OK) return st;
    for (int i = 0; i < n; ++i)
        if (!(buf[i] == -buf[n + i])) return LH_E_BADARG;   // max != min somewhere (NaN options fail too)
    return LH_OK;
}

}  // namespace

// ============================================================================
// C ABI
// ============================================================================
extern "C" {

const char* lh_strerror(int status) {
    switch (status) {
        case LH_OK: return "ok";
        case LH_E_EMPTY: return "empty problem: no vertices or no edges";
        case LH_E_BADARG: return "bad argument";
        case LH_E_HIP: return "HIP runtime error";
        case LH_E_RCCL: return "RCCL / exchange error";
        case LH_E_UNSUPPORTED: return "window outside the supported envelope";
        case LH_E_STATE: return "call out of order";
        case LH_E_SINGULAR: return "singular system: no free pose, a pivot that is not positive, or rank-deficient landmarks";
        default: return "unknown status";
    }
}

const char* lh_kernel_name(int kc) { return (kc >= 0 && kc < KC_N) ? kKernelNames[kc] : ""; }

// (the exported symbol, not the header's macro: binaries built against the ABI-4 header call it by this name)
#undef lh_default_options
void lh_default_options(lh_options* o) { lh_default_options_v(o, 4); }

void lh_default_options_v(lh_options* o, int abi) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->abi_version = abi;
    o->max_iters = 10;
    o->max_trials = 10;
    o->strategy = LH_STRATEGY_DEFAULT;
    o->huber_delta = 5.991;
    o->stop_dchi2 = 1e-5;
    o->tau = 1e-5;
    o->lambda_cap = 5e10;
    o->lambda_init = -1.0;
    o->linear_solver = LH_SOLVER_LDLT;
    o->verbose = 0;
    o->device = -1;
    o->world_size = 1;
    o->rank = 0;
    o->degenerate_guard = 0;
    o->trials_per_sync = 0;
    o->profile = 0;
    o->pcg_max_iters = 0;
    o->pcg_tol = 1e-6;
    o->gate_mode = 0;
    o->chunk_landmarks = 0;
    o->comm_mode = LH_COMM_RCCL;
    o->host_threads = 0;
    o->allreduce = nullptr;
    o->allreduce_user = nullptr;
    o->precision = LH_PREC_FP64;
}

int lh_comm_unique_id(uint8_t out[128]) {
    if (!out) return LH_E_BADARG;
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    std::memcpy(out, &id, 128);
    return LH_OK;
}

int lh_create(lh_handle** hp, const lh_options* opt) {
    if (!hp || !opt) return LH_E_BADARG;
    *hp = nullptr;
    if (opt->abi_version != LH_ABI_VERSION && opt->abi_version != 4) return LH_E_BADARG;
    if (opt->max_iters < 0 || opt->max_trials < 0 || opt->world_size < 1 || opt->rank < 0 ||
        opt->rank >= opt->world_size || (opt->strategy != 0 && opt->strategy != 1))
        return LH_E_BADARG;
    if (opt->linear_solver != LH_SOLVER_LDLT && opt->linear_solver != LH_SOLVER_PCG) return LH_E_BADARG;
    if (opt->linear_solver == LH_SOLVER_PCG && !(opt->pcg_tol >= 0.0)) return LH_E_BADARG;
    if (opt->gate_mode != 0 && opt->gate_mode != 1) return LH_E_BADARG;
    if (opt->precision != LH_PREC_FP64 && opt->precision != LH_PREC_FP32_RESID) return LH_E_BADARG;
    if (opt->degenerate_guard != 0 && opt->degenerate_guard != 1) return LH_E_BADARG;
    if (opt->chunk_landmarks < 0 || opt->host_threads < 0) return LH_E_BADARG;
    if (opt->comm_mode != LH_COMM_RCCL && opt->comm_mode != LH_COMM_HOST && opt->comm_mode != LH_COMM_P2P)
        return LH_E_BADARG;
    if (opt->world_size > 1 && opt->comm_mode != LH_COMM_RCCL && !opt->allreduce) return LH_E_BADARG;
    if (opt->comm_mode == LH_COMM_P2P && opt->world_size > LH_P2P_MAX) return LH_E_UNSUPPORTED;
    lh_handle* h = new (std::nothrow) lh_handle();
    if (!h) return LH_E_HIP;
    h->opt = *opt;
    int dev = opt->device;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) { delete h; return LH_E_HIP; }
    }
    if (hipSetDevice(dev) != hipSuccess) { delete h; return LH_E_HIP; }
    h->device = dev;
    int lds = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && lds > 0)
        h->lds_limit = lds;
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0) h->n_cu = ncu;
    if (lh_prepare_lin(h->lds_limit) != hipSuccess) { delete h; return LH_E_HIP; }
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { delete h; return LH_E_HIP; }
    if (hipHostMalloc((void**)&h->h_ctrl, sizeof(lh_ctrl), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&h->h_done, sizeof(lh_host_words), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void**)&h->d_done, h->h_done, 0) != hipSuccess) {
        lh_destroy(h);
        return LH_E_HIP;
    }
    // the pool starts std::threads, which throw std::system_error when the process may not create
    // more (e.g. under a cgroup pids limit): no exception crosses the ABI
    try {
        h->pool = new lh::Pool(opt->host_threads > 0 ? std::min(opt->host_threads, 64) : auto_host_threads());
    } catch (...) {
        h->pool = nullptr;
    }
    if (!h->pool) { lh_destroy(h); return LH_E_HIP; }
    if (hipEventCreateWithFlags(&h->ev_staging, hipEventDisableTiming) != hipSuccess) {
        h->ev_staging = nullptr;
        lh_destroy(h);
        return LH_E_HIP;
    }
    // The transport.  LH_FORCE_RCCL=1 builds a one-rank communicator on a single GPU, so the data-path
    // collectives (and their stream ordering) run in single-GPU tests too
    const char* force = std::getenv("LH_FORCE_RCCL");
    const bool force_comm = opt->world_size == 1 && force && force[0] == '1';
    h->transport = opt->world_size == 1 ? (force_comm ? TR_RCCL : TR_NONE)
                 : opt->comm_mode == LH_COMM_HOST ? TR_HOST : opt->comm_mode == LH_COMM_P2P ? TR_P2P : TR_RCCL;
    if (h->transport == TR_P2P) {
        if (hipHostMalloc((void**)&h->p2p.h_xerr, sizeof(int), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostGetDevicePointer((void**)&h->p2p.d_xerr, h->p2p.h_xerr, 0) != hipSuccess) {
            lh_destroy(h);
            return LH_E_HIP;
        }
        *h->p2p.h_xerr = 0;
    }
    if (h->transport == TR_RCCL) {
        ncclUniqueId id;
        if (force_comm) {
            if (ncclGetUniqueId(&id) != ncclSuccess) { lh_destroy(h); return LH_E_RCCL; }
        } else {
            std::memcpy(&id, opt->comm_id, sizeof(id));
        }
        if (ncclCommInitRank(&h->comm, opt->world_size, id, opt->rank) != ncclSuccess) {
            h->comm = nullptr;
            lh_destroy(h);
            return LH_E_RCCL;
        }
    }
    if (opt->world_size > 1) {
        const int st = check_rank_options(h);
        if (st != LH_OK) { lh_destroy(h); return st; }
    }
    *hp = h;
    return LH_OK;
}

// What depends on order (also of a handle lh_create gave up on half-built); `delete h` frees the handle's buffers
void lh_destroy(lh_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->comm) ncclCommDestroy(h->comm);
    p2p_close_peers(h->p2p);   // the peers' mappings, while this rank's own exchange buffer is still there
    for (auto e : h->event_pool) (void)hipEventDestroy(e);
    if (h->ev_staging) (void)hipEventDestroy(h->ev_staging);
    delete h->pool;
    if (h->p2p.h_xerr) (void)hipHostFree(h->p2p.h_xerr);
    if (h->h_ctrl) (void)hipHostFree(h->h_ctrl);
    if (h->h_done) (void)hipHostFree(h->h_done);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int lh_upload(lh_handle* h, const lh_window* in) {
    if (!h) return LH_E_BADARG;
    if (hipSetDevice(h->device) != hipSuccess) return LH_E_HIP;
    try {
        return upload_impl(h, in, true);
    } catch (const std::bad_alloc&) {
        return LH_E_HIP;
    } catch (...) {
        return LH_E_BADARG;
    }
}

int lh_solve_resident(lh_handle* h, lh_result* out) {
    if (!h) return LH_E_BADARG;
    if (hipSetDevice(h->device) != hipSuccess) return LH_E_HIP;
    h->solved = false;
    try {
        const int st = solve_resident_impl(h, out);
        h->solved = st == LH_OK;   // (lh_covariance works on the state this solve returned)
        return st;
    } catch (...) {
        return LH_E_HIP;
    }
}

int lh_solve(lh_handle* h, const lh_window* in, lh_result* out) {
    if (!h) return LH_E_BADARG;
    if (hipSetDevice(h->device) != hipSuccess) return LH_E_HIP;
    int st;
    try {
        st = upload_impl(h, in, false);   // the copies stay queued ahead of the solve's kernels
    } catch (const std::bad_alloc&) {
        return LH_E_HIP;
    } catch (...) {
        return LH_E_BADARG;
    }
    if (st != LH_OK) return st;
    return lh_solve_resident(h, out);
}

int lh_kernel_stats_get(lh_handle* h, lh_kernel_stats* out) {
    if (!h || !out) return LH_E_BADARG;
    for (int i = 0; i < KC_N; ++i) { out->launches[i] = h->launches[i]; out->total_ms[i] = h->total_ms[i]; }
    return LH_OK;
}

int lh_set_profiling(lh_handle* h, int on) {
    if (!h) return LH_E_BADARG;
    h->opt.profile = on ? 1 : 0;
    return LH_OK;
}

void lh_kernel_stats_reset(lh_handle* h) {
    if (!h) return;
    for (int i = 0; i < KC_N; ++i) { h->launches[i] = 0; h->total_ms[i] = 0.0; }
}

int lh_classify_outliers(const double* rchi2, int64_t n_obs, double chi2_th, uint8_t* is_outlier, double* th_out,
                         int64_t* n_inlier, int64_t* n_outlier) {
    if (n_obs < 0 || (n_obs > 0 && !rchi2)) return LH_E_BADARG;
    // backend_lego.cpp:164-184
    int64_t cin = 0, cout = 0;
    int iteration = 0;
    while (iteration < 5) {
        cout = 0;
        cin = 0;
        for (int64_t i = 0; i < n_obs; ++i) {
            if (rchi2[i] > chi2_th) cout++;
            else cin++;
        }
        double ratio = cin / double(cin + cout);
        if (ratio > 0.5) break;
        chi2_th *= 2;
        iteration++;
    }
    // :186-194
    if (is_outlier)
        for (int64_t i = 0; i < n_obs; ++i) is_outlier[i] = rchi2[i] > chi2_th ? 1 : 0;
    if (th_out) *th_out = chi2_th;
    if (n_inlier) *n_inlier = cin;
    if (n_outlier) *n_outlier = cout;
    return LH_OK;
}

// diagnostic hook: per-phase wave-cycle totals of the -DLH_STAMPS build (zeros otherwise)
int lh_debug_stamps(unsigned long long* out, int n, int reset) {
    if (!out || n < 0) return LH_E_BADARG;
    // an array-free solve returns before its stream drains (solve_resident_impl): the stamps of its
    // last kernels land first
    if (hipDeviceSynchronize() != hipSuccess) return LH_E_HIP;
    return lh_read_stamps(out, n, reset) == hipSuccess ? LH_OK : LH_E_HIP;
}

// diagnostic hook: k_lin's per-wave records of the -DLH_STAMPS build (zeros otherwise)
int lh_debug_lin_stamps(unsigned long long* out, int n) {
    if (!out || n < 0) return LH_E_BADARG;
    if (hipDeviceSynchronize() != hipSuccess) return LH_E_HIP;
    return lh_read_lin_stamps(out, n) == hipSuccess ? LH_OK : LH_E_HIP;
}

// test hook: k_ctrl's reduced-system solve on a dense symmetric S, device pointers
// (n > LH_NPAD: k_ctrl_g's global-memory solve, the windows past LH_PMAX poses)
int lh_debug_ldlt_probe(const double* S, const double* b, int n, double* x) {
    if (!S || !b || !x) return LH_E_BADARG;
    if (n < 1 || n > 6 * LH_PMAX_WIN) return LH_E_UNSUPPORTED;
    if (n <= LH_NPAD) {
        HIPCHK(lh_launch_ldlt_probe(S, b, n, x, 0, 0.0, 0, nullptr));
    } else {
        const size_t ng = (size_t)((n + 31) & ~31);
        double* gA = nullptr;
        HIPCHK(hipMalloc(&gA, ng * ng * sizeof(double)));
        hipError_t e = lh_launch_ldlt_g_probe(S, b, n, x, gA);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        (void)hipFree(gA);
        if (e != hipSuccess) return LH_E_HIP;
    }
    HIPCHK(hipDeviceSynchronize());
    return LH_OK;
}

int lh_debug_pcg_probe(const double* S, const double* b, int n, double tol, int max_iters, double* x, int* iters) {
    if (!S || !b || !x || !(tol >= 0.0)) return LH_E_BADARG;
    if (n < 1 || n > LH_NPAD) return LH_E_UNSUPPORTED;
    int* d_it = nullptr;
    HIPCHK(hipMalloc(&d_it, sizeof(int)));
    hipError_t e = lh_launch_ldlt_probe(S, b, n, x, 1, tol, max_iters, d_it);
    int it = 0;
    if (e == hipSuccess) e = hipMemcpy(&it, d_it, sizeof(int), hipMemcpyDeviceToHost);
    (void)hipFree(d_it);
    if (e != hipSuccess) return LH_E_HIP;
    if (iters) *iters = it;
    return LH_OK;
}

// The per-kernel HIP-event bracket of lh_set_profiling includes the launch itself: this is the
// same bracket around an empty kernel on the handle's stream (mean of 64 after 8 warm-ups).
int lh_debug_event_floor(lh_handle* h, double* ms) {
    if (!h || !ms) return LH_E_BADARG;
    if (hipSetDevice(h->device) != hipSuccess) return LH_E_HIP;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess) return LH_E_HIP;
    if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); return LH_E_HIP; }
    double tot = 0.0;
    int st = LH_OK;
    for (int i = 0; i < 72 && st == LH_OK; ++i) {
        if (hipEventRecord(a, h->stream) != hipSuccess || lh_launch_nop(h->stream) != hipSuccess ||
            hipEventRecord(b, h->stream) != hipSuccess || hipEventSynchronize(b) != hipSuccess) {
            st = LH_E_HIP;
            break;
        }
        float e = 0.f;
        if (hipEventElapsedTime(&e, a, b) != hipSuccess) st = LH_E_HIP;
        if (i >= 8) tot += e;
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    if (st == LH_OK) *ms = tot / 64.0;
    return st;
}

// k_lin's duration per trial: after a solve, clear the stop flag, replay the trial-mode k_lin
// launch(es) `reps` times back to back between two events, raise the flag again.  Each replay reads
// the committed buffers and rewrites the candidate ones: the same work as every trial of the solve.
int lh_debug_time_lin(lh_handle* h, int reps, double* ms) {
    if (!h || !ms || reps < 1) return LH_E_BADARG;
    if (!h->uploaded) return LH_E_STATE;
    if (hipSetDevice(h->device) != hipSuccess) return LH_E_HIP;
    hipStream_t s = h->stream;
    int* done = reinterpret_cast<int*>(reinterpret_cast<char*>(h->d_ctrl.p) + offsetof(lh_ctrl, done));
    int* evo = reinterpret_cast<int*>(reinterpret_cast<char*>(h->d_ctrl.p) + offsetof(lh_ctrl, evo));
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess) return LH_E_HIP;
    if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); return LH_E_HIP; }
    int st = LH_OK;
    const int zero = 0, one = 1;
    int evo_saved = 0;   // a solve stopped by max_iters leaves evo set: replay the full linearisation
    if (hipMemcpyAsync(&evo_saved, evo, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) st = LH_E_HIP;
    if (st == LH_OK && hipMemcpyAsync(evo, &zero, sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) st = LH_E_HIP;
    if (st == LH_OK && hipMemcpyAsync(done, &zero, sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) st = LH_E_HIP;
    if (st == LH_OK && launch_lin(h, 1) != LH_OK) st = LH_E_HIP;   // warm-up
    if (st == LH_OK && hipEventRecord(a, s) != hipSuccess) st = LH_E_HIP;
    for (int r = 0; r < reps && st == LH_OK; ++r)
        if (launch_lin(h, 1) != LH_OK) st = LH_E_HIP;
    if (st == LH_OK && hipEventRecord(b, s) != hipSuccess) st = LH_E_HIP;
    if (hipMemcpyAsync(done, &one, sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) st = LH_E_HIP;
    if (hipStreamSynchronize(s) != hipSuccess) st = LH_E_HIP;
    if (hipMemcpy(evo, &evo_saved, sizeof(int), hipMemcpyHostToDevice) != hipSuccess) st = LH_E_HIP;
    float e = 0.f;
    if (st == LH_OK && hipEventElapsedTime(&e, a, b) != hipSuccess) st = LH_E_HIP;
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    if (st == LH_OK) *ms = (double)e / reps;
    return st;
}

int lh_debug_comm_count(lh_handle* h, int64_t* n) {
    if (!h || !n) return LH_E_BADARG;
    *n = h->n_coll;
    return LH_OK;
}

int lh_debug_chains(lh_handle* h, int* chains) {
    if (!h || !chains) return LH_E_BADARG;
    *chains = h->last_chains;
    return LH_OK;
}

int lh_debug_ladder(lh_handle* h, int* rungs, int* skipped) {
    if (!h || !rungs || !skipped) return LH_E_BADARG;
    if (!h->uploaded) return LH_E_STATE;
    *rungs = h->cfg.ladder;
    *skipped = h->last_lskips;
    return LH_OK;
}

int lh_debug_batch(lh_handle* h, int* batch_max, int* batches, int* retrials) {
    if (!h || !batch_max || !batches) return LH_E_BADARG;
    if (!h->uploaded) return LH_E_STATE;
    *batch_max = h->cfg.batch;
    *batches = h->last_batches;
    if (retrials) { retrials[0] = h->last_retrials[0]; retrials[1] = h->last_retrials[1]; }
    return LH_OK;
}

int lh_debug_controller(lh_handle* h, int* which) {
    if (!h || !which) return LH_E_BADARG;
    if (!h->uploaded) return LH_E_STATE;
    // lh_ctrl_kind | bit 8: k_ctrl_b's one-row-per-lane back substitution | bit 9: its stream loaders take units
    *which = h->cfg.debug_word();
    return LH_OK;
}

int lh_debug_lin_shape(lh_handle* h, int* waves, int* chunks, int* chunk_landmarks) {
    if (!h || !waves || !chunks || !chunk_landmarks) return LH_E_BADARG;
    if (!h->uploaded) return LH_E_STATE;
    *waves = h->cfg.lin_waves;
    *chunks = h->plan.n_chunks;
    *chunk_landmarks = h->plan.chunk_lm;
    return LH_OK;
}

// test hook: the reduced system as the last chain left it (which: include/lego_ba.h), read behind the handle's stream
int lh_debug_reduced_system(lh_handle* h, int which, double* out, int64_t cap, int64_t* n_out, int32_t* npairs_out) {
    if (!h || !out || !n_out || !npairs_out || which < 0 || which > 3) return LH_E_BADARG;
    if (!h->uploaded) return LH_E_BADARG;
    if (hipSetDevice(h->device) != hipSuccess) return LH_E_HIP;
    HIPCHK(hipStreamSynchronize(h->stream));
    const double* src = nullptr;
    int64_t n = 0;
    if (which == 0 || which == 1) {
        src = which == 0 ? h->d_rs_stage.p : h->d_rs_commit.p;
        n = h->LY.total;
    } else if (which == 2) {   // the pending pose step: rung ctrl->lad of the ladder's steps
        int32_t lad = 0;
        HIPCHK(hipMemcpy(&lad, reinterpret_cast<const char*>(h->d_ctrl.p) + offsetof(lh_ctrl, lad), sizeof(lad),
                         hipMemcpyDeviceToHost));
        n = 6 * (int64_t)h->P;
        if (lad < 0 || lad >= std::max(h->cfg.ladder, 1)) return LH_E_STATE;
        src = h->d_dxp.p + (size_t)lad * (size_t)n;
    } else {   // the staged half of k_reduce's image of S (prm.img, prm.bimg; nothing otherwise)
        src = h->d_img.p;
        n = (int64_t)(h->cfg.n_img / 2);
    }
    *n_out = n;
    *npairs_out = h->LY.npairs;
    if (cap < n) return LH_E_BADARG;
    if (n > 0) HIPCHK(hipMemcpy(out, src, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return LH_OK;
}

// test hook: every step of the lambda ladder the last factoring controller built (include/lego_ba.h), read behind
// the handle's stream.  It only copies: lh_ctrl, the steps and every later solve are left as they are.
int lh_debug_ladder_steps(lh_handle* h, double* dxp_out, int64_t cap, int64_t* n_out, int32_t* lad_n_out,
                          int32_t* lad_out, double* spose_out, int32_t* its_out) {
    if (!h || !dxp_out || !n_out || !lad_n_out || !lad_out || !spose_out || !its_out) return LH_E_BADARG;
    if (!h->uploaded) return LH_E_BADARG;
    if (hipSetDevice(h->device) != hipSuccess) return LH_E_HIP;
    HIPCHK(hipStreamSynchronize(h->stream));
    // lad, lad_n and the two per-rung arrays (lh_ctrl keeps them in this order: one copy each, device to host)
    int32_t lad[2] = {0, 0}, its[LH_LAD];
    double sp[LH_LAD];
    const char* c = reinterpret_cast<const char*>(h->d_ctrl.p);
    static_assert(offsetof(lh_ctrl, lad_n) == offsetof(lh_ctrl, lad) + sizeof(int32_t), "lad, lad_n are adjacent");
    HIPCHK(hipMemcpy(lad, c + offsetof(lh_ctrl, lad), sizeof(lad), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(its, c + offsetof(lh_ctrl, lad_its), sizeof(its), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sp, c + offsetof(lh_ctrl, spose_l), sizeof(sp), hipMemcpyDeviceToHost));
    const int rungs = std::max(h->cfg.ladder, 1);   // d_dxp holds this many steps (lh_upload)
    if (lad[1] < 0 || lad[1] > rungs || lad[1] > LH_LAD || lad[0] < 0 || lad[0] >= rungs) return LH_E_STATE;
    const int64_t n = (int64_t)lad[1] * 6 * (int64_t)h->P;
    *n_out = n;
    *lad_n_out = lad[1];
    if (cap < n) return LH_E_BADARG;
    if (n > 0) HIPCHK(hipMemcpy(dxp_out, h->d_dxp.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    *lad_out = lad[0];
    for (int r = 0; r < lad[1]; ++r) { spose_out[r] = sp[r]; its_out[r] = its[r]; }
    return LH_OK;
}

int lh_debug_mfma_probe(const double* A, const double* B, double* D) {
    if (lh_launch_mfma_probe(A, B, D) != hipSuccess) return LH_E_HIP;
    if (hipDeviceSynchronize() != hipSuccess) return LH_E_HIP;
    return LH_OK;
}

}  // extern "C"
