// lh_handle.h — the handle behind include/lego_ba.h and the buffer types it is made of: internal to the library's
// host files (lh_host.cpp: the solver; lh_frontend.cpp and lh_frame.cpp: the frontend; lh_cov_host.cpp: lh_covariance; lh_marg_host.cpp: lh_marginalize).
// DevBuf and HostBuf free their memory in their destructors, so `delete h` frees every buffer of the handle.  Neither
// may live at namespace or static scope: its destructor would then call into the HIP runtime during process teardown,
// after the runtime is gone.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/lego_ba.h"
#include "lh_common.h"
#include "lh_gftt.h"
#include "lh_plan.h"

namespace lh {

enum { KC_LIN = 0, KC_REDUCE = 1, KC_CTRL = 2, KC_ALLREDUCE = 3, KC_INIT = 4, KC_N = 8 };

// An owned allocation, grown on demand and reused across calls: device memory (DevBuf), or pinned host staging
// (HostBuf) with headroom, since the next window is similar
template <typename T, bool kPinned>
struct Buf {
    T* p = nullptr; size_t n = 0;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }
    hipError_t ensure(size_t count) {
        if (count <= n && p) return hipSuccess;
        release();
        const size_t c = std::max<size_t>(kPinned ? count + count / 4 : count, 1);
        hipError_t e = kPinned ? hipHostMalloc((void**)&p, c * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, c * sizeof(T));
        if (e == hipSuccess) n = c;
        return e;
    }
    void release() {
        if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        n = 0;
    }
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using HostBuf = Buf<T, true>;

// A typed window into an arena (no ownership): the per-window tables share one device and one pinned
// allocation so they cross the link as one copy (upload_impl)
template <typename T>
struct View { T* p = nullptr; size_t n = 0; };

// How the ranks exchange ("One seam"): not at all (one rank), RCCL (also LH_FORCE_RCCL=1 on one rank),
// LH_COMM_HOST, LH_COMM_P2P.  Decided once in lh_create; only the collective functions switch on it.
enum Transport { TR_NONE, TR_RCCL, TR_HOST, TR_P2P };
struct P2pState {
    DevBuf<double> d_xchg;        // this rank's exchange buffer (lh_common.h), IPC-exported
    lh_peers peers{};             // every rank's exchange buffer as mapped here (opened IPC handles)
    long xchg_slot = 0;           // doubles per slot
    uint32_t solve_gen = 0;       // tags: solves so far (the same count on every rank)
    int *h_xerr = nullptr, *d_xerr = nullptr;   // host-mapped failure word (a peer's tag did not arrive)
};

// The resident image of lh_track_frame and lh_insert_keyframe (lh_frame.cpp): two pyramid buffers, rows packed to
// `cols` bytes and sized for every level (lh::pyramid_bytes), of which img[cur] holds the last successful call's image
// with levels 0 .. levels - 1 built.  The protocol of a call that uses it: invalidate() before its first enqueue,
// commit() once it has succeeded; a call that returns an argument or state error touches nothing.
struct ResidentImage {
    DevBuf<uint8_t> img[2];
    bool matches(int c, int r) const { return valid && cols == c && rows == r; }
    // the first level of img[cur]'s pyramid a call has to build: all above 0 of an image it is given, else those missing
    int first_level_to_build(bool given) const { return given ? 1 : levels; }
    int slot() const { return cur; }
    void invalidate() { valid = false; }
    void commit(int cur_, int cols_, int rows_, int levels_) {
        cur = cur_; cols = cols_; rows = rows_; levels = levels_;
        valid = true;
    }

private:
    int cur = 0, cols = 0, rows = 0, levels = 0;
    bool valid = false;
};

// What the frontend entry points keep between calls (lh_frontend.cpp, lh_frame.cpp)
struct FrontendState {
    // frontend pose-only batch (lh_estimate_pose)
    // inputs and outputs each packed into one arena, so a call is one upload and one download
    // through pinned staging (a single frame is latency-bound: every extra copy costs ~10 us)
    DevBuf<uint8_t> f_in, f_out;
    DevBuf<double> f_res;
    HostBuf<uint8_t> s_fin, s_fout;
    // optical flow (lh_lk_track, lh_klt_track; the stereo calls read them in place): both images' pyramids, keypoints
    DevBuf<uint8_t> k_img[2], k_succ;
    DevBuf<float> k_kp1, k_kp2;
    // triangulation (lh_triangulate, lh_stereo_landmarks): the inputs packed into one arena, the outputs into another
    DevBuf<uint8_t> t_in, t_out;
    // feature detection (lh_detect_features): image, allow and state bytes; lambda; candidate and corner lists
    DevBuf<uint8_t> g_img, g_allow, g_state;
    DevBuf<double> g_eig, g_acc_lam, g_resp;
    DevBuf<uint32_t> g_cand, g_acc_idx;
    DevBuf<float> g_excl, g_kp;
    DevBuf<lh_gftt_ctl> g_ctl;
    HostBuf<lh_gftt_ctl> s_gctl;   // pinned: read back once per batch of selection rounds
    // one frame of Frontend::Track (lh_track_frame).  The resident image is the last successful call's img2; a call
    // reads it as img1 and makes its own img2 the other buffer.  lh_insert_keyframe reads it as its left image, or
    // replaces it with the one it is given; no other entry point touches it.
    ResidentImage res;
    // its arenas (lh_frontend_layout.h TrackLayout): one upload, one download, and k_frames' inputs as k_track_pack
    // writes them
    DevBuf<uint8_t> tk_in, tk_out, tk_work;
    HostBuf<uint8_t> s_tkin, s_tkout;
    // a keyframe's half of the frame (lh_insert_keyframe).  Its left image is the resident one above, which the detector
    // and the tracker read in place; the right image's pyramid (the resident layout) is this call's own.  One input
    // arena and one download arena (KeyframeLayout), the slots' states.
    DevBuf<uint8_t> kf_right, kf_in, kf_out, kf_state;
    HostBuf<uint8_t> s_kfin, s_kfout;
};

// The returned state of the last solve, linearised again (lh_cov_host.cpp relin_enqueue; lh_covariance and
// lh_marginalize each keep one): a second set of lh_reset_args holding that state, and everything the linearisation
// there writes that the solve's own state also holds (controller, step, poses, tables, records, reduced system), so
// that the handle's solver state is only read
struct ReLin {
    DevBuf<double> qt_init, ptab_init, lm;     // the snapshot: lh_reset_args' three arrays
    DevBuf<double> qt, ptab, rec, dxp, rs, maxd;
    DevBuf<lh_ctrl> ctrl;
};

// What lh_covariance keeps between calls (lh_cov_host.cpp)
struct CovState {
    ReLin lin;
    DevBuf<int32_t> rowmap;
    DevBuf<double> A, W, full;                 // S[f, f] and its factor, L^-1, Sigma_pp (when it is not downloaded)
    DevBuf<double> out;                        // the download: the result block, then the arrays asked for
};

// What lh_marginalize keeps between calls (lh_marg_host.cpp): the observation words with the edges outside M masked
// out, and the per-edge outputs of the linearisation on them (the solve's own rho0 and inlier flags stay as they are)
struct MargState {
    ReLin lin;
    DevBuf<uint32_t> meta;
    DevBuf<int32_t> counts;
    DevBuf<double> rho;
    DevBuf<uint8_t> wflag;
    DevBuf<double> prior;                      // the earlier prior as uploaded: H [6P][6P], then b [6P]
    HostBuf<double> s_prior;                   // its pinned staging
    DevBuf<double> A, b, Y;                    // A_M + the earlier prior (lower), its right-hand side, C^-1 A[m, :] and C^-1 b[m]
    DevBuf<double> out;                        // the download: the result block, H_prior, b_prior, lm_marginalised
};

}  // namespace lh

struct lh_handle {
    template <typename T> using DevBuf = lh::DevBuf<T>;
    template <typename T> using HostBuf = lh::HostBuf<T>;
    template <typename T> using View = lh::View<T>;
    lh_options opt;
    int device = 0;
    int lds_limit = 160 * 1024;   // hipDeviceAttributeMaxSharedMemoryPerBlock of the device
    int n_cu = 256;               // hipDeviceAttributeMultiprocessorCount of the device (the planner's k_lin shape)
    hipStream_t stream = nullptr;
    lh::Transport transport = lh::TR_NONE;
    ncclComm_t comm = nullptr;    // TR_RCCL's communicator
    lh::P2pState p2p;             // TR_P2P's buffers and counters
    bool uploaded = false;
    bool upload_joined = false;   // this upload has taken part in the sharded envelope all-reduce
    bool upload_tail = false;     // ... and every rank passed it: the upload's closing status all-reduce follows
    lh::Pool* pool = nullptr;

    // window
    lh::Plan plan;
    int P = 0, L = 0, ncam = 1, n_rec = 0;
    int64_t O = 0, n_slots = 0;
    lh_params prm{};
    lh_rs_layout LY{};
    double last_prep_ms = 0.0, last_upload_ms = 0.0;

    // pinned staging of the upload
    View<lh_chunk> s_chunks;                                  // the per-window tables: views into s_arena
    View<lh_subbatch> s_sbs;
    View<uint32_t> s_items, s_pair_ptr, s_rsmap, s_brow_ent, s_red;
    View<uint16_t> s_pair_pq;
    View<uint16_t> s_units;                                   // k_ctrl's work units (lh_ctrl_units)
    View<uint16_t> s_bunits;                                  // k_ctrl_b's work units
    View<int32_t> s_bblk;                                     // k_ctrl_b's pair -> block table
    View<int32_t> s_lm_perm, s_brow_ptr;
    View<uint64_t> s_fixed;
    View<double> s_qt, s_ptab, s_ext;
    HostBuf<uint8_t> s_arena;
    size_t arena_bytes = 0;
    HostBuf<uint32_t> s_meta;
    HostBuf<int32_t> s_obs_perm;
    HostBuf<float> s_uv;                                     // pixels, 2 floats per slot
    HostBuf<double> s_lm, s_rs;                              // s_rs: the host-exchange buffer
    HostBuf<double> s_out;                                   // pinned staging of the download
    DevBuf<unsigned> d_ocnt;                                 // the outlier pass's per-block counts (ABI 5)
    DevBuf<uint8_t> d_oflag;                                 // its flags (window order), then threshold and counts
    DevBuf<double> d_otot;                                   // a sharded pass: this rank's counts, then all ranks' sums
    HostBuf<uint8_t> s_oflag;                                // pinned staging of the flags
    hipEvent_t ev_staging = nullptr;   // the upload's last copy out of the staging (reused by the next upload)
    bool staging_pending = false;

    // device buffers
    View<lh_chunk> d_chunks;                                  // the per-window tables: views into d_arena
    View<lh_subbatch> d_sbs;
    View<uint32_t> d_pair_ptr, d_items, d_rsmap, d_red;
    int n_red = 0;   // k_reduce's pair blocks (d_red: 4 words each, then the scalar block's sentinel)
    View<uint16_t> d_pair_pq, d_units, d_bunits;
    View<int32_t> d_bblk;
    DevBuf<double> d_band;        // k_ctrl_b's scratch per ladder rung (lh::band_scratch)
    lh::SolveConfig cfg;          // how the uploaded window is solved (lh::solve_config): the controller kind and its sizes
    View<int32_t> d_lm_perm;
    View<double> d_ptab_init, d_qt_init, d_ext;
    DevBuf<uint8_t> d_arena;
    DevBuf<uint32_t> d_meta;
    DevBuf<int32_t> d_obs_perm;
    DevBuf<float> d_uv;
    DevBuf<double> d_lm_in, d_rec, d_ptab, d_qt, d_rho, d_rows, d_csc, d_gA, d_gS, d_rs_stage,
        d_rs_commit, d_maxd, d_dxp, d_out_xyz, d_out_rho;
    DevBuf<lh_ctrl> d_ctrl;
    View<uint64_t> d_fixed;      // fixed-pose bits (Plan::fixed_bits)
    View<int32_t> d_brow_ptr;    // the reduced system's block rows (Plan::brow_ptr / brow_ent, k_ctrl_p)
    View<uint32_t> d_brow_ent;
    DevBuf<uint8_t> d_wflag;     // [2][n_slots] inlier flags of each state buffer's linearisation (k_lin)
    DevBuf<double> d_img;        // [2][LH_IMG_SZ] k_ctrl's LDS system image, staged / committed (prm.img)
    lh::FrontendState fe;
    lh::CovState cov;
    lh::MargState marg;
    bool solved = false;         // a solve of the uploaded window has completed (lh_covariance, lh_marginalize read its state)
    lh_ctrl* h_ctrl = nullptr;   // pinned
    int last_chains = -1;        // lh_debug_chains: the last synchronous solve's stop chain
    int last_lskips = -1;        // lh_debug_ladder: its rejections onto a built ladder rung
    int last_batches = -1;       // lh_debug_batch: its batches of evaluate-only rungs
    int last_retrials[2] = {-1, -1};   // lh_debug_batch: their acceptances (re-run; re-run and stopping)
    size_t rho_off = 0;          // the last solve's per-edge rho0 "as last evaluated": its rung buffer in d_rho (a batch)
    int* h_done = nullptr;       // pinned, mapped lh_host_words: [0] k_ctrl raises it when the LM loop stops, [1] progress
                                 // word 2 * (last live trial) + (one iteration from max_iters)
    int* d_done = nullptr;       // device alias of h_done

    // per-solve bookkeeping
    int64_t n_coll = 0;          // data-path all-reduces of the last solve

    // profiling
    struct PendingEv { int kc; int trial; hipEvent_t a, b; };
    std::vector<PendingEv> pending;
    int cur_trial = 0;
    std::vector<hipEvent_t> event_pool;
    size_t event_next = 0;
    int64_t launches[lh::KC_N] = {0};
    double total_ms[lh::KC_N] = {0};
};

namespace lh {

inline bool g_debug = getenv("LH_DEBUG") != nullptr;

#define HIPCHK(x)                                                                                        \
    do {                                                                                                 \
        hipError_t e_ = (x);                                                                             \
        if (e_ != hipSuccess) {                                                                          \
            if (lh::g_debug) fprintf(stderr, "lego_ba: %s failed: %s\n", #x, hipGetErrorString(e_));   \
            return LH_E_HIP;                                                                             \
        }                                                                                                \
    } while (0)

#define NCCLCHK(x)                                                                                       \
    do {                                                                                                 \
        ncclResult_t r_ = (x);                                                                           \
        if (r_ != ncclSuccess) {                                                                         \
            if (lh::g_debug) fprintf(stderr, "lego_ba: %s failed: %s\n", #x, ncclGetErrorString(r_));  \
            return LH_E_RCCL;                                                                            \
        }                                                                                                \
    } while (0)

// a step that returns a status: any but LH_OK is the caller's return value
#define STAGE(x)                                                                                         \
    do {                                                                                                 \
        const int st_ = (x);                                                                             \
        if (st_ != LH_OK) return st_;                                                                    \
    } while (0)

// the next event of the handle's pool (nullptr: none could be created); the taker puts the pool back (event_next = 0)
hipEvent_t next_event(lh_handle* h);

// One call on the handle's stream (the frontend's entry points, lh_covariance): the device selection, the two events
// around its kernels (start() in front of the first, stop() behind the last), time_ms once the stream has drained, and
// on every way out (the error returns included) the handle's event pool put back.
struct FrontendCall {
    lh_handle* h;
    hipStream_t s;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    explicit FrontendCall(lh_handle* hh) : h(hh), s(hh->stream) {}
    ~FrontendCall() { h->event_next = 0; }
    int select() { return hipSetDevice(h->device) == hipSuccess ? LH_OK : LH_E_HIP; }
    int record(hipEvent_t* e) {
        if (!(*e = next_event(h))) return LH_E_HIP;
        HIPCHK(hipEventRecord(*e, s));
        return LH_OK;
    }
    int start() { return record(&e0); }
    int stop() { return record(&e1); }
    int time(double* time_ms) {   // after the call's last synchronise
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        *time_ms = ms;
        return LH_OK;
    }
};

// the staging copies build std::vectors (par_copy): no exception crosses the ABI
template <typename In, typename Out>
int no_throw(int (*impl)(lh_handle*, const In*, Out*), lh_handle* h, const In* in, Out* out) {
    try {
        return impl(h, in, out);
    } catch (...) {
        return LH_E_HIP;
    }
}

// host copies between caller memory and pinned staging, in ~256 KB blocks over the planner's pool
struct ByteSeg { void* dst; const void* src; size_t n; };
void par_copy(lh_handle* h, const ByteSeg* seg, int nseg);

// The linearisation at the state the last solve returned (lh_cov_host.cpp): relin_ensure sizes rl's buffers for the
// uploaded window; relin_enqueue puts k_cov_snapshot, k_lin<T, false> and k_reduce (mode 0) on the handle's stream,
// unchanged, writing rl alone: the lambda-free packed system in rl.rs, the records with chol(H_ll) in the second half
// of rl.rec, the committed pose tables in rl.ptab_init.  meta: the observation words to linearise; rho [n_slots] and
// wflag [2][n_slots]: where k_lin writes its per-edge rho0 and inlier flags; prm: k_lin's and k_reduce's parameters.
int relin_ensure(lh_handle* h, ReLin& rl);
int relin_enqueue(lh_handle* h, ReLin& rl, const uint32_t* meta, double* rho, uint8_t* wflag, const lh_params& prm);

}  // namespace lh
