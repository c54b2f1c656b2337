// lh_plan.h — window preprocessing for the device layout (host only, no HIP).
//
// One sliding window (include/lego_ba.h lh_window) becomes:
//   * a landmark-major order of the observations, each landmark's observations in ascending pose
//     order (the reference visits edges in unordered_map order, problem.cpp:285; any order is the
//     same problem);
//   * landmarks ordered by observation span and packed into chunks whose union of observing poses
//     fits one MFMA window (<= LH_UMAX poses), chunks split into wave sub-batches (<= 8 landmarks,
//     <= 64 observations, landmark l owning the aligned lane group [l*G, l*G + k_l));
//   * the reduce plan: for every pose pair p <= q, the chunks whose slab holds a block of it.
// Two phases so the bulk arrays are written once, straight into the caller's (pinned) staging:
// plan_structure() sizes everything (O(O) scan + O(L) ordering), plan_fill() writes the arrays.
// Both run on a small thread pool; the result does not depend on the thread count.
#pragma once
#include <stdint.h>

#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/lego_ba.h"
#include "lh_common.h"

namespace lh {

// Persistent worker pool: run(n, fn) calls fn(i) for i in [0, n) on the workers and the caller.
// The job hand-off is lock-free (Pool::loop); an idle worker polls the job generation briefly
// (kSpin pauses) and then sleeps on the condition variable.  Polling longer (300 us after each job,
// so that a planning pass's back-to-back jobs never wait for a wake-up) measured slower on the box's
// 16-CPU cgroup share: lh_solve's preprocessing 1.80 ms against 1.49 ms.
class Pool {
  public:
    explicit Pool(int threads);
    ~Pool();
    int size() const { return (int)workers_.size() + 1; }
    void run(int n, const std::function<void(int)>& fn);

  private:
    struct Job {
        const std::function<void(int)>* fn = nullptr;
        int n = 0;
        std::atomic<int> next{0};
    };
    static constexpr unsigned kSpin = 256;
    void loop();
    std::vector<std::thread> workers_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::atomic<Job*> job_{nullptr};    // the live job, nullptr once run() retires it
    std::atomic<uint64_t> gen_{0};      // bumped per job
    std::atomic<int> active_{0};        // workers that may still touch job_'s job
    std::atomic<int> sleepers_{0};
    std::atomic<bool> stop_{false};
    std::vector<int> pinned_;           // the CPU id each worker is pinned to (its use count released on destruction)
};

struct PlanCfg {
    int chunk_lm = 0;      // landmarks per chunk; 0 = auto (~512 chunks, 2 workgroups per CU; or the 8-wave shape)
    bool rank_invariant_pairs = false;   // P > LH_PMAX_WIN: list every pair within the 64-pose span (sharded solves)
    // ---- k_lin's workgroup shape (Plan::lin_waves; plan_structure's chunking stage has the rule) ----
    int n_cu = 256;        // the device's compute units (256 where there is no device: the CPU tests)
    bool no_wg8 = false;   // Switches::no_lin_wg8: always 4 waves
    bool force_wg8 = false;   // Switches::test_lin_wg8: 8 waves on any chunking whose chunks are all T <= 3
    // k_lin's dynamic LDS for (T, cameras, waves) and the device's limit: 8 waves are refused where they do not
    // fit (null: no device, every shape fits)
    size_t (*lin_smem)(int T, int ncam, int nw) = nullptr;
    size_t lds_limit = 0;
};

struct Plan {
    // ---- sizes (plan_structure) ----
    int P = 0, L = 0, ncam = 1;
    int64_t O = 0;
    int n_chunks = 0, n_sb = 0, n_items = 0, npairs = 0;
    int n_rec = 0;                      // landmark records (8 per sub-batch)
    int64_t n_slots = 0;                // observation slots (64 per sub-batch)
    int tgroup_begin[LH_TMAX + 2] = {0};
    int lin_waves = LH_WAVES;           // waves per k_lin workgroup: LH_WAVES, or LH_WAVES_WG8 (every chunk T <= 3)
    int chunk_lm = 0;                   // the landmarks-per-chunk bound the chunks were cut with
    uint64_t fixed_mask = 0;            // bit p: pose p < 64 is fixed (fixed_bits[0])
    std::vector<uint64_t> fixed_bits;   // [(P + 63) / 64] bit p % 64 of word p / 64: pose p is fixed
    std::vector<uint16_t> pair_list;    // [2 npairs] (p, q), p <= q, of each reduced-system block
    // the blocks by block row (the PCG's S p, k_ctrl_p): row p holds, in ascending column q, entry
    // (b << 13) | (q << 1) | t for block b = pair (min(p, q), max(p, q)), t = 1 where it is read transposed
    std::vector<int32_t> brow_ptr;      // [P + 1]
    std::vector<uint32_t> brow_ent;     // [2 npairs - P]
    // ---- internal (reused across windows) ----
    std::vector<int64_t> lm_ptr;        // [L+1] CSR over landmarks
    std::vector<int64_t> csr;           // [O] window obs, landmark-major, ascending pose
    std::vector<uint64_t> lm_mask;      // [L] observing-pose mask, bit i = pose lm_base + i
    std::vector<int32_t> lm_base;       // [L] first observing pose
    std::vector<int32_t> order;         // [L_act] landmarks with edges, span order
    std::vector<uint64_t> ord_mask;     // [L_act] lm_mask / lm_base / log2 lane group, in span order
    std::vector<int32_t> ord_base;
    std::vector<uint8_t> ord_lg;
    std::vector<int32_t> chunk_lm0;     // [n_chunks + 1] chunk c owns order[chunk_lm0[c] .. chunk_lm0[c+1])
    std::vector<uint64_t> chunk_mask;   // [n_chunks] union pose mask, bit i = pose chunk_base + i
    std::vector<int32_t> chunk_base;    // [n_chunks]
    std::vector<int32_t> chunk_sb0;     // [n_chunks + 1] sub-batch prefix (chunks in T order)
    std::vector<int32_t> corder;        // [n_chunks] launch order (grouped by T) -> chunk
    std::vector<int32_t> sb_lm0;        // [n_sb + 1] sub-batch -> first position in order[]
    std::vector<uint8_t> sb_lg;         // [n_sb]
    std::vector<uint32_t> pair_ptr;     // [npairs + 1]
    std::vector<uint32_t> chunk_ib;     // [n_chunks + 1] first item of each chunk (launch order)
    double t_stage[8] = {0};            // diagnostic: ms at plan_structure's stage ends (lhp_plan_stages)
};

struct PlanOut {
    lh_chunk* chunks;        // [n_chunks]
    lh_subbatch* sbs;        // [n_sb]
    uint32_t* meta;          // [n_slots]
    float* uv;               // [2 n_slots] pixels as float: toVec2 of cv::KeyPoint::pt (algorithm.h:37),
                             // so every measurement is a float (plan_structure rejects one that is not)
    int32_t* obs_perm;       // [n_slots] slot -> window obs (-1: padding)
    int32_t* lm_perm;        // [n_rec] record -> window landmark (-1: padding)
    uint32_t* items;         // [n_items] per chunk (launch order), per slot pair (s <= t): its pair row
    uint16_t* pair_pq;       // [2 npairs]
    uint32_t* rsmap;         // [npairs * 36]
    double* lm_xyz;          // [3 L] copy of the window's positions (nullptr: not wanted)
};

// lh_status.  LH_E_BADARG for out-of-range indices, LH_E_UNSUPPORTED outside the envelope
// (DESIGN.md "Limits"), LH_E_EMPTY mirrors problem.cpp:157-161.
int plan_structure(const lh_window* w, const PlanCfg& cfg, bool allow_empty, Plan& pl, Pool* pool);
// on_slots(slot_begin, slot_end), if given, is called on the calling thread each time the observation
// slots [slot_begin, slot_end) (meta, uv, obs_perm) are final, in ascending order, so the caller can
// start copying them while the rest is filled; `batches` splits the chunk pass for that.
using SlotsReady = void (*)(void* user, int64_t slot_begin, int64_t slot_end);
// Returns LH_OK (the window was validated by plan_structure).
int plan_fill(const lh_window* w, const Plan& pl, const PlanOut& out, Pool* pool, SlotsReady on_slots = nullptr,
              void* user = nullptr, int batches = 1);

// ---------------------------------------------------------------------------------------------
// A window's solve configuration: which controller runs it, with which tables and
// scratch sizes.  Pure functions of the plan, the handle's options and the environment switches;
// lh_host.cpp allocates, fills and launches from what they return and decides nothing itself.
// ---------------------------------------------------------------------------------------------

// The environment switches of the solve configuration (A/B hooks of the bitwise tests and bench.py).
// Read once per upload: a caller sets a variable and then uploads through a new solver.
struct Switches {
    bool no_band = false;         // LH_NO_BAND: past LH_PMAX poses LDL^T never runs banded (k_ctrl_g, up to LH_PMAX_WIN)
    bool no_ladder = false;       // LH_NO_LADDER: one lambda-ladder rung
    bool no_red_skip = false;     // LH_NO_RED_SKIP: k_reduce keeps the blocks of pose pairs no chunk couples
    bool no_narrow = false;       // LH_NO_NARROW: k_ctrl_b's two-rows-per-lane back substitution on every window
    bool no_batch = false;        // LH_NO_BATCH: one evaluate-only rung per chain
    int batch_max = INT32_MAX;    // LH_BATCH_MAX=m: at most m (at least 1) rungs per batch
    bool nd = false;              // LH_ND=1: k_ctrl's two-chain schedule where the window splits (LDL^T)
    bool no_evo = false;          // LH_NO_EVO: every trial linearises in full
    bool no_eval_first = false;   // LH_NO_EVAL_FIRST: a trial after a rejection is linearised, not only evaluated
    bool ladder_lazy = false;     // LH_LADDER_LAZY: only a factor after a rejection builds the ladder
    bool no_bimg = false;         // LH_NO_BIMG: k_ctrl_b's loaders read the packed blocks, not k_reduce's band image
    bool no_img = false;          // LH_NO_IMG: k_ctrl scatters the packed system, not k_reduce's LDS image
    bool no_lin_wg8 = false;      // LH_NO_LIN_WG8: k_lin keeps 4 waves per workgroup on a window that fills the GPU
    bool test_lin_wg8 = false;    // LH_TEST_LIN_WG8=1 (tests): k_lin's 8-wave shape on any window of T <= 3 chunks,
                                  // whatever its chunking
};
// the switches that enter the plan itself
inline void apply_switches(PlanCfg& cfg, const Switches& sw) {
    cfg.no_wg8 = sw.no_lin_wg8;
    cfg.force_wg8 = sw.test_lin_wg8 && !sw.no_lin_wg8;
}
Switches read_switches();

// pf[p]: pose p's first coupled pose, the lowest pose of any chunk window holding p (a chunk writes a
// block for every pair of its window): the envelope of S in natural pose order.  A sharded solve
// factors the sum of every rank's blocks, so it unites the ranks' envelopes before solve_config.
std::vector<int> plan_envelope(const Plan& pl);

constexpr int kBandSteps = 6 * LH_PMAX_ANY / 8;   // k_ctrl_b's steps at most (its unit table's row length)

// k_ctrl_b's unit table [16][kBandSteps] for an n-row system (lh_ctrl_units): the 11 unit waves when
// every step fits them (*lu false, k_ctrl_b<false>), else the stream loaders take units too.  Returns
// the most units a step needed (more than LH_BAND_UNIT_WAVES: the window cannot run banded).
int band_units(int n, const int32_t* fcb, uint16_t* units, bool* lu);

// k_ctrl_b's global scratch per ladder rung, in doubles: the L rows [ceil16(6P)][128], then ND per
// block [kBandSteps][64]
struct BandScratch {
    size_t nd_off, per_rung;
};
inline BandScratch band_scratch(int P) {
    const size_t NE = (size_t)((6 * P + 15) & ~15);
    return {NE * 128, NE * 128 + (size_t)kBandSteps * 64};
}

// What is needed before a sharded upload's envelope collective, to size what every rank allocates
// alike: may the window run banded at all (the arena reserves k_ctrl_b's tables), and the ladder's rungs.
bool band_possible(int P, int linear_solver, const Switches& sw);
int ladder_rungs(int max_trials, const Switches& sw);

struct SolveIn {
    int P = 0;
    size_t n_brow_ent = 0;        // Plan::brow_ent.size()
    const int* pf = nullptr;      // [P] plan_envelope, united over the ranks
    int lin_waves = LH_WAVES;     // Plan::lin_waves
    int linear_solver = LH_SOLVER_LDLT, max_trials = 1, world_size = 1;
    bool rccl = false;            // the trials' exchange is an RCCL all-reduce
    Switches sw;
};

struct SolveConfig {
    int kind = LH_CTRL_LDS;       // lh_ctrl_kind: the controller kernel
    int lin_waves = LH_WAVES;     // k_lin's waves per workgroup (the plan's choice; every k_lin launch follows it)
    bool band_narrow = false;     // k_ctrl_b: every row's envelope starts within 56 rows of its 8-row block
    bool band_lu = false;         // k_ctrl_b: some step needs the stream loaders as unit waves too
    int ladder = 1, batch = 1;    // lambda-ladder rungs; evaluate-only rungs per batch
    int ladder_eager = 1, no_evo = 0, eval_first = 1;   // lh_params fields that are switches alone
    int dec_in_reduce = 0, commit_in_reduce = 0, img = 0, bimg = 0;   // lh_params fields of the same names
    lh_ctrl_nd nd{};              // k_ctrl's two-chain schedule (nd.nsteps 0: the one-chain one)
    size_t lad_stride = 0;        // doubles of d_gA per ladder rung (k_ctrl_g, k_ctrl_p)
    size_t n_band = 0;            // doubles of d_band per ladder rung (k_ctrl_b: band_scratch)
    size_t n_gA = 0, n_gS = 0;    // doubles of d_gA (every rung) and d_gS (k_ctrl_g, k_ctrl_p)
    size_t n_img = 0;             // doubles of d_img (img: k_ctrl's two LDS images; bimg: k_ctrl_b's two band images)
    std::vector<uint16_t> units;  // the controller's work units: k_ctrl's [16][LH_NSTEP], k_ctrl_b's [16][kBandSteps]
    // lh_debug_controller's word
    int debug_word() const { return kind | (band_narrow ? 1 << 8 : 0) | (band_lu ? 1 << 9 : 0); }
};
// LH_OK, or LH_E_UNSUPPORTED: LDL^T past LH_PMAX_WIN poses on a window that cannot run banded
int solve_config(const SolveIn& in, SolveConfig& out);

// ---------------------------------------------------------------------------------------------
// The trial schedule of a solve: how many chains the host may enqueue, and how far ahead of the
// device.  lh_host.cpp's enqueue loop, its top-up and lh_create's option comparison all read it here.
// With more than one rank every rank must issue the same number of exchanges per solve:
//   * the progress word (2 * last live chain + near) only advances on live chains, so it never passes
//     the stop chain s, and may_enqueue keeps a rank's count within s + depth;
//   * s is decided on identical all-reduced data, so every rank tops up to the same topup_target(s).
// tests/test_trial_schedule_cpu.py checks both by simulation.
// ---------------------------------------------------------------------------------------------
struct TrialSchedule {
    int max_total;   // trials a solve can run: every trial, plus one re-linearisation chain per iteration at most
                     // (an evaluate-only acceptance, ctrl.relin)
    int depth;       // trials kept enqueued past the progress word (1: the synchronous host transport)
};
TrialSchedule trial_schedule(int max_iters, int max_trials, int eval_first, int trials_per_sync, bool host_transport);
// May one more trial be enqueued, `enqueued` being out already?  progress: the mapped progress word, -1
// before the first decision; its low bit (the next completed iteration reaches max_iters) allows one ahead.
// (inline: the enqueue loop spins on it)
inline bool may_enqueue(const TrialSchedule& ts, int progress, int enqueued) {
    const int last = progress < 0 ? -1 : (progress >> 1);
    return enqueued - last < ((progress >= 0 && (progress & 1)) ? 1 : ts.depth);
}
// The count every rank reaches after the device stopped on chain stop_chain (lh_ctrl.seq_last)
int topup_target(const TrialSchedule& ts, int stop_chain);

// k_reduce's blocks, one per pose pair that some chunk's rows reach ({block, first row, end row, p | q << 16}),
// then the scalar block's sentinel, into out[4 (npairs + 1)].  One rank skips the pairs no chunk couples:
// their blocks of S are zero for the whole window (the caller clears the reduced-system buffers per
// window).  A sharded solve keeps every pair: a rank's empty pair still has to write its zero
// contribution over last trial's all-reduced sum.  Returns the pair blocks listed.
bool reduce_skip(int world_size, const Switches& sw);
int reduce_table(const Plan& pl, bool skip, uint32_t* out);

// k_ctrl_b's pair -> block table: bblk[p * 64 + d] is the block of pose pair (p, p + d), -1 if absent
void band_block_table(const Plan& pl, int32_t* bblk);

}  // namespace lh
