// lh_ctrl_b.hip — k_ctrl_b, the banded controller, and its band helpers.
// Not a unit of its own: lh_kernels.hip includes it (see there).

// ============================================================================
// k_ctrl_b: the controller for windows past LH_PMAX poses whose reduced system is banded (the
// reference's live solver, LDL^T, problem.cpp:420, at any window size).  In
// natural pose order a sliding window's S is block-banded: a landmark couples the poses of its run
// of keyframes, so row r's nonzeros start at its envelope fc(r) >= r - 104 (the host checks this per
// window, lh_host.cpp; other windows go to k_ctrl_g or PCG).  The blocked LDL^T of k_ctrl then needs
// only 8 tile rows (128 rows) of S at a time: the window holds them in one CU's LDS as a circular
// buffer (BandSys), and waves 12-15 stream the next tile row in, written into the slots of the tile row
// that just retired: one rank reads it from the band image k_reduce wrote in the loaders' order (prm.bimg,
// two steps ahead); a sharded solve from the all-reduced packed blocks (block indices two steps ahead,
// values one step ahead).  L goes
// to global memory row by row, ND per block; the back substitution (one wave) reads them back.  The
// per-step work units come from the same envelope (lh_ctrl_units over 11 unit waves).  One 1024-thread
// workgroup; the LM bookkeeping is k_reduce's (dec_in_reduce: one rank) or thread 0's (the initial
// linearisation); k_reduce also commits accepted systems (commit_in_reduce), so nothing here copies S.
// ============================================================================
// Where the blocked LDL^T (lh_ldlt.h, beside LdsSys) keeps k_ctrl_b's operands: a 128-row circular window of the
// lower band in LDS (row r at r mod 128, column c at c mod 128: no two live entries of a band narrower than the
// window share a slot), the rhs in its own LDS array, L rows to global memory (L[r][c] at
// Lg[r * LH_LBW + c - r + LH_LBW], c in [r - LH_LBW, r)).
#define LH_LBW 128   // k_ctrl_b: L entries kept per row (columns r - 128 .. r - 1)
struct BandSys {
    static constexpr bool rewrite_masked = false;
    double* A;   // LDS, 128 rows of stride AS
    double* y;   // LDS rhs
    double* Lg;  // global, LH_LBW per row
    __device__ __forceinline__ double& at(int r, int c) const { return A[(r & 127) * AS + (c & 127)]; }
    __device__ __forceinline__ double& rhs(int r) const { return y[r]; }
    __device__ __forceinline__ void store_l(int r, int c, double v) const { Lg[(size_t)r * LH_LBW + (c - r + LH_LBW)] = v; }
    __device__ __forceinline__ int wrap(int x) const { return x & 127; }
    __device__ __forceinline__ double& atw(int r, int c) const { return A[r * AS + c]; }
};
template <bool B> struct BoolTag { static constexpr bool value = B; };
constexpr int BNMAX = 6 * LH_PMAX_ANY;  // largest reduced system (1536 rows)
constexpr int BSTEP_MAX = BNMAX / 8;    // LDL^T steps
// the stream loaders: waves 12-15 (moving them off wave 0's SIMD, to 11 and 13-15, measured slower: the
// wave forming z then set the step); z and the ND copy are wave LH_BZW's (below)
__device__ __forceinline__ bool band_loader(int w) { return w >= 12; }
__device__ __forceinline__ int band_loader_slot(int w) { return w - 12; }
#ifndef LH_BZW
#define LH_BZW 8   // the wave that forms z and copies ND out: a unit wave idle in most steps (wave 12, a loader:
                    // P = 128 0.2113 against 0.2104 ms per trial, profiles/r05l_band_ab_bzw8.txt)
#endif
constexpr int BZW = LH_BZW;

// S(r, c), c <= r < n, of the packed system: block (pose(c), pose(r)) through the per-window table
// bblk[p * 64 + d] (the block of pose pair (p, p + d), -1 where no chunk couples them)
__device__ __forceinline__ int band_block(const int32_t* __restrict__ bblk, int r, int c, int n) {
    const int pc = c / 6, pr = r / 6, d = pr - pc;
    return (c <= r && r < n && d < 64) ? bblk[pc * 64 + d] : -1;
}
__device__ __forceinline__ double band_value(const double* __restrict__ src, int blk, int r, int c, double lambda,
                                             int strategy, int n) {
    double v = (blk >= 0) ? src[(size_t)blk * 36 + (c % 6) * 6 + (r % 6)] : 0.0;
    if (r == c) {
        if (r >= n) v = 1.0;   // identity padding
        else v = (strategy == 0) ? v + lambda : v + lambda * v;
    }
    return v;
}

// LU: some step needs more than the 11 unit waves (chunk windows of ~16 poses), so the stream loaders take units
// too (a separate instantiation: the loaders' unit path costs ~1 % where no step needs it)
template <bool LU>
__global__ __launch_bounds__(CT) void k_ctrl_b(lh_ctrl* __restrict__ ctrl, const double* __restrict__ rs_commit,
                                               const double* __restrict__ rs_stage, const double* __restrict__ maxd_in,
                                               const int32_t* __restrict__ bblk, const uint16_t* __restrict__ bunits,
                                               double* __restrict__ Lg, double* __restrict__ NDg, double* __restrict__ dxp,
                                               lh_params prm, int mode, volatile int* __restrict__ host_done, int seq,
                                               const double* __restrict__ bimg) {
    __shared__ __attribute__((aligned(16))) double A[128 * AS];   // the circular window of the lower band
    __shared__ __attribute__((aligned(16))) double y[BNMAX];   // rhs (forward substitution), then x
    __shared__ double z[BNMAX];                             // D^-1 L^-1 b
    __shared__ __attribute__((aligned(16))) double Nl[2][64], NDl[2][64];
    __shared__ double s_red[CT / 64];
    __shared__ CtrlDecLds s_dec;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int P = prm.P, n = 6 * P, NE = (n + 15) & ~15, nb = (n + 7) & ~7, NT = NE / 16, nstep = nb / 8;
    const lh_rs_layout LY = lh_rs_make(P, prm.npairs);
    const int rung = (int)blockIdx.x;
    CSTAMP_START;
    // ---------------- the LM decision (workgroup `rung` > 0: a lambda-ladder rung with its own L rows and ND) ----------------
    const CtrlDec dec = ctrl_take_decision<CT>(ctrl, prm, mode, rs_stage, LY, maxd_in, host_done, seq, s_red, s_dec);
    if (!dec.run) return;
    const int accept = dec.accept;
    const double lambda = dec.lambda;
    Lg += (size_t)rung * ((size_t)NE * LH_LBW + (size_t)BSTEP_MAX * 64);   // lh_band_args: per rung, L rows | ND
    NDg += (size_t)rung * ((size_t)NE * LH_LBW + (size_t)BSTEP_MAX * 64);
    dxp += (size_t)rung * n;
    CSTAMP_LIVE();
    CSTAMP(1);
    const double* __restrict__ src = accept ? rs_stage : rs_commit;
    // prm.bimg: k_reduce wrote the band in the loaders' order (lh_bimg_idx; staged, then committed): one load per
    // element, no block-index round trip before it
    const bool bim = prm.bimg != 0;
    const double* __restrict__ bsrc = bimg + (accept ? 0 : (size_t)NT * LH_BIMG_TR);

    // ---------------- the rhs, the first 8 tile rows, this wave's unit words ----------------
    for (int i = tid; i < NE; i += CT) {
        y[i] = (i < n) ? src[LY.off_bs + i] : 0.0;
        z[i] = 0.0;
    }
    {
        // 16 elements of the first window per thread: element k at row 8 k + tid / 128, column tid mod 128, so a
        // wave's writes go to consecutive columns (one row of 16-column stripes per thread put 8 lanes of a
        // 16-lane write group on one bank pair)
        constexpr int PER = 128 * 128 / CT;
        const int c0 = tid & 127, rr = tid >> 7;
        int bk[PER];
        if (bim) {
            double bv[PER];
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int r = 8 * k + rr;
                bv[k] = (r < NE && c0 <= r) ? bsrc[lh_bimg_idx(r, c0)] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int r = 8 * k + rr;
                double v = bv[k];
                if (r == c0) v = (r >= n) ? 1.0 : ((prm.strategy == 0) ? v + lambda : v + lambda * v);
                A[r * AS + c0] = v;
            }
        } else {
#pragma unroll
            for (int k = 0; k < PER; ++k) bk[k] = band_block(bblk, 8 * k + rr, c0, n);
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int r = 8 * k + rr;
                A[r * AS + c0] = (r < NE && c0 <= r) ? band_value(src, bk[k], r, c0, lambda, prm.strategy, n) : 0.0;
            }
        }
    }
    uint32_t uwa = 0, uwb = 0;   // this wave's unit words: steps 2j, 2j + 1 in u32 j (lane j, lane j + 64)
    {
        const uint32_t* uw32 = reinterpret_cast<const uint32_t*>(bunits + (size_t)wv * BSTEP_MAX);
        uwa = uw32[lane];
        if (lane + 64 < BSTEP_MAX / 2) uwb = uw32[lane + 64];
    }
    auto unit_word = [&](int t) -> uint32_t {
        const int j = t >> 1;
        const uint32_t w = (j < 64) ? __builtin_amdgcn_readlane(uwa, j & 63) : __builtin_amdgcn_readlane(uwb, j & 63);
        return (t & 1) ? (w >> 16) : (w & 0xffffu);
    };
    // loader lane lq of 256 owns the elements k = 0..7 at row 16 I + 2 k + lq / 128, column 16 (I - 7) + lq mod 128
    // (consecutive lanes, consecutive columns: conflict-free window writes)
    const int lq = 64 * band_loader_slot(wv) + lane, lrow = lq >> 7, lcol = lq & 127;
    int lbk[8];
    uint32_t lok = 0;   // bit k: element k is a stored entry (kept apart from lbk: overwriting a register with a
                        // load in flight waits for the load, which put the block-index latency on the step)
    double lval[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { lbk[k] = -1; lval[k] = 0.0; }
    lds_barrier();
    CSTAMP(4);

    const BandSys SY{A, y, Lg};
    if (wv == 0) factor_block8(SY, Nl[0], NDl[0], 0, lane);
    lds_barrier();
    CSTAMP(5);
#ifdef LH_STAMPS
    unsigned long long ss_[5] = {0, 0, 0, 0, 0}, sa_ = __builtin_amdgcn_s_memtime(), sb_, bst_ = sa_;
    uint32_t su_ = 0;
#endif
    for (int t = 0; t < nstep; ++t) {
        const int k0 = 8 * t, par = t & 1, m0 = k0 + 8;
        const double* N = Nl[par];
        const double* ND = NDl[par];
        if (wv == BZW) {
            if (lane < 8) {   // z_t = b_t N_t, zeroed where |D| <= DBL_MIN (LDLT::_solve_impl)
                double zz = 0.0;
#pragma unroll
                for (int q = 0; q < 8; ++q) zz += y[k0 + q] * N[q * 8 + lane];
                const double d = SY.at(k0 + lane, k0 + lane);
                z[k0 + lane] = fabs(d) > 2.2250738585072014e-308 ? zz : 0.0;
            }
            NDg[64 * t + lane] = ND[lane];   // the back substitution's copy, off wave 0's chain
        }
        if (m0 < nb) {
            const int g0 = m0 >> 4;
            const uint32_t uw = unit_word(t);
#ifdef LH_STAMPS
            su_ = uw;
#endif
            if (wv == 0) {
                if (uw & LH_UNIT_VALID) {
                    diag_tile(SY, N, ND, k0, 16 * g0, lane);
                    wave_sync();
                }
                LDLT_SSTAMP(0);
                factor_block8(SY, Nl[par ^ 1], NDl[par ^ 1], m0, lane);
                LDLT_SSTAMP(1);
            } else if ((LU || !band_loader(wv)) && (uw & LH_UNIT_VALID)) {   // LU: the loaders too (steps of 12-15 units)
                const int I = g0 + (uw & 7), jb0 = g0 + ((uw >> 3) & 7), jb1 = g0 + ((uw >> 6) & 15);
                ldlt_tile_row(SY, N, ND, k0, 16 * I, 16 * jb0, 16 * jb1, -1, (uw & LH_UNIT_STORE) != 0, lane);
            }
            if (wv != 0) LDLT_SSTAMP(3);
        }
        if (band_loader(wv)) {
            // tile row I enters the window at step 2 I - 14, into the slots of tile row I - 8 (retired
            // after step 2 I - 15).  From the band image (prm.bimg, one rank) its values are loaded at step
            // 2 I - 16, in pairs; from the packed blocks (sharded solves) its block indices at 2 I - 16 and its
            // values at 2 I - 15
            // Every load is unconditional (clamped index): a conditional load becomes a branch whose join
            // waits for it.  Selections and the diagonal's lambda wait until the values are written.
            if ((t & 1) == 0) {
                const int Iw = t / 2 + 7;
                if (Iw >= 8 && Iw < NT) {
#ifdef LH_STAMPS
                    // (diagnostic) loader wave 12: the wait for its value loads, then the window writes
                    unsigned long long lt0_ = __builtin_amdgcn_s_memtime();
                    __builtin_amdgcn_s_waitcnt(0);
                    __builtin_amdgcn_sched_barrier(0);
                    unsigned long long lt1_ = __builtin_amdgcn_s_memtime();
                    if (wv == 12 && lane == 0) atomicAdd(&lh_stamps[56], lt1_ - lt0_);
#endif
                    if (bim) {
                        // pairs: lane lq holds columns 2 (lq mod 64) + {0, 1} of rows 16 Iw + 4 k + lq / 64 (lval[2k],
                        // lval[2k + 1]): one 16-byte store each, consecutive lanes on consecutive pairs
                        const int c = 16 * (Iw - 7) + 2 * (lq & 63);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int r = 16 * Iw + 4 * k + (lq >> 6);
                            double v0 = lval[2 * k], v1 = lval[2 * k + 1];
                            if (r == c) v0 = (r >= n) ? 1.0 : ((prm.strategy == 0) ? v0 + lambda : v0 + lambda * v0);
                            if (r == c + 1) v1 = (r >= n) ? 1.0 : ((prm.strategy == 0) ? v1 + lambda : v1 + lambda * v1);
                            *reinterpret_cast<double2*>(&SY.at(r, c)) = double2{(c <= r) ? v0 : 0.0, (c + 1 <= r) ? v1 : 0.0};
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            const int r = 16 * Iw + 2 * k + lrow, c = 16 * (Iw - 7) + lcol;
                            double v = ((lok >> k) & 1) ? lval[k] : 0.0;
                            if (r == c) v = (r >= n) ? 1.0 : ((prm.strategy == 0) ? v + lambda : v + lambda * v);
                            SY.at(r, c) = (c <= r) ? v : 0.0;
                        }
                    }
#ifdef LH_STAMPS
                    __builtin_amdgcn_s_waitcnt(0);
                    __builtin_amdgcn_sched_barrier(0);
                    if (wv == 12 && lane == 0) {
                        atomicAdd(&lh_stamps[57], __builtin_amdgcn_s_memtime() - lt1_);
                        atomicAdd(&lh_stamps[58], 1ull);
                    }
#endif
                }
                const int Ia = t / 2 + 8;
                if (bim && Ia < NT) {
                    // tile row Ia's values from the band image, two steps before they are written: the pair at
                    // row 16 Ia + 4 k + lq / 64, columns 16 (Ia - 7) + 2 (lq mod 64) + {0, 1} is double2 256 k + lq
                    const double2* __restrict__ bt = reinterpret_cast<const double2*>(bsrc + (size_t)Ia * LH_BIMG_TR) + lq;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const double2 v = bt[256 * k];
                        lval[2 * k] = v.x;
                        lval[2 * k + 1] = v.y;
                    }
                } else if (Ia < NT) {
                    const int c = 16 * (Ia - 7) + lcol, pc = c / 6;
                    lok = 0;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int r = 16 * Ia + 2 * k + lrow, pr = r / 6, d = pr - pc;
                        lbk[k] = bblk[min(max(pc, 0), P - 1) * 64 + min(max(d, 0), 63)];
                        lok |= (c <= r && r < n && d < 64) ? (1u << k) : 0u;
                    }
                }
            } else if (!bim) {
                const int Ib = (t - 1) / 2 + 8;
                if (Ib < NT) {
                    const int c = 16 * (Ib - 7) + lcol;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int r = 16 * Ib + 2 * k + lrow;
                        lval[k] = src[(size_t)max(lbk[k], 0) * 36 + (c % 6) * 6 + (r % 6)];
                        if (lbk[k] < 0) lok &= ~(1u << k);   // a pair no chunk couples
                    }
                }
            }
        }
#ifdef LH_STAMPS
        // (diagnostic) each wave's arrival at the step barrier, from its own exit of the previous one
        if (lane == 0) atomicAdd(&lh_stamps[128 + 16 * (t & 1) + wv], __builtin_amdgcn_s_memtime() - bst_);
#endif
        lds_barrier();
#ifdef LH_STAMPS
        bst_ = __builtin_amdgcn_s_memtime();
#endif
        if (wv == 0) LDLT_SSTAMP(2); else LDLT_SSTAMP(4);
    }
#ifdef LH_STAMPS
    if (lane == 0) {
        if (wv == 0) {
            atomicAdd(&lh_stamps[46], ss_[0]);
            atomicAdd(&lh_stamps[47], ss_[1]);
            atomicAdd(&lh_stamps[48], ss_[2]);
            atomicAdd(&lh_stamps[51], 1ull);
        } else {
            atomicAdd(&lh_stamps[49], ss_[3]);
            atomicAdd(&lh_stamps[50], ss_[4]);
        }
    }
#endif
    __syncthreads();   // L and ND rows in global memory, z in LDS
    CSTAMP(6);

    // ---------------- back substitution x = L^-T z, blocks descending, one wave ----------------
    // The rows a block updates (L[KB+v][r] != 0 needs r >= KB + v - 104) live in registers: lane l,
    // slot s holds the row r = l + 64 s (mod 128) of the window [KB - 120, KB + 8), so the block's own 8
    // rows sit in 8 consecutive lanes of one 16-lane row (DPP broadcasts, as k_ctrl's backsub_block),
    // and once solved their lanes take the rows 128 below, which enter the window for the next block.
    // Per block: x_b = ND_b y_b, then every other held row takes y_r -= sum_v L[KB+v][r] x_b[v]; the
    // next block's L rows and ND are loaded while this one computes.
    // The L rows and ND come from global memory through an LDS ring the other 15 waves fill ahead of
    // wave 0 (the window's LDS is free now): block j of the descent (KB = nb - 8 - 8 j) goes to slot
    // j mod BRING, loaded by wave 1 + j mod 15 once wave 0 has read block j - BRING, and published by
    // a workgroup-scope release of bring_ready[slot] = j + 1.  Wave 0 reads each block's L from LDS one
    // block ahead (its ND when it starts the block).
    constexpr int BSLOT = 8 * LH_LBW + 64;   // one block: its 8 L rows as stored, then its ND
    constexpr int BRING = (128 * AS) / BSLOT;
    static_assert(BRING >= 15, "ring deeper than the producer count");
    __shared__ int bring_ready[BRING], bring_used;
    const int nblk = nb / 8;
    if (tid < BRING) bring_ready[tid] = 0;
    if (tid == 0) bring_used = 0;
    lds_barrier();
    if (wv > 0) {   // producers
        for (int j = wv - 1; j < nblk; j += 15) {
            if (j >= BRING)
                while (__hip_atomic_load(&bring_used, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < j - BRING + 1)
                    __builtin_amdgcn_s_sleep(1);
            const int KB = nb - 8 - 8 * j;
            const double2* gl = reinterpret_cast<const double2*>(Lg + (size_t)KB * LH_LBW);
            const double2* gn = reinterpret_cast<const double2*>(NDg + (size_t)8 * KB);
            double2 v[8], vn = double2{0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = gl[k * 64 + lane];
            if (lane < 32) vn = gn[lane];
            double2* dst = reinterpret_cast<double2*>(A + (j % BRING) * BSLOT);
#pragma unroll
            for (int k = 0; k < 8; ++k) dst[k * 64 + lane] = v[k];
            if (lane < 32) dst[8 * 64 + lane] = vn;
            __hip_atomic_store(&bring_ready[j % BRING], j + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    } else {
      // NW (band_narrow: every row's envelope within 56 rows of its block): one held row per lane, the
      // window [KB - 56, KB + 8); else two, the window [KB - 120, KB + 8)
      auto consumer = [&](auto nw_tag) {
        constexpr bool NW = decltype(nw_tag)::value;
        constexpr int WROWS = NW ? 64 : 128;
        auto row_of = [&](int KB, int sl) {
            const int lo = KB + 8 - WROWS;
            return lo + ((lane + 64 * sl - lo) & (WROWS - 1));
        };
        // every block in [j0, j1] published (one round trip for the batch; producers run far ahead)
        auto wait_ready = [&](int j0, int j1) {
            for (;;) {
                int miss = 0;   // every flag read in one round trip (no short circuit)
                for (int j = j0; j <= j1; ++j)
                    miss |= __hip_atomic_load(&bring_ready[j % BRING], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != j + 1;
                if (!miss) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");   // orders the slot reads after
                    return;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        };
        // block j's L entries of this lane's two rows from its slot (clamped: the own block's rows and rows
        // past the band read in-bounds values never used)
        // (a held row is >= KB - 120 >= KB + v - LH_LBW, inside every stored L row: one clamp, and the 8 reads
        // of a row share one address, v (LH_LBW - 1) doubles apart as immediate offsets)
        auto load_blk = [&](int j, double (&l0)[8], double (&l1)[8]) {
            const int KB = nb - 8 - 8 * j;
            const double* sl = A + (j % BRING) * BSLOT + LH_LBW - KB;   // + v (LH_LBW - 1) + r: L[KB+v][r]
            const double* p0 = sl + min(row_of(KB, 0), KB - 1);
            const double* p1 = sl + min(row_of(KB, 1), KB - 1);
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                l0[v] = p0[v * (LH_LBW - 1)];
                l1[v] = NW ? 0.0 : p1[v * (LH_LBW - 1)];
            }
        };
        double y0, y1;
        {
            const int r0 = row_of(nb - 8, 0), r1 = row_of(nb - 8, 1);
            y0 = (r0 >= 0) ? z[r0] : 0.0;
            y1 = (!NW && r1 >= 0) ? z[r1] : 0.0;
        }
        // block j with its L entries ca / cb: x_b = ND_b y_b, then the held rows' updates
#ifdef LH_STAMPS
        unsigned long long bs_[3] = {0, 0, 0}, ba_ = 0, bb_ = 0;
#define BSUB_STAMP(i) do { __builtin_amdgcn_sched_barrier(0); bb_ = __builtin_amdgcn_s_memtime(); \
        if ((i) >= 0) bs_[(i) < 0 ? 0 : (i)] += bb_ - ba_; ba_ = bb_; __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define BSUB_STAMP(i)
#endif
        // block j's ND row (lane & 7) from its slot
        auto load_nd = [&](int j, double (&cn)[8]) {
            const double* p = A + (j % BRING) * BSLOT + 8 * LH_LBW + (lane & 7) * 8;
#pragma unroll
            for (int v = 0; v < 8; ++v) cn[v] = p[v];
        };
        double cn[8];   // block j's ND row on entry; block j + 1's, loaded once x_b is formed, on exit
        auto solve_blk = [&](int j, const double (&ca)[8], const double (&cb)[8]) {
            BSUB_STAMP(-1);
            const int KB = nb - 8 - 8 * j;
            const int sb_ = NW ? 0 : (KB >> 6) & 1, kl = KB & 63;
            const bool mine = lane >= kl && lane < kl + 8;
            const int re = KB - WROWS + (lane - kl);                     // the row entering this lane's slot
            const double zin = z[max(re, 0)];
            const double ys = sb_ ? y1 : y0;
            double yb[8];
            if (KB & 8) {
                yb[0] = bcast16<8>(ys); yb[1] = bcast16<9>(ys); yb[2] = bcast16<10>(ys); yb[3] = bcast16<11>(ys);
                yb[4] = bcast16<12>(ys); yb[5] = bcast16<13>(ys); yb[6] = bcast16<14>(ys); yb[7] = bcast16<15>(ys);
            } else {
                yb[0] = bcast16<0>(ys); yb[1] = bcast16<1>(ys); yb[2] = bcast16<2>(ys); yb[3] = bcast16<3>(ys);
                yb[4] = bcast16<4>(ys); yb[5] = bcast16<5>(ys); yb[6] = bcast16<6>(ys); yb[7] = bcast16<7>(ys);
            }
            const double xv = ((cn[0] * yb[0] + cn[1] * yb[1]) + (cn[2] * yb[2] + cn[3] * yb[3])) +
                              ((cn[4] * yb[4] + cn[5] * yb[5]) + (cn[6] * yb[6] + cn[7] * yb[7]));
            load_nd(min(j + 1, nblk - 1), cn);   // published: j + 1 < j + 4, checked an iteration before
#ifdef LH_STAMPS
            double xvs = xv;
            asm volatile("" : "+v"(xvs));
#endif
            BSUB_STAMP(0);
            double xb[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) xb[v] = readlane_d(xv, kl + v);
            const double sa = ((ca[0] * xb[0] + ca[1] * xb[1]) + (ca[2] * xb[2] + ca[3] * xb[3])) +
                              ((ca[4] * xb[4] + ca[5] * xb[5]) + (ca[6] * xb[6] + ca[7] * xb[7]));
            // rows past the band have zero L; the block's own rows (r >= KB) take no update
            if (row_of(KB, 0) < KB) y0 -= sa;
            if constexpr (!NW) {
                const double sbb = ((cb[0] * xb[0] + cb[1] * xb[1]) + (cb[2] * xb[2] + cb[3] * xb[3])) +
                                   ((cb[4] * xb[4] + cb[5] * xb[5]) + (cb[6] * xb[6] + cb[7] * xb[7]));
                if (row_of(KB, 1) < KB) y1 -= sbb;
            }
            if (mine) {
                y[KB + (lane - kl)] = xv;                                // the solution, natural order
                const double zi = re >= 0 ? zin : 0.0;
                if (sb_) y1 = zi; else y0 = zi;
            }
#ifdef LH_STAMPS
            asm volatile("" : "+v"(y0), "+v"(y1));
#endif
            BSUB_STAMP(1);
        };
        // two register sets in turn (no copies between blocks); every 4 blocks one batched readiness check
        // for the next 4 and one release of the slots read so far (the release waits for this wave's
        // outstanding LDS reads, so no producer rewrites a slot still being read)
        double la[8], lb[8], ma[8], mb[8];
        wait_ready(0, min(3, nblk - 1));
        load_blk(0, la, lb);
        load_nd(0, cn);
        for (int j = 0; j < nblk; j += 2) {
            // the flags of blocks j + 4 .. j + 7 (first loaded at iteration j + 2) are read now and checked
            // after block j, so the read's round trip overlaps the block instead of preceding it
            const bool chk = (j & 3) == 0 && j + 4 < nblk;
            int miss = 0;
            if (chk)
                for (int q = j + 4; q <= min(j + 7, nblk - 1); ++q)
                    miss |= __hip_atomic_load(&bring_ready[q % BRING], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != q + 1;
            load_blk(min(j + 1, nblk - 1), ma, mb);
            solve_blk(j, la, lb);
            BSUB_STAMP(-1);
            if (chk) {
                if (miss) wait_ready(j + 4, min(j + 7, nblk - 1));
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            }
            BSUB_STAMP(2);
            if (j + 1 >= nblk) break;
            load_blk(min(j + 2, nblk - 1), la, lb);
            solve_blk(j + 1, ma, mb);
            if ((j & 3) == 2 && lane == 0)
                __hip_atomic_store(&bring_used, j + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
#ifdef LH_STAMPS
        if (lane == 0) {
            atomicAdd(&lh_stamps[52], bs_[0]);
            atomicAdd(&lh_stamps[53], bs_[1]);
            atomicAdd(&lh_stamps[54], bs_[2]);
            atomicAdd(&lh_stamps[55], (unsigned long long)nblk);
        }
#endif
#undef BSUB_STAMP
      };
      if (prm.band_narrow) consumer(BoolTag<true>{});
      else consumer(BoolTag<false>{});
    }
    __syncthreads();
    CSTAMP(8);
    ctrl_step_tail<CT>(ctrl, prm, n, lambda, y, src + LY.off_bp, src + LY.off_hd, s_red, dxp, rung);
    CSTAMP(12);
    CSTAMP_END();
}
