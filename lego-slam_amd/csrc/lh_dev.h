// lh_dev.h — device helpers shared by every kernel file of the sliding-window BA solver (gfx950).
// (lh_lin.hip, lh_kernels.hip with its headers lh_lm.h and lh_ldlt.h, lh_frames.hip, lh_aux.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(fast)

typedef double v4d __attribute__((ext_vector_type(4)));

// Diagnostic build (-DLH_STAMPS): per-phase wave-cycle totals via s_memtime,
// summed over all waves into lh_stamps[] (cdna_hip_programming.md §7 "In-kernel
// stamps").  The product build compiles these to nothing.
#ifdef LH_STAMPS
// One array for all kernels, so the diagnostic library is one translation unit, lh_stamps_unit.hip: a second unit
// under LH_STAMPS (an A/B build with it, say) would add into an array of its own that lh_read_stamps never reads.
#ifndef LH_STAMPS_UNIT
#error "LH_STAMPS is for lh_stamps_unit.hip alone: the stamped kernels must share one lh_stamps array"
#endif
__device__ unsigned long long lh_stamps[256];   // [64, 128): k_ctrl's LDL^T steps, per step (lds_ldlt_solve);
                                                // [128, 160): k_ctrl_b's barrier arrival per wave, even / odd steps
#define STAMP_DECL unsigned long long st0_ = __builtin_amdgcn_s_memtime(), st1_, sacc_[24] = {0};
#define STAMP(i)                                                                   \
    do {                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                         \
        st1_ = __builtin_amdgcn_s_memtime();                                       \
        sacc_[(i) % 24] += st1_ - st0_;                                            \
        st0_ = st1_;                                                               \
        __builtin_amdgcn_sched_barrier(0);                                         \
    } while (0)
#define STAMP_FLUSH(base, cnt)                                                     \
    do {                                                                           \
        if ((threadIdx.x & 63) == 0)                                               \
            for (int i_ = 0; i_ < (cnt); ++i_)                                     \
                if (sacc_[((base) + i_) % 24]) atomicAdd(&lh_stamps[(base) + i_], sacc_[((base) + i_) % 24]); \
    } while (0)
// k_lin's waves, one record of LH_LSTAMP_REC words per (workgroup, wave) of the last full trial launch: [0] the
// wave's HW_ID word | its XCC_ID << 32 | 1 << 40, [1] s_memtime when it enters the sub-batch loop, [2 + r] s_memtime
// at the end of its r-th sub-batch (r < 6).  Which waves share a SIMD, and which of them run the extra sub-batch
// beside another such wave or alone (scripts/lin_wave_stamps.py).
#define LH_LSTAMP_REC 8
#define LH_LSTAMP_N 16384
__device__ unsigned long long lh_lin_stamps[LH_LSTAMP_N];
#define LSTAMP_DECL(on, blk, nw, wave)                                                              \
    unsigned long long* lst_ = nullptr;                                                             \
    int lround_ = 0;                                                                                \
    if ((on) && ((blk) * (nw) + (wave) + 1) * LH_LSTAMP_REC <= LH_LSTAMP_N && (threadIdx.x & 63) == 0) { \
        lst_ = lh_lin_stamps + ((blk) * (nw) + (wave)) * LH_LSTAMP_REC;                             \
        for (int i_ = 2; i_ < LH_LSTAMP_REC; ++i_) lst_[i_] = 0ull;                                 \
        lst_[0] = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4) |                             \
                  ((unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32) | (1ull << 40); \
        lst_[1] = __builtin_amdgcn_s_memtime();                                                     \
    }
#define LSTAMP_ROUND()                                                                              \
    do {                                                                                            \
        if (lst_ && lround_ < LH_LSTAMP_REC - 2) lst_[2 + lround_] = __builtin_amdgcn_s_memtime();  \
        ++lround_;                                                                                  \
    } while (0)
// k_ctrl wall-clock stamps: thread 0 (wave 0, the critical chain) adds s_memtime at each
// barrier-aligned phase boundary of every live launch into lh_stamps[32 + i]; consecutive sums
// difference to per-phase latency.  [61] live launches, [62]/[63] s_memrealtime at start / end.
#define CSTAMP(i)                                                                  \
    do {                                                                           \
        if (threadIdx.x == 0) {                                                    \
            __builtin_amdgcn_sched_barrier(0);                                     \
            atomicAdd(&lh_stamps[32 + (i)], (unsigned long long)__builtin_amdgcn_s_memtime()); \
            __builtin_amdgcn_sched_barrier(0);                                     \
        }                                                                          \
    } while (0)
// a controller's launch: its start times taken at the top, added with the live-launch count once the launch is
// known to be live (after the decision's exits), and the end time
#define CSTAMP_START \
    const unsigned long long ct_start = __builtin_amdgcn_s_memtime(), rt_start = __builtin_amdgcn_s_memrealtime()
#define CSTAMP_LIVE()                                                              \
    do {                                                                           \
        if (threadIdx.x == 0) {                                                    \
            atomicAdd(&lh_stamps[32], ct_start);                                   \
            atomicAdd(&lh_stamps[61], 1ull);                                       \
            atomicAdd(&lh_stamps[62], rt_start);                                   \
        }                                                                          \
    } while (0)
#define CSTAMP_END()                                                               \
    do {                                                                           \
        if (threadIdx.x == 0) atomicAdd(&lh_stamps[63], (unsigned long long)__builtin_amdgcn_s_memrealtime()); \
    } while (0)
#else
#define STAMP_DECL
#define STAMP(i)
#define STAMP_FLUSH(base, cnt)
#define LSTAMP_DECL(on, blk, nw, wave)
#define LSTAMP_ROUND()
#define CSTAMP(i)
#define CSTAMP_START
#define CSTAMP_LIVE()
#define CSTAMP_END()
#endif

__device__ __forceinline__ double readlane_d(double v, int l) {
    const long long x = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)x, l);
    const int hi = __builtin_amdgcn_readlane((int)(x >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Workgroup barrier ordering LDS only.  __syncthreads() also releases global memory, i.e. waits
// (s_waitcnt vmcnt(0)) for every global store and prefetch load the wave has in flight; these
// kernels never hand global data between threads of a workgroup, so that wait is pure stall
// (measured: ~15k cycles per wave at the end of k_lin).
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// 1/d with one v_rcp_f64 and two Newton steps (the LDLT pivots and the H_ll Cholesky are not a bitwise-mirrored path)
__device__ __forceinline__ double fast_rcp(double d) {
    double r = __builtin_amdgcn_rcp(d);
    r = fma(r, fma(-d, r, 1.0), r);
    r = fma(r, fma(-d, r, 1.0), r);
    return r;
}

// 1/sqrt(a) with v_rsq_f64 and two Newton steps (the H_ll Cholesky is not a mirrored path)
__device__ __forceinline__ double fast_rsq(double a) {
    double y = __builtin_amdgcn_rsq(a);
    const double h = 0.5 * a;
    y = y * fma(-h * y, y, 1.5);
    y = y * fma(-h * y, y, 1.5);
    return y;
}

// butterfly sum over the aligned lane group of G = 1 << lg lanes (every lane gets the total):
// v + v[lane^1], + [lane^2], + [lane^4], ... in that order.  Partners within a 16-lane row come
// through DPP (plain VALU: quad_perm for ^1 and ^2, row rotations for ^4 and ^8); ^16 and ^32
// through the permlane swaps.
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const long long x = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(x >> 32), CTRL, 0xF, 0xF, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// v + v[lane ^ 16] and v + v[lane ^ 32] by the gfx950 half-row / half-wave swaps (plain VALU, no LDS
// round trip as ds_bpermute takes).  With both operands v, permlane16_swap returns v[lane & ~16] and
// v[lane | 16], permlane32_swap v[lane & 31] and v[32 + (lane & 31)]: their sum is v + the partner in
// every lane (IEEE addition commutes, so the bits are those of v + partner).
__device__ __forceinline__ double xor16_sum(double v) {
    const long long x = __double_as_longlong(v);
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(x >> 32), (unsigned)(x >> 32), false, false);
    return __longlong_as_double(((long long)hi[0] << 32) | lo[0]) + __longlong_as_double(((long long)hi[1] << 32) | lo[1]);
}
__device__ __forceinline__ double xor32_sum(double v) {
    const long long x = __double_as_longlong(v);
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(x >> 32), (unsigned)(x >> 32), false, false);
    return __longlong_as_double(((long long)hi[0] << 32) | lo[0]) + __longlong_as_double(((long long)hi[1] << 32) | lo[1]);
}

// N values at once: one uniform branch per level and N independent DPP + add chains per level
// (a sum at a time serialises the branches and the DPP latencies)
template <int N>
__device__ __forceinline__ void group_sum(double (&v)[N], int lg) {
    if (lg >= 1) {                                          // quad_perm [1,0,3,2]: lane ^ 1
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] += dpp_d<0xB1>(v[i]);
    }
    if (lg >= 2) {                                          // quad_perm [2,3,0,1]: lane ^ 2
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] += dpp_d<0x4E>(v[i]);
    }
    if (lg >= 3) {                                          // lane ^ 4: row_ror 12 / row_ror 4
        const bool up = (__lane_id() & 4) != 0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const double a = dpp_d<0x12C>(v[i]), b = dpp_d<0x124>(v[i]);
            v[i] += up ? b : a;
        }
    }
    if (lg >= 4) {                                          // row_ror 8: lane ^ 8
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] += dpp_d<0x128>(v[i]);
    }
    if (lg >= 5) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = xor16_sum(v[i]);
    }
    if (lg >= 6) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = xor32_sum(v[i]);
    }
}

// the whole-wave butterfly in the other order, v + v[lane ^ 32], then ^16, ^8, ^4, ^2, ^1: the bits of the
// `v += __shfl_xor(v, off)` loop over off = 32 .. 1 (k_reduce's scalar sums) in plain VALU (ds_bpermute takes LDS
// bandwidth, which a batch's 32 sums per wave exhausted)
template <int N>
__device__ __forceinline__ void wave_sum_desc(double (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = xor32_sum(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = xor16_sum(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_d<0x128>(v[i]);
    const bool up = (__lane_id() & 4) != 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double a = dpp_d<0x12C>(v[i]), b = dpp_d<0x124>(v[i]);
        v[i] += up ? b : a;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_d<0x4E>(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_d<0xB1>(v[i]);
}

// max over the wave, every lane gets it: DPP within 16-lane rows, then the permlane swaps
__device__ __forceinline__ double wave_max(double v) {
    v = fmax(v, dpp_d<0xB1>(v));                                            // ^1
    v = fmax(v, dpp_d<0x4E>(v));                                            // ^2
    {   // ^4: both rotations by every lane, then the select, as group_sum.  (A DPP in each arm of a conditional runs
        // under that arm's exec mask, and its source lane, in the other arm, is then disabled and reads as 0: the
        // step was a no-op, and max |diag H_ll| lost the landmarks whose lead lane has bit 2 set, lg <= 2.)
        const double a = dpp_d<0x12C>(v), b = dpp_d<0x124>(v);
        v = fmax(v, (__lane_id() & 4) ? b : a);
    }
    v = fmax(v, dpp_d<0x128>(v));                                           // ^8
    const long long x = __double_as_longlong(v);
    auto lo = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);
    auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(x >> 32), (unsigned)(x >> 32), false, false);
    v = fmax(__longlong_as_double(((long long)hi[0] << 32) | lo[0]), __longlong_as_double(((long long)hi[1] << 32) | lo[1]));
    const long long y = __double_as_longlong(v);
    lo = __builtin_amdgcn_permlane32_swap((unsigned)y, (unsigned)y, false, false);
    hi = __builtin_amdgcn_permlane32_swap((unsigned)(y >> 32), (unsigned)(y >> 32), false, false);
    return fmax(__longlong_as_double(((long long)hi[0] << 32) | lo[0]), __longlong_as_double(((long long)hi[1] << 32) | lo[1]));
}

// k_lin's outputs (pair rows, per-edge rho0, landmark records) are read by later kernels only.  Stored
// plain, they sit dirty in the XCD's L2 and the kernel's end-of-launch release writes them back
// (~B / 6 TB/s at the boundary, MI355X_MICROARCH.md "boundary").  Write-through (sc1) stores leave no
// dirty line behind: k_lin 37.4 -> 36.2 us per trial launch.  LH_WT / LH_WT_REC = 0
// restore plain stores (A/B builds).
#ifndef LH_WT
#define LH_WT 1
#endif
#ifndef LH_WT_REC
#define LH_WT_REC 1
#endif

__device__ __forceinline__ void st_out(double* p, double v) {
    if constexpr (LH_WT) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}
// k_reduce's outputs (the reduced system, its LDS images) likewise, read by the controller that follows
#ifndef LH_WT_RED
#define LH_WT_RED 1   // k_reduce 6.86 / 6.86 -> 6.71 / 6.66 us, k_ctrl +0.06 (same-box A/B, profiles/r05s_ab_wt_reduce.txt)
#endif
__device__ __forceinline__ void st_red(double* p, double v) {
    if constexpr (LH_WT_RED) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}
