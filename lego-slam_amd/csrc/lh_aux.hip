// lh_aux.hip — the small kernels around a solve: k_gather, the outlier pass, the peer-write exchange, k_nop;
// and the stamps' reader.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>

#include "lh_launch.h"
#include "lh_dev.h"

#pragma clang fp contract(fast)

extern "C" {

// ---- k_gather: results back into window order for the download: landmark positions from the
//      committed records (into out_xyz, pre-filled with the input positions, so landmarks without an
//      edge keep theirs), per-edge rho0 "as last evaluated" from the slots ----
__global__ __launch_bounds__(256) void k_gather(const lh_ctrl* __restrict__ ctrl, const double* __restrict__ rec,
                                                const int32_t* __restrict__ lm_perm, int nrec,
                                                const double* __restrict__ rho, const int32_t* __restrict__ obs_perm,
                                                long nslots, double* __restrict__ out_xyz, double* __restrict__ out_rho) {
    const int cur = __builtin_amdgcn_readfirstlane(ctrl->cur);
    const double* rc = rec + (size_t)cur * nrec * LH_REC;
    const long i0 = (long)blockIdx.x * 256 + threadIdx.x, st = (long)gridDim.x * 256;
    for (long i = i0; i < nslots; i += st) {
        const int o = obs_perm[i];
        if (o >= 0) out_rho[o] = rho[i];
    }
    for (long i = i0; i < 3L * nrec; i += st) {
        const int r = (int)(i / 3), a = (int)(i - 3L * r);
        const int l = lm_perm[r];
        if (l >= 0) out_xyz[3 * (size_t)l + a] = rc[(size_t)r * LH_REC + LH_REC_X + a];
    }
}

hipError_t lh_launch_gather(hipStream_t st, const lh_ctrl* ctrl, const double* rec, const int32_t* lm_perm, int nrec,
                            const double* rho, const int32_t* obs_perm, long nslots, double* out_xyz, double* out_rho) {
    const long n = std::max(nslots, 3L * nrec);
    if (n <= 0) return hipSuccess;
    const int blocks = (int)std::max(1L, std::min(4096L, (n + 255) / 256));
    hipLaunchKernelGGL(k_gather, dim3(blocks), dim3(256), 0, st, ctrl, rec, lm_perm, nrec, rho, obs_perm, nslots,
                       out_xyz, out_rho);
    return hipGetLastError();
}

// ---- Backend::Optimize's outlier pass (backend_lego.cpp:163-194) on the device, over rho0 as last
//      evaluated (d_rho, slot order).  The loop counts edges with rho0 > th for th = th0 2^k, k < 5 (the
//      thresholds it can visit: doubling is exact), so one pass counts all five, as per-block partials
//      (integers: the same totals in any order, and no counter to zero first); the second pass sums the
//      partials, replays the loop on the totals and writes one flag per edge in window order, with the
//      threshold and the counts behind the flags, so one copy brings all of it back. ----
#define LH_OCB 256   // blocks of the counting pass
__global__ __launch_bounds__(256) void k_outlier_count(const double* __restrict__ rho, const int32_t* __restrict__ obs_perm,
                                                       long nslots, double th0, unsigned* __restrict__ part) {
    __shared__ unsigned wsum[4][5];
    unsigned c[5] = {0u, 0u, 0u, 0u, 0u};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nslots; i += (long)gridDim.x * 256) {
        if (obs_perm[i] < 0) continue;   // padding slot
        const double r = rho[i];
        double th = th0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            c[k] += (r > th) ? 1u : 0u;   // a NaN rho0 counts as an inlier, as in the reference
            th *= 2;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        unsigned v = c[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) wsum[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 5)
        part[blockIdx.x * 5 + threadIdx.x] = wsum[0][threadIdx.x] + wsum[1][threadIdx.x] + wsum[2][threadIdx.x] + wsum[3][threadIdx.x];
}

// A sharded window's pass (the reference counts the whole window's edges): the counting blocks' partials summed
// into this rank's {5 counts, its edge count} as doubles (exact below 2^53), which the handle's exchange sums
// over the ranks before k_outlier_flags reads them (gtot)
__global__ __launch_bounds__(64) void k_outlier_total(const unsigned* __restrict__ part, int nparts, long n_obs,
                                                      double* __restrict__ tot) {
    long c[5] = {0, 0, 0, 0, 0};
    for (int b = threadIdx.x; b < nparts; b += 64)
#pragma unroll
        for (int k = 0; k < 5; ++k) c[k] += part[b * 5 + k];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        long v = c[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (threadIdx.x == 0) tot[k] = (double)v;
    }
    if (threadIdx.x == 0) tot[5] = (double)n_obs;
}

__global__ __launch_bounds__(256) void k_outlier_flags(const double* __restrict__ rho, const int32_t* __restrict__ obs_perm,
                                                       long nslots, long n_obs, double th0, const unsigned* __restrict__ part,
                                                       int nparts, uint8_t* __restrict__ flags, double* __restrict__ res,
                                                       const double* __restrict__ gtot) {
    __shared__ long tot[5];
    if (gtot) {   // the all-ranks totals (k_outlier_total + the exchange)
        if (threadIdx.x < 5) tot[threadIdx.x] = (long)gtot[threadIdx.x];
        n_obs = (long)gtot[5];
    } else if (threadIdx.x < 64) {
        long c[5] = {0, 0, 0, 0, 0};
        for (int b = threadIdx.x; b < nparts; b += 64)
#pragma unroll
            for (int k = 0; k < 5; ++k) c[k] += part[b * 5 + k];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            long v = c[k];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if (threadIdx.x == 0) tot[k] = v;
        }
    }
    __syncthreads();
    // backend_lego.cpp:164-184, on the totals (every thread the same)
    double th = th0;
    long cin = 0, cout = 0;
    for (int it = 0; it < 5; ++it) {
        cout = tot[it];
        cin = n_obs - cout;
        const double ratio = cin / double(cin + cout);
        if (ratio > 0.5) break;
        th *= 2;
    }
    const long i0 = (long)blockIdx.x * 256 + threadIdx.x, st = (long)gridDim.x * 256;
    for (long i = i0; i < nslots; i += st) {   // :186-194
        const int o = obs_perm[i];
        if (o >= 0) flags[o] = rho[i] > th ? 1 : 0;
    }
    if (i0 == 0) {
        res[0] = th;
        res[1] = (double)cin;
        res[2] = (double)cout;
    }
}

// ---- the one-shot peer-write exchange (LH_COMM_P2P, lh_common.h) ----
// Block d writes this rank's partial (the packed reduced system, and max|diag H_ll| at the initial linearisation)
// into slot `rank` of rank d's buffer, then its arrival tag.  The buffers are plain device memory mapped over IPC,
// whose caches are not coherent with another agent's: the data goes out as system-scope stores and is read back as
// system-scope loads (no stale line in either GPU's L2), every thread's stores are fenced at system scope before
// the block's barrier, and thread 0 stores the tag with a system-scope release.
__global__ __launch_bounds__(1024) void k_p2p_push(const double* __restrict__ src, const double* __restrict__ maxd,
                                                   int n, lh_peers peers, int rank, int world, int parity,
                                                   unsigned long long tag, long slot) {
    const int d = blockIdx.x;
    double* dst = peers.p[d] + ((size_t)parity * world + rank) * slot;
    for (int i = threadIdx.x; i < n; i += 1024) __hip_atomic_store(dst + i, src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (threadIdx.x == 0) __hip_atomic_store(dst + n, maxd ? *maxd : 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long* tags = reinterpret_cast<unsigned long long*>(peers.p[d] + (size_t)2 * world * slot);
        __hip_atomic_store(tags + parity * world + rank, tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Every block waits for the trial's tags of all ranks in this rank's buffer (system-scope acquire; a bounded
// wait: past ~4 s the exchange is declared failed in *err, a host-mapped word, and the block exits), then sums
// its elements over the slots in rank order into the reduced system (max for max|diag H_ll|): every rank gets the
// same bits.
__global__ __launch_bounds__(256) void k_p2p_sum(double* __restrict__ dst, double* __restrict__ maxd, int n,
                                                 const double* __restrict__ buf, int world, int parity,
                                                 unsigned long long tag, long slot, int mode, volatile int* err) {
    __shared__ int s_ok;
    if (threadIdx.x == 0) {
        const unsigned long long* tags = reinterpret_cast<const unsigned long long*>(buf + (size_t)2 * world * slot) +
                                         parity * world;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
        int ok = *err ? 0 : 1;   // (an earlier exchange of this handle failed: no second wait)
        for (int r = 0; r < world && ok; ++r)
            while (__hip_atomic_load(tags + r, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != tag) {
                if (__builtin_amdgcn_s_memrealtime() - t0 > 400000000ull) { ok = 0; *err = 1; break; }
                __builtin_amdgcn_s_sleep(2);
            }
        s_ok = ok;
    }
    __syncthreads();
    if (!s_ok) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const double* src = buf + (size_t)parity * world * slot;
    auto ld = [](const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); };
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        double v = ld(src + i);
        for (int r = 1; r < world; ++r) v += ld(src + (size_t)r * slot + i);
        dst[i] = v;
    }
    if (mode == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
        double m = ld(src + n);
        for (int r = 1; r < world; ++r) m = fmax(m, ld(src + (size_t)r * slot + n));
        *maxd = m;
    }
}

hipError_t lh_launch_p2p(hipStream_t st, double* rs, double* maxd, int n, lh_peers peers, int rank, int world,
                         int parity, unsigned long long tag, long slot, int mode, int* err) {
    if (world < 1 || world > LH_P2P_MAX || (long)n + 1 > slot) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_p2p_push, dim3(world), dim3(1024), 0, st, (const double*)rs, mode == 0 ? (const double*)maxd : nullptr,
                       n, peers, rank, world, parity, tag, slot);
    const int nb = std::max(1, std::min(32, (n + 255) / 256));
    hipLaunchKernelGGL(k_p2p_sum, dim3(nb), dim3(256), 0, st, rs, maxd, n, (const double*)peers.p[rank], world, parity,
                       tag, slot, mode, (volatile int*)err);
    return hipGetLastError();
}

// part: LH_OCB * 5 counters; flags: n_obs bytes, then (16-byte aligned) the threshold and the two counts
hipError_t lh_launch_outliers(hipStream_t st, const double* rho, const int32_t* obs_perm, long nslots, long n_obs,
                              double th0, unsigned* part, uint8_t* flags) {
    if (nslots <= 0) return hipSuccess;
    const int nb_c = (int)std::max(1L, std::min((long)LH_OCB, (nslots + 255) / 256));
    const int nb_f = (int)std::max(1L, std::min(2048L, (nslots + 255) / 256));
    double* res = reinterpret_cast<double*>(flags + ((n_obs + 15) & ~15L));
    hipLaunchKernelGGL(k_outlier_count, dim3(nb_c), dim3(256), 0, st, rho, obs_perm, nslots, th0, part);
    hipLaunchKernelGGL(k_outlier_flags, dim3(nb_f), dim3(256), 0, st, rho, obs_perm, nslots, n_obs, th0,
                       (const unsigned*)part, nb_c, flags, res, (const double*)nullptr);
    return hipGetLastError();
}

// the sharded pass in two halves around the exchange of tot[6] (this rank's counts and edge count)
hipError_t lh_launch_outlier_counts(hipStream_t st, const double* rho, const int32_t* obs_perm, long nslots, long n_obs,
                                    double th0, unsigned* part, double* tot) {
    const int nb_c = (int)std::max(1L, std::min((long)LH_OCB, (nslots + 255) / 256));
    if (nslots > 0) hipLaunchKernelGGL(k_outlier_count, dim3(nb_c), dim3(256), 0, st, rho, obs_perm, nslots, th0, part);
    hipLaunchKernelGGL(k_outlier_total, dim3(1), dim3(64), 0, st, (const unsigned*)part, nslots > 0 ? nb_c : 0, n_obs, tot);
    return hipGetLastError();
}

hipError_t lh_launch_outlier_flags(hipStream_t st, const double* rho, const int32_t* obs_perm, long nslots, long n_obs,
                                   double th0, const double* gtot, uint8_t* flags) {
    const int nb_f = (int)std::max(1L, std::min(2048L, (nslots + 255) / 256));
    double* res = reinterpret_cast<double*>(flags + ((n_obs + 15) & ~15L));
    hipLaunchKernelGGL(k_outlier_flags, dim3(nb_f), dim3(256), 0, st, rho, obs_perm, nslots, n_obs, th0,
                       (const unsigned*)nullptr, 0, flags, res, gtot);
    return hipGetLastError();
}

// ---- empty kernel: the HIP-event bracket floor of one launch (bench.py's roofline timing) ----
__global__ void k_nop() {}

hipError_t lh_launch_nop(hipStream_t st) {
    hipLaunchKernelGGL(k_nop, dim3(1), dim3(64), 0, st);
    return hipGetLastError();
}

hipError_t lh_read_stamps(unsigned long long* out, int n, int reset) {
#ifdef LH_STAMPS
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(lh_stamps), sizeof(unsigned long long) * (n < 256 ? n : 256));
    if (e != hipSuccess) return e;
    if (reset) {
        unsigned long long z[256] = {0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(lh_stamps), z, sizeof(z));
    }
    return e;
#else
    for (int i = 0; i < n; ++i) out[i] = 0;
    (void)reset;
    return hipSuccess;
#endif
}

// k_lin's per-wave records of the -DLH_STAMPS build (lh_dev.h lh_lin_stamps; zeros otherwise), cleared after the read
hipError_t lh_read_lin_stamps(unsigned long long* out, int n) {
#ifdef LH_STAMPS
    static unsigned long long z[LH_LSTAMP_N];
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(lh_lin_stamps),
                                       sizeof(unsigned long long) * (n < LH_LSTAMP_N ? n : LH_LSTAMP_N));
    if (e != hipSuccess) return e;
    for (int i = LH_LSTAMP_N; i < n; ++i) out[i] = 0;
    return hipMemcpyToSymbol(HIP_SYMBOL(lh_lin_stamps), z, sizeof(z));
#else
    for (int i = 0; i < n; ++i) out[i] = 0;
    return hipSuccess;
#endif
}

}  // extern "C"
