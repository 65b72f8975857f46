// shud_reduce.h — internal, device: the one deterministic two-level reduction of the project.  The integrator's
// vector kernels (shud_ode_kernels.hip) and the water-balance diagnostics (shud_wb.hip) both sum through it, so the
// summation order is stated here and nowhere else.
//
// Order.  One entry per thread on a one-shot grid of B = ceil(n / kRedThreads) blocks of kRedThreads threads; a
// lane past n holds the identity (0.0 for a sum, +inf for a min).
//   block_partial: each 64-lane wave combines by an xor butterfly over offsets 32 .. 1 (own value first), lane 0
//     keeps the result; wave 0 combines the block's kRedThreads/64 wave results by waves_tree (an xor butterfly over
//     offsets 8 .. 1); lane 0 stores partial[b].
//   ordered_total (the finalize, one block of kFinThreads threads): thread t keeps kFinAcc accumulators from the
//     identity, acc[k] over partials t + (kFinAcc*j + k)*kFinThreads for j = 0, 1, ... (the kFinAcc loads of one j in
//     flight together; the identity past B; any B, there is no single-pass limit); x = (acc0 + acc1) + (acc2 + acc3);
//     wave butterfly; the kFinThreads/64 wave results by waves_tree.
// No fp64 atomics: the result does not depend on scheduling.
//
// Pins.  tests/ode_kernels_py.py (device_order_sum / device_order_min) and oracle/shud_oracle_ode.c
// (device_order_sum) restate this order independently; tests/test_ode_kernels.py holds the two equal on the CPU,
// tests/test_gpu_ode_kernels.py holds every integrator kernel to it bit for bit at the block and finalize edges, and
// tests/test_gpu_wb.py / tests/test_gpu_wb_quad.py hold the water-balance sums to it bit for bit at theirs.
//
// Measured choices: the reductions run on the full one-shot grid rather than a grid-stride loop (4.7 TB/s against
// 5.7 TB/s one-shot, tools/ode_red_bench); waves_tree replaced a serial sum on thread 0 (16 dependent LDS reads per
// accumulator held every 1024-thread block's slot ~1.5 us: k_ewt 105 -> 173 us); finalizing in the producer's
// last-arriving block instead measured slower (tickets on one counter).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace shud {
namespace red {

constexpr int kRedThreads = 1024;   // producing passes: one entry per thread, ceil(n / 1024) blocks
constexpr int kFinThreads = 1024;   // finalize block
constexpr int kFinAcc = 4;          // interleaved accumulators per finalize thread

// single-use streams: non-temporal loads and stores (global_load/store ... nt).  The vectors are far beyond L2; nt
// loads+stores measured 7 % faster on the integrator's five-operand pass (profiles/r03/ode/ode_red_bench.log)
template <class T>
__device__ __forceinline__ T ldn(const T *p) { return __builtin_nontemporal_load(p); }
template <class T>
__device__ __forceinline__ void stn(T *p, T v) { __builtin_nontemporal_store(v, p); }

// mn a compile-time false (a minmask of 0 at the call) folds to the plain add
__device__ inline double comb(double a, double b, bool mn) { return mn ? fmin(a, b) : a + b; }

// the NW wave results of a block (sm[0..NW), one per wave) combined by wave 0: lane l < NW holds sm[l], an xor
// butterfly over offsets NW/2 .. 1 (lanes >= NW never mix in), lane 0 keeps the result
template <int NW>
__device__ inline double waves_tree(const double *sm, bool mn, int lane) {
    static_assert(NW <= 64 && (NW & (NW - 1)) == 0, "power-of-two wave count");
    double x = lane < NW ? sm[lane] : (mn ? INFINITY : 0.0);
#pragma unroll
    for (int off = NW / 2; off >= 1; off >>= 1) x = comb(x, __shfl_xor(x, off, 64), mn);
    return x;
}

// the block's partial of each of NACC accumulators into part[a * nblk + blockIdx.x]; bit a of minmask: accumulator
// a is a min.  Every thread of a kRedThreads-thread block calls it (one barrier); sm is the calling kernel's own
template <int NACC>
__device__ inline void block_partial(double (&v)[NACC], unsigned minmask, double *part, int nblk) {
    constexpr int NW = kRedThreads / 64;
    __shared__ double sm[NACC][NW];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
        const bool mn = (minmask >> a) & 1u;
        double x = v[a];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x = comb(x, __shfl_xor(x, off, 64), mn);
        if (lane == 0) sm[a][wid] = x;
    }
    __syncthreads();
    if (wid == 0) {
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
            const bool mn = (minmask >> a) & 1u;
            const double s = waves_tree<NW>(sm[a], mn, lane);
            if (lane == 0) part[(int64_t)a * nblk + blockIdx.x] = s;
        }
    }
}

// the nblk partials pp[0..nblk) of one quantity; the result is valid on thread 0.  Every thread of a
// kFinThreads-thread block calls it; sm[kFinThreads / 64] is shared scratch the call is done with when it returns
// (two barriers), so a loop over quantities reuses it
__device__ inline double ordered_total(const double *pp, int nblk, bool mn, double *sm) {
    constexpr int NW = kFinThreads / 64;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const double id = mn ? INFINITY : 0.0;
    double acc[kFinAcc];
#pragma unroll
    for (int k = 0; k < kFinAcc; ++k) acc[k] = id;
    for (int b0 = threadIdx.x; b0 < nblk; b0 += kFinAcc * kFinThreads) {
        double v[kFinAcc];
#pragma unroll
        for (int k = 0; k < kFinAcc; ++k) {
            const int b = b0 + k * kFinThreads;
            v[k] = b < nblk ? pp[b] : id;
        }
#pragma unroll
        for (int k = 0; k < kFinAcc; ++k) acc[k] = comb(acc[k], v[k], mn);
    }
    static_assert(kFinAcc == 4, "the pairwise combine below");
    double x = comb(comb(acc[0], acc[1], mn), comb(acc[2], acc[3], mn), mn);
    for (int off = 32; off >= 1; off >>= 1) x = comb(x, __shfl_xor(x, off, 64), mn);
    if (lane == 0) sm[wid] = x;
    __syncthreads();
    const double s = wid == 0 ? waves_tree<NW>(sm, mn, lane) : id;
    __syncthreads();
    return s;
}

}  // namespace red
}  // namespace shud
