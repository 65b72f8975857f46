// shud_perm.hip — the permute kernel of ordered handles (include/shud_order.h, shud_rhs_permute).
//
// Both directions are gathers, dst[p*n + i] = src[p*n + idx[i]] (idx = perm to the internal numbering, inv to the
// caller's), so the stores are coalesced and only the loads scatter.  One launch moves a whole state vector: a lane
// loads its two indices once (one 8-byte load) and moves its two elements' entries of all three blocks, and the reach
// tail is copied by the same launch.
//
// Access width: a lane owns two consecutive destination elements, so a block whose base is 16-byte aligned is stored
// 16 bytes per lane (8-byte accesses run at 0.54-0.70x the 16-byte rate); a block that starts on an odd double (odd
// n) takes two 8-byte stores — uniform per block, no divergence.  The gathered loads are 8 bytes each and cannot be
// widened.  Cache policy: the source is a single-use stream (a staging copy, a diagnostic array) and is loaded
// non-temporally; the index is read again by every later call and the destination is what the next kernel (or the
// D2H copy) reads, so both stay plain.  No LDS, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace shud {

constexpr int kPermBS = 256;

// PLANES (1 or 3) is a template argument so that a lane's 2 * PLANES gathered loads are all issued before the first
// store waits for one of them
template <int PLANES>
__global__ void __launch_bounds__(kPermBS)
shud_perm_kernel(const int *__restrict__ idx, int n, const double *__restrict__ src, double *__restrict__ dst,
                 int ntail) {
    const int t = blockIdx.x * kPermBS + threadIdx.x;
    const int i = 2 * t;
    if (i < n) {
        const bool two = i + 1 < n;
        int a, b;
        if (two) {                                   // idx comes from hipMalloc: 2*t ints is 8-byte aligned
            const int2 ab = *(const int2 *)(idx + i);
            a = ab.x;
            b = ab.y;
        } else {
            a = b = idx[i];
        }
        double va[PLANES], vb[PLANES];
#pragma unroll
        for (int p = 0; p < PLANES; p++) {
            const double *s = src + (size_t)p * n;
            va[p] = __builtin_nontemporal_load(s + a);
            vb[p] = __builtin_nontemporal_load(s + b);
        }
#pragma unroll
        for (int p = 0; p < PLANES; p++) {
            double *d = dst + (size_t)p * n + i;
            if (two && ((uintptr_t)d & 15u) == 0) {
                *(double2 *)d = make_double2(va[p], vb[p]);
            } else {
                d[0] = va[p];
                if (two) d[1] = vb[p];
            }
        }
    }
    // the reach (and anything else after the element blocks) tail: a straight copy, grid-stride
    const size_t off = (size_t)PLANES * n;
    const int stride = gridDim.x * kPermBS;
    for (int r = t; r < ntail; r += stride) dst[off + r] = __builtin_nontemporal_load(src + off + r);
}

void launch_perm_kernel(const int *idx, int n, int planes, const double *src, double *dst, int ntail, hipStream_t s) {
    const long long pairs = ((long long)n + 1) / 2;
    long long blocks = (pairs + kPermBS - 1) / kPermBS;
    if (blocks < 1) blocks = 1;
    if (n <= 0 && ntail <= 0) return;
    if (planes == 1)
        hipLaunchKernelGGL(shud_perm_kernel<1>, dim3((unsigned)blocks), dim3(kPermBS), 0, s, idx, n, src, dst, ntail);
    else                                             // 3: a state vector or an edge-major array (the callers pass 1 or 3)
        hipLaunchKernelGGL(shud_perm_kernel<3>, dim3((unsigned)blocks), dim3(kPermBS), 0, s, idx, n, src, dst, ntail);
}

}  // namespace shud
