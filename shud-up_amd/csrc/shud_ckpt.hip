// shud_ckpt.hip — the checkpoint's pack kernel (include/shud_ckpt.h): one launch copies up to kMaxSeg device
// buffers into one staging slab and forms each one's checksum on the way.
//
// Words move as integers (no floating-point instruction touches them: NaN payloads, signed zeros and denormals
// survive), 16 bytes per lane with non-temporal loads and stores (every stream is single-use; the one-shot shape is
// shud_stream.hip's variant 1, the fastest copy measured on MI355X: each lane of a 256-lane workgroup moves 4 records
// one workgroup-width apart, loads first, then stores).  A source is only 8-byte aligned: the slab offset takes the
// source's 16-byte phase (ckpt::place), so the body is 16-byte aligned on both sides and only a head and a tail word
// fall back to 8-byte accesses (lane 0 of the segment's first workgroup).  A workgroup moves kTiles such tiles
// (128 KiB) before it reduces.
//
// Checksum per segment: c0 = sum w_i, c1 = sum (i + 1) w_i (mod 2^64, i the word index in the segment).  Integer
// addition commutes and associates, so the sums do not depend on lane, wave or workgroup order: reduced in the wave
// (shuffles), across the four waves through LDS, then one 64-bit vector atomic add per workgroup and sum.
#include "shud_ckpt_dev.h"

namespace shud {
namespace ckpt {

typedef unsigned long long u64;
typedef u64 v2u __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ void __launch_bounds__(kLanes) k_ckpt_pack(const SegTable t, u64 *__restrict__ dst, u64 *__restrict__ sums) {
    // this workgroup's segment: the last one that starts at or before it (an empty segment owns no workgroup: it
    // shares blk0 with its successor, which comes later in the table)
    int si = 0;
    for (int k = 1; k < t.nseg; k++)
        if (t.s[k].blk0 <= blockIdx.x) si = k;
    const Seg g = t.s[si];
    const u64 tile = blockIdx.x - g.blk0;
    const u64 head = ((uintptr_t)g.src >> 3) & 1u;                  // g.n > 0: a segment with workgroups
    const u64 npairs = (g.n - head) >> 1, tail = (g.n - head) & 1u;
    const v2u *sp = reinterpret_cast<const v2u *>(g.src + head);
    v2u *dp = dst ? reinterpret_cast<v2u *>(dst + g.dst_off + head) : nullptr;
    u64 c0 = 0, c1 = 0;
    for (int tl = 0; tl < kTiles; tl++) {
        const u64 base = tile * kBlockPairs + (u64)tl * kTilePairs + threadIdx.x;
        if (base - threadIdx.x >= npairs) break;                      // (uniform: the tile's first record)
        v2u v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const u64 p = base + (u64)u * kLanes;
            v[u] = p < npairs ? __builtin_nontemporal_load(&sp[p]) : (v2u){0ull, 0ull};
        }
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const u64 p = base + (u64)u * kLanes;
            if (p < npairs) {
                if (dp) __builtin_nontemporal_store(v[u], &dp[p]);
                const u64 i = head + 2 * p;                           // word index of v[u].x
                c0 += v[u].x + v[u].y;
                c1 += (i + 1) * v[u].x + (i + 2) * v[u].y;
            }
        }
    }
    if (tile == 0 && threadIdx.x == 0) {                              // 8-byte head and tail
        if (head) {
            const u64 w = __builtin_nontemporal_load(&g.src[0]);
            if (dst) __builtin_nontemporal_store(w, &dst[g.dst_off]);
            c0 += w;
            c1 += w;
        }
        if (tail) {
            const u64 i = g.n - 1;
            const u64 w = __builtin_nontemporal_load(&g.src[i]);
            if (dst) __builtin_nontemporal_store(w, &dst[g.dst_off + i]);
            c0 += w;
            c1 += (i + 1) * w;
        }
    }
    c0 = wave_sum(c0);
    c1 = wave_sum(c1);
    __shared__ u64 part[2 * (kLanes / 64)];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[2 * wave] = c0;
        part[2 * wave + 1] = c1;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        u64 a = 0;
#pragma unroll
        for (int w = 0; w < kLanes / 64; w++) a += part[2 * w + threadIdx.x];
        atomicAdd(&sums[2 * si + threadIdx.x], a);
    }
}

void launch_pack(const SegTable &t, uint64_t *dst, unsigned long long *sums, hipStream_t s) {
    if (!t.nblk) return;
    hipLaunchKernelGGL(k_ckpt_pack, dim3(t.nblk), dim3(kLanes), 0, s, t, (u64 *)dst, (u64 *)sums);
}

}  // namespace ckpt
}  // namespace shud
