// shud_ckpt_dev.h — the pack kernel's segment table (shud_ckpt.hip / shud_ckpt.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace shud {
namespace ckpt {

constexpr int kMaxSeg = 64;              // segments per launch (the table travels as a kernel argument: 2 KiB)
constexpr int kLanes = 256, kUnroll = 4;
constexpr uint64_t kTilePairs = (uint64_t)kLanes * kUnroll;   // 16-byte records per tile (16 KiB)
// tiles a workgroup moves before its one reduction and its two atomic adds (128 KiB per workgroup: the 1.5 GB
// Nordsieck segment of syn-10M then sends 11k adds to its two sum words where one tile per workgroup sent 90k)
constexpr int kTiles = 8;
constexpr uint64_t kBlockPairs = kTilePairs * kTiles;

struct Seg {
    const uint64_t *src;                 // 8-byte aligned
    uint64_t dst_off;                    // words into the slab; same 16-byte phase as src (place())
    uint64_t n;                          // 8-byte words
    uint32_t blk0, pad;                  // first workgroup of this segment
};
struct SegTable {
    Seg s[kMaxSeg];
    int nseg;
    uint32_t nblk;
};

// the first slab offset >= off whose 16-byte phase is that of src: the body of a segment then moves as 16-byte
// records on both sides, whatever the source's alignment
inline uint64_t place(uint64_t off, const void *src) { return off + ((((uintptr_t)src >> 3) ^ off) & 1u); }
inline uint32_t seg_blocks(const void *src, uint64_t n) {
    if (!n) return 0;
    const uint64_t head = ((uintptr_t)src >> 3) & 1u, pairs = (n - head) >> 1;
    const uint64_t b = (pairs + kBlockPairs - 1) / kBlockPairs;
    return (uint32_t)(b ? b : 1);
}

// dst: the slab, or nullptr = verify mode (checksums only).  sums[2 k], sums[2 k + 1] += segment k's c0, c1
// (zeroed by the caller, stream-ordered).
void launch_pack(const SegTable &t, uint64_t *dst, unsigned long long *sums, hipStream_t s);

}  // namespace ckpt
}  // namespace shud
