// shud_zone.cpp — create-time plan of a zonal print control (shud_zone.h): validation, the stable sort of the columns
// by zone, the chunk table and W_z.  Touches no device, so shud_zone_plan (below) runs on any machine.
#include <cmath>
#include <cstring>

#include "shud_handle.h"
#include "shud_zone.h"

namespace shud {

namespace {
constexpr int kFin = 1024, kAcc = 4;     // red::kFinThreads, red::kFinAcc

// lane 0 of the xor butterfly over offsets m/2 .. 1: stage `off` leaves lane l < off with x[l] + x[l + off]
double tree(double *x, int m) {
    while (m > 1) {
        m /= 2;
        for (int l = 0; l < m; l++) x[l] = x[l] + x[l + m];
    }
    return x[0];
}
// 1024 lanes: the 64-lane butterfly of every wave, then the 16 wave results by waves_tree
double block_tree(double *lanes) {
    double w[kZoneChunk / 64];
    for (int k = 0; k < kZoneChunk / 64; k++) w[k] = tree(lanes + 64 * k, 64);
    return tree(w, kZoneChunk / 64);
}
}  // namespace

double zone_order_sum(const double *p, int64_t n) {
    const int64_t nblk = n > 0 ? (n + kZoneChunk - 1) / kZoneChunk : 1;
    std::vector<double> part((size_t)nblk);
    double lanes[kZoneChunk];
    for (int64_t b = 0; b < nblk; b++) {                         // block_partial
        for (int l = 0; l < kZoneChunk; l++) {
            const int64_t i = b * kZoneChunk + l;
            lanes[l] = i < n ? p[i] : 0.0;
        }
        part[(size_t)b] = block_tree(lanes);
    }
    // ordered_total: lane t, acc[k] += part[t + (4j + k) * 1024]; (acc0 + acc1) + (acc2 + acc3); the block's tree
    std::vector<double> acc((size_t)kAcc * kFin, 0.0);
    for (int64_t b0 = 0; b0 < nblk; b0 += (int64_t)kAcc * kFin)
        for (int k = 0; k < kAcc; k++)
            for (int t = 0; t < kFin; t++) {
                const int64_t b = b0 + (int64_t)k * kFin + t;
                if (b0 + t < nblk) acc[(size_t)k * kFin + t] = acc[(size_t)k * kFin + t] + (b < nblk ? part[(size_t)b] : 0.0);
            }
    for (int t = 0; t < kFin; t++)
        lanes[t] = (acc[t] + acc[kFin + t]) + (acc[2 * kFin + t] + acc[3 * kFin + t]);
    return block_tree(lanes);
}

int zone_plan(const char *name, int n_all, const int32_t *col_src, const ShudZoneSpec *z, ZonePlan *plan) {
    if (!z || !plan || !name) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (n_all < 0) return shud_fail(SHUD_ERR_ARG, "Print_Ctrl %s: bad n_all", name);
    if (z->n_zone < 1) return shud_fail(SHUD_ERR_ARG, "Print_Ctrl %s: n_zone = %d (at least one zone)", name, z->n_zone);
    if (!z->zone) return shud_fail(SHUD_ERR_ARG, "Print_Ctrl %s: null zone", name);
    if (z->op != SHUD_ZONE_SUM && z->op != SHUD_ZONE_WMEAN)
        return shud_fail(SHUD_ERR_ARG, "Print_Ctrl %s: op = %d is neither SHUD_ZONE_SUM nor SHUD_ZONE_WMEAN", name, z->op);
    if (z->op == SHUD_ZONE_WMEAN && !z->weight)
        return shud_fail(SHUD_ERR_ARG, "Print_Ctrl %s: SHUD_ZONE_WMEAN needs a weight", name);
    const int nz = z->n_zone;
    for (int c = 0; c < n_all; c++) {
        if (z->zone[c] < 0 || z->zone[c] > nz)
            return shud_fail(SHUD_ERR_ARG, "Print_Ctrl %s: zone[%d] = %d outside 0..%d", name, c, z->zone[c], nz);
        if (col_src && (col_src[c] < 0 || col_src[c] >= n_all))
            return shud_fail(SHUD_ERR_ARG, "Print_Ctrl %s: col_src[%d] = %d outside the source", name, c, col_src[c]);
    }
    ZonePlan &p = *plan;
    p = ZonePlan();
    p.nz = nz;
    // a stable (counting) sort by zone: ascending column within each zone
    p.zone_off.assign((size_t)nz + 1, 0);
    for (int c = 0; c < n_all; c++)
        if (z->zone[c] > 0) p.zone_off[(size_t)z->zone[c]]++;
    for (int k = 0; k < nz; k++) p.zone_off[(size_t)k + 1] += p.zone_off[(size_t)k];
    const int nm = p.zone_off[(size_t)nz];
    p.member.resize((size_t)nm);
    if (z->weight) p.weight.resize((size_t)nm);
    std::vector<int> at(p.zone_off.begin(), p.zone_off.end() - 1);
    for (int c = 0; c < n_all; c++) {
        if (z->zone[c] <= 0) continue;
        const int i = at[(size_t)z->zone[c] - 1]++;
        p.member[(size_t)i] = col_src ? col_src[c] : c;
        if (z->weight) p.weight[(size_t)i] = z->weight[c];
    }
    p.zone_chunk.assign((size_t)nz + 1, 0);
    for (int k = 0; k < nz; k++) {
        const int lo = p.zone_off[(size_t)k], hi = p.zone_off[(size_t)k + 1];
        for (int f = lo; f < hi; f += kZoneChunk) {
            p.chunk_zone.push_back(k);
            p.chunk_first.push_back(f);
        }
        p.zone_chunk[(size_t)k + 1] = (int)p.chunk_zone.size();
        if (p.zone_chunk[(size_t)k + 1] - p.zone_chunk[(size_t)k] > 1) p.multi.push_back(k);
    }
    if (z->op == SHUD_ZONE_WMEAN) {
        p.wsum.resize((size_t)nz);
        for (int k = 0; k < nz; k++) {
            const int lo = p.zone_off[(size_t)k], hi = p.zone_off[(size_t)k + 1];
            if (hi == lo)
                return shud_fail(SHUD_ERR_ARG, "Print_Ctrl %s: SHUD_ZONE_WMEAN over the empty zone %d", name, k + 1);
            const double w = zone_order_sum(p.weight.data() + lo, hi - lo);
            if (w == 0.0 || !std::isfinite(w))
                return shud_fail(SHUD_ERR_ARG, "Print_Ctrl %s: weight sum of zone %d is %g (SHUD_ZONE_WMEAN needs a "
                                               "finite, non-zero one)", name, k + 1, w);
            p.wsum[(size_t)k] = w;
        }
    }
    return SHUD_OK;
}

}  // namespace shud

// the plan as plain arrays (tests and tools; no device).  member / weight: [n_all]; zone_off: [n_zone + 1]; chunk_zone
// (1-based zone) / chunk_first: [n_all / 1024 + n_zone + 1]; wsum: [n_zone] (WMEAN).  Any output may be NULL.
extern "C" int shud_zone_plan(int32_t n_all, const int32_t *col_src, const ShudZoneSpec *z, int32_t *n_member,
                              int32_t *member, double *weight, int32_t *zone_off, int32_t *n_chunk, int32_t *chunk_zone,
                              int32_t *chunk_first, double *wsum) {
    shud::ZonePlan p;
    const int rc = shud::zone_plan("(plan)", n_all, col_src, z, &p);
    if (rc) return rc;
    if (n_member) *n_member = (int32_t)p.member.size();
    if (n_chunk) *n_chunk = (int32_t)p.chunk_zone.size();
    if (member) memcpy(member, p.member.data(), p.member.size() * sizeof(int32_t));
    if (weight && !p.weight.empty()) memcpy(weight, p.weight.data(), p.weight.size() * sizeof(double));
    if (zone_off) memcpy(zone_off, p.zone_off.data(), p.zone_off.size() * sizeof(int32_t));
    for (size_t k = 0; k < p.chunk_zone.size(); k++) {
        if (chunk_zone) chunk_zone[k] = p.chunk_zone[k] + 1;
        if (chunk_first) chunk_first[k] = p.chunk_first[k];
    }
    if (wsum && !p.wsum.empty()) memcpy(wsum, p.wsum.data(), p.wsum.size() * sizeof(double));
    return SHUD_OK;
}

extern "C" double shud_zone_order_sum(const double *p, int64_t n) { return shud::zone_order_sum(p, n); }
