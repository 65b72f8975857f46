// shud_zone.h — internal: the create-time plan of a zonal print control (shud_out_add_zonal, include/shud_out.h).
// Host-side and device-free, like shud_tables.cpp: shud_zone_plan (include/shud_out.h) shows it on any machine.
#pragma once
#include <cstdint>
#include <vector>

#include "shud_out.h"

namespace shud {

constexpr int kZoneChunk = 1024;         // members per chunk = red::kRedThreads: one block_partial each

struct ZonePlan {
    int nz = 0;
    std::vector<int> member;             // source index (col_src applied) of every member, zone-major (zone 1 first),
                                         // ascending caller column within a zone; columns of zone 0 are absent
    std::vector<double> weight;          // the members' weights in member order; empty when the spec has none
    std::vector<int> zone_off;           // [nz + 1] zone z (1-based) owns members zone_off[z-1] .. zone_off[z]
    std::vector<int> zone_chunk;         // [nz + 1] ... and chunks (= partials) zone_chunk[z-1] .. zone_chunk[z]
    std::vector<int> chunk_zone;         // [n_chunk] 0-based zone of the chunk
    std::vector<int> chunk_first;        // [n_chunk] its first member; it ends 1024 on, or with its zone
    std::vector<int> multi;              // 0-based zones of more than one chunk (the finalize's ordered_total blocks)
    std::vector<double> wsum;            // [nz] W_z = zone_order_sum of the zone's weights (WMEAN only)
};

// shud_reduce.h's order (block_partial over chunks of 1024 with 0.0 past n, then ordered_total) on the host, in plain
// IEEE additions: W_z is formed with it once per control.  tests/test_zonal.py holds it to
// ode_kernels_py.device_order_sum, and tests/test_gpu_zonal.py holds the device to the same restatement.
double zone_order_sum(const double *p, int64_t n);

// Validates col_src, the zone ids and (WMEAN) the weights, and derives the plan.  name: the control, for messages.
// SHUD_OK, or SHUD_ERR_ARG with shud_fail's message naming the field.
int zone_plan(const char *name, int n_all, const int32_t *col_src, const ShudZoneSpec *z, ZonePlan *plan);

}  // namespace shud
