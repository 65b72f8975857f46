// shud_tables.h — internal: the host tables of a handle, derived once at create from the C-ABI inputs
// (shud_tables.cpp).  Plain vectors and scalars, no device: shud_rhs.cpp uploads them and lets them go,
// shud_rhs_plan_layout reports them.
#pragma once
#include <vector>

#include "shud_dev.h"
#include "shud_rhs.h"

namespace shud {

struct MeshTables {                      // the handle's scalars and the derived arrays of DevMesh
    int mode = SHUD_MODE_SERIAL, NL = 0;
    bool open = false, lakeon = false;   // lakeon: any iLake > 0
    int n_own = 0, n_segghost = 0, n_own_riv = 0;
    int n_int = 0;                       // partitioned: owned prefix independent of ghost data
    int max_col[4] = {0, 0, 0, 0};       // highest BC column referenced: eyBC, eqBC, ryBC, rqBC
    std::vector<int> eflags;             // DevMesh::eflags
    std::vector<int> riv_down, riv_bc;   // reach codes as the kernels see them (into a lake: -3); BC column or 0
    // segments in element-sorted order (stable in reference index); seg_perm: that position -> reference index
    std::vector<int> seg_perm, seg_off, seg_riv;
    std::vector<double> seg_len, seg_cwr;
    // segments by reach (ascending reference order inside a reach): reach_off [NR + 1] over all local reaches, its
    // first n_own_riv + 1 entries are DevMesh::rseg_off; rseg_pos: element-sorted positions, owned reaches (+ 8 pad)
    std::vector<int> reach_off, rseg_pos;
    std::vector<int> up_off, up_idx;     // upstream reaches of each owned reach, ascending (global) id
};

struct PackedTables {                    // DevPacked: its scalars (pointers null) and what its pointers receive
    DevPacked dp{};
    int n_shared = 0;                    // interior edges evaluated once (in-tile edge sharing)
    std::vector<double> ctab, hv;
    std::vector<double2> zz, ged, sg_lc, rrec, rv;
    std::vector<int4> meta, rv_u;
    std::vector<int> seg_first;
};

struct LakeTables {                      // DevLake's lists
    std::vector<int> lake_of, ele_off, ele_idx, bank_off, bank_pos, rin_off, rin_idx;
};

struct HostTables {
    MeshTables mesh;
    bool packed = false;                 // pk is filled: the class-table / 16-byte-record layout
    PackedTables pk;
    LakeTables lake;                     // filled when mesh.lakeon
};

// Validates the inputs and derives every table; SHUD_OK, or a code with shud_fail's message.  part may be NULL.
int build_tables(const ShudMeshSoA *m, const ShudParamsSoA *p, const ShudRhsOptions *opt, const ShudPartition *part,
                 HostTables *out);

}  // namespace shud
