// shud_diag_host.h — internal, host: what the diagnostics units (shud_out.hip, shud_wb.hip, shud_mon.hip) share on
// the host side: the event timing of their measurement helpers and the reference's binary .dat preamble.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "shud_handle.h"

namespace shud {

// One warm-up pass() then `reps` of them between two HIP events on `stream`; *ms_pass = milliseconds per pass (0.0
// when a pass or a HIP call fails; the code is returned).  pass() returns 0 or an error code and carries the
// caller's own state changes.
template <class Pass>
int time_passes(hipStream_t stream, int reps, Pass pass, double *ms_pass) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0.f;
    auto timed = [&]() -> int {
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        int rc = pass();                             // warm-up
        if (rc) return rc;
        HIP_TRY(hipEventRecord(e0, stream));
        for (int k = 0; k < reps; k++)
            if ((rc = pass())) return rc;
        HIP_TRY(hipEventRecord(e1, stream));
        HIP_TRY(hipEventSynchronize(e1));
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        return 0;
    };
    const int rc = timed();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    *ms_pass = (double)ms / reps;
    return rc;
}

// The preamble of a binary .dat file (Print_Ctrl::open_file, Model_Control.cpp:683-758; writeDatHeader,
// WaterBalanceDiag.cpp:90-130): the fixed 1024-byte zero-filled text header, StartTime, NumVar and the numvar
// column numbers icol.  wb_label != nullptr adds the water-balance files' "# Water-balance diagnostic:" line.
// Returns whether every write succeeded.
inline bool write_dat_preamble(FILE *fp, const char *wb_label, int radiation_input_mode, int terrain_radiation,
                               const char *solar_lonlat_mode, double solar_lon_deg, double solar_lat_deg,
                               double start_time, int numvar, const double *icol) {
    char header[1024];
    memset(header, 0, sizeof(header));
    snprintf(header, sizeof(header),
             "# SHUD output\n"
             "%s%s%s"
             "# Radiation input mode: %s\n"
             "# Terrain radiation (TSR): %s\n"
             "# Solar lon/lat mode: %s\n"
             "# Solar lon/lat (deg): lon=%.6f, lat=%.6f\n",
             wb_label ? "# Water-balance diagnostic: " : "", wb_label ? wb_label : "", wb_label ? "\n" : "",
             radiation_input_mode == 1 ? "SWNET" : "SWDOWN", terrain_radiation ? "ON" : "OFF",
             solar_lonlat_mode ? solar_lonlat_mode : "", solar_lon_deg, solar_lat_deg);
    bool ok = fwrite(header, sizeof(char), 1024, fp) == 1024;
    const double numvar_d = (double)numvar;
    ok &= fwrite(&start_time, sizeof(double), 1, fp) == 1;
    ok &= fwrite(&numvar_d, sizeof(double), 1, fp) == 1;
    if (numvar > 0) ok &= fwrite(icol, sizeof(double), (size_t)numvar, fp) == (size_t)numvar;
    return ok;
}

}  // namespace shud
