// shud_mon_fmt.h — internal: the device-free formatters of the run monitors (shud_mon_fmt.cpp), shared with the
// writer thread of shud_mon.hip.  No HIP include.
#pragma once
#include <cstdint>
#include <cstdio>

// packed record of one flooded reach (written by the scatter kernel, read by the writer)
struct ShudFloodRec {
    int32_t idx;                 // reach index, 0-based
    int32_t pad;
    double stage, qdown;
};

// FloodWarning's rows of n records to fp; returns 0 or SHUD_MON_ERR_IO
int shud_mon_fmt_flood_file(FILE *fp, double t, const ShudFloodRec *rec, int64_t n, const int32_t *type,
                            const double *depth);
// PrintInit's file at `path` through <path>.tmp + rename.  Element i's column k is col[k][i * stride] (k: canopy,
// snow, surface, unsat, gw): stride 1 for separate arrays, 5 for packed row-major records
int shud_mon_fmt_write_ic(const char *path, double t, int32_t n_ele, int32_t n_riv, int32_t n_lake,
                          const double *const col[5], int stride, const double *riv, const double *lake);
