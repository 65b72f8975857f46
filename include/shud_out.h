/* shud_out.h — C-ABI of the output path on the device (`.dat` binary outputs).
 *
 * Replaces, for a model whose state and fluxes live in HBM (shud_rhs.h / shud_ode.h), the reference's
 *   Model_Data::summary(udata)          src/ModelData/MD_update.cpp:190-216   -> shud_rhs_summary
 *   Control_Data::ExportResults(t)      src/classes/Model_Control.cpp:123-127 -> shud_out_export
 *   Print_Ctrl::Init / InitIJ           src/classes/Model_Control.cpp:759-858 -> shud_out_add
 *   Print_Ctrl::open_file               src/classes/Model_Control.cpp:683-758 (1024-B header, StartTime,
 *                                        NumVar, icol[NumVar]; optional ASCII twin)
 *   Print_Ctrl::PrintData               src/classes/Model_Control.cpp:926-960 (running sum, mean over the
 *                                        interval times tau, quantised left-endpoint time stamp, reset)
 *   Print_Ctrl::fun_printBINARY/ASCII   src/classes/Model_Control.cpp:893-909
 * Each exported step adds every registered variable into its device-resident buffer with one batched
 * kernel (no PCIe traffic); only at the end of an output interval is the buffer scaled on the device,
 * copied to the host and written, in the reference's byte layout.
 *
 * NetCDF sinks (OUTPUT_MODE NETCDF / BOTH; MD_initialize.cpp:346-371, NetcdfOutputContext.cpp:953-1085): up to three
 * files of include/shud_nc.h are attached to an output set and a control is registered with a sink in one of them,
 * alone or beside its .dat / .csv.  At the interval's end the control's record slab is formed on the device (the
 * float of the same mean, big-endian, fill at unselected columns) and crosses PCIe at 4 bytes per value.
 */
#ifndef SHUD_OUT_H
#define SHUD_OUT_H

#include <stdint.h>

#include "shud_nc.h"
#include "shud_rhs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* device arrays a print control can point at (shud_rhs_device_array) */
enum {
    /* Model_Data::summary (filled by shud_rhs_summary from a state vector) */
    SHUD_ARR_Y_ELE_SURF = 0,     /* yEleSurf                                     NE  */
    SHUD_ARR_Y_ELE_UNSAT,        /* yEleUnsat                                    NE  */
    SHUD_ARR_Y_ELE_GW,           /* yEleGW (yBC where iBC > 0)                   NE  */
    SHUD_ARR_Y_RIV_STG,          /* yRivStg (Riv.yBC where BC > 0)              NR  */
    SHUD_ARR_Y_LAKE_STG,         /* yLakeStg: lake entries of the last RHS input NL  */
    /* fluxes of the last RHS evaluation (filled by shud_rhs_refresh_diagnostics) */
    SHUD_ARR_QELE_SURF_TOT,      /* QeleSurfTot                                  NE  */
    SHUD_ARR_QELE_SUB_TOT,       /* QeleSubTot                                   NE  */
    SHUD_ARR_QELE_SURF,          /* QeleSurf, edge-major [3][NE]: column j at +j*NE   */
    SHUD_ARR_QELE_SUB,           /* QeleSub,  edge-major [3][NE]                      */
    SHUD_ARR_QE2R_SURF,          /* Qe2r_Surf                                    NE  */
    SHUD_ARR_QE2R_SUB,           /* Qe2r_Sub                                     NE  */
    SHUD_ARR_Q_INFIL,            /* qEleInfil                                    NE  */
    SHUD_ARR_Q_EXFIL,            /* qEleExfil                                    NE  */
    SHUD_ARR_Q_RECHARGE,         /* qEleRecharge                                 NE  */
    SHUD_ARR_Q_ETA,              /* qEleETA                                      NE  */
    SHUD_ARR_Q_E_IC,             /* qEleE_IC (as mutated by the last RHS)        NE  */
    SHUD_ARR_Q_TRANS,            /* qEleTrans = qTu + qTg; 0 on a lake element  NE  */
    SHUD_ARR_Q_EVAPO,            /* qEleEvapo = qEu + qEg + qEs; qPotEvap on a lake element NE */
    SHUD_ARR_QRIV_DOWN,          /* QrivDown                                     NR  */
    SHUD_ARR_QRIV_UP,            /* QrivUp                                       NR  */
    SHUD_ARR_QRIV_SURF,          /* QrivSurf                                     NR  */
    SHUD_ARR_QRIV_SUB,           /* QrivSub                                      NR  */
    /* per-ET-step inputs on the device (after shud_rhs_set_step_inputs or shud_et_step) */
    SHUD_ARR_Q_PRCP,             /* qElePrep                                     NE  */
    SHUD_ARR_Q_NET_PRCP,         /* qEleNetPrep                                  NE  */
    SHUD_ARR_Q_ETP,              /* qEleETP                                      NE  */
    /* ET-step prelude state (shud_et_attach'ed handles; NULL otherwise) */
    SHUD_ARR_Y_ELE_IS,           /* yEleIS (interception storage)                NE  */
    SHUD_ARR_Y_ELE_SNOW,         /* yEleSnow                                     NE  */
    SHUD_ARR_RN_H,               /* ele_rn_h_wm2: forcing shortwave (MD_ET.cpp:201) NE */
    SHUD_ARR_RN_T,               /* ele_rn_t_wm2: terrain-corrected shortwave    NE  */
    SHUD_ARR_RN_FACTOR,          /* ele_rn_factor: TSR factor                    NE  */
    /* lake fluxes of the last RHS evaluation (lake models; MD_initialize.cpp:331-342 order) */
    SHUD_ARR_LAKE_TOPAREA,       /* y2LakeArea                                   NL  */
    SHUD_ARR_Q_LAKE_EVAP,        /* qLakeEvap                                    NL  */
    SHUD_ARR_Q_LAKE_PRCP,        /* qLakePrcp                                    NL  */
    SHUD_ARR_Q_LAKE_RIVIN,       /* QLakeRivIn                                   NL  */
    SHUD_ARR_Q_LAKE_RIVOUT,      /* QLakeRivOut: zeroed by f_update, never assigned (MD_update.cpp:184) NL */
    SHUD_ARR_Q_LAKE_SURF,        /* QLakeSurf                                    NL  */
    SHUD_ARR_Q_LAKE_SUB,         /* QLakeSub                                     NL  */
    SHUD_ARR_COUNT
};

/* fills the SHUD_ARR_Y_* arrays from y (device pointer, NY values; the Model_Data::summary step).  yLakeStg is not
 * summary's: the reference sets it in LoadIC and f_update (MD_update.cpp:175), so it is taken from y only before
 * the handle's first evaluation (the initial condition) and by shud_rhs_refresh_diagnostics afterwards */
int shud_rhs_summary(shud_rhs_t h, const double *d_y);
/* replays the last RHS evaluation with diagnostic stores into the device arrays (no host copy; carried
 * state unchanged): what the reference's flux arrays, yLakeStg and y2LakeArea hold after CVODE's last f() call */
int shud_rhs_refresh_diagnostics(shud_rhs_t h);
/* allocates every array above (zero-filled) without evaluating anything, so print controls can be registered
 * before the first RHS call (the serial RHS is stateful: an extra evaluation would change the trajectory) */
int shud_rhs_prepare_outputs(shud_rhs_t h);
/* device pointer of one of the arrays above (NULL if unknown / not yet materialised) and its length */
const double *shud_rhs_device_array(shud_rhs_t h, int which, int64_t *n);

typedef struct shud_out *shud_out_t;

typedef struct {
    const char *basename;        /* Print_Ctrl::filename: writes <basename>.dat and/or <basename>.csv     */
    const double *d_src;         /* device array with n_all values (PrintVar targets), stride 1             */
    int32_t n_all;               /* NumAll                                                                  */
    const int32_t *flag_io;      /* host, n_all flags (Init with flag_IO); NULL = every column              */
    int32_t interval;            /* Interval [min] (> 0; the reference exits with ERRCONSIS on 0)           */
    int32_t iflux;               /* tau = 1440 if iflux else 1                                              */
    int64_t start_time;          /* StartTime (ForcStartTime, written into the header as a double)          */
    int32_t binary, ascii;       /* files to write (reference defaults: binary 1, ascii 0)                  */
    int32_t radiation_input_mode;/* header: 0 SWDOWN, 1 SWNET                                               */
    int32_t terrain_radiation;   /* header: TSR ON/OFF                                                      */
    const char *solar_lonlat_mode; /* header: SolarLonLatModeName(...)                                      */
    double solar_lon_deg, solar_lat_deg;
} ShudPrintSpec;

/* an output set on `stream` (hipStream_t; NULL = the default stream) of `device` */
int shud_out_create(int device, void *stream, shud_out_t *out);
/* Print_Ctrl::Init[IJ] + open_file: creates/truncates the files and writes their headers */
int shud_out_add(shud_out_t o, const ShudPrintSpec *spec);
/* on != 0: controls added from now on keep the files of an earlier run (include/shud_ckpt.h) — opened without
 * truncation, the header compared with the one shud_out_add writes (SHUD_ERR_ARG if it differs or the file is
 * missing), positioned at the end; shud_ckpt_restore then cuts each file back to its length at the checkpoint. */
int shud_out_resume(shud_out_t o, int on);
/* shud_out_add over a source in another numbering (include/shud_order.h): column c of the file reads
 * d_src[col_src[c]], col_src host [n_all] with values in [0, n_all); flag_io and the header's column numbers are
 * still indexed by the caller's column c.  A create-time change: the export kernel already reads index lists. */
int shud_out_add_mapped(shud_out_t o, const ShudPrintSpec *spec, const int32_t *col_src);
/* Zonal controls: a print control that reduces its source to one value per zone BEFORE accumulating, so its state is
 * n_zone doubles and n_zone * 8 bytes cross PCIe per interval.  At every shud_out_export, for each zone z = 1..n_zone:
 *   members: the columns c with zone[c] == z, ascending c; term p_c = weight[c] * x_c (one IEEE multiplication, never
 *   fused into an addition), or x_c without a weight; x_c = d_src[col_src ? col_src[c] : c];
 *   S_z = the project's deterministic order (csrc/shud_reduce.h) over the zone's own term vector: block_partial over
 *   chunks of 1024 consecutive members (0.0 past the last), then ordered_total over the zone's partials; an empty zone
 *   has S_z = +0.0; buf_z += S_z.
 * At the interval's end the row holds buf_z * (tau / NumUpdate) (SHUD_ZONE_SUM), or that product divided by
 * W_z = the same ordered sum of the zone's weights, formed once at registration (SHUD_ZONE_WMEAN); then buf_z = 0.
 * The file has NumVar = n_zone and icol = 1..n_zone; header, time stamps and interval rule are any control's. */
enum { SHUD_ZONE_SUM = 0, SHUD_ZONE_WMEAN = 1 };
typedef struct {
    int32_t n_zone;              /* NZ >= 1                                                                  */
    const int32_t *zone;         /* host, n_all ids in the caller's column numbering: 0 = in no zone, 1..NZ  */
    const double *weight;        /* host, n_all weights by caller column; NULL = unweighted (SUM only)       */
    int32_t op;                  /* SHUD_ZONE_SUM / SHUD_ZONE_WMEAN                                          */
} ShudZoneSpec;
/* registers a zonal control over spec->d_src (n_all values; col_src NULL or as in shud_out_add_mapped).  Refused with
 * SHUD_ERR_ARG and nothing created: n_zone < 1, a zone id outside 0..NZ, a non-NULL spec->flag_io, WMEAN without a
 * weight, WMEAN with an empty zone or a W_z that is zero or not finite, a col_src entry out of range.  Zonal controls
 * have no NetCDF sink.  All zonal controls of a set share two launches per export; plain controls launch what they
 * launch without them. */
int shud_out_add_zonal(shud_out_t o, const ShudPrintSpec *spec, const int32_t *col_src, const ShudZoneSpec *zones);
/* the create-time plan of shud_out_add_zonal as plain arrays, without a device (tests, tools): the member list (source
 * indices, zone-major, ascending column within a zone) and the weights in member order [n_all each], zone_off
 * [n_zone + 1], the chunk table (1-based zone and first member of every 1024-member chunk; [n_all / 1024 + n_zone + 1]
 * each) and W_z [n_zone] (WMEAN).  Any output may be NULL.  Same refusals as shud_out_add_zonal. */
int shud_zone_plan(int32_t n_all, const int32_t *col_src, const ShudZoneSpec *zones, int32_t *n_member, int32_t *member,
                   double *weight, int32_t *zone_off, int32_t *n_chunk, int32_t *chunk_zone, int32_t *chunk_first,
                   double *wsum);
/* the ordered sum above of p[0..n) on the host (W_z is formed with it) */
double shud_zone_order_sum(const double *p, int64_t n);
/* the kernels an output set launches, and how many launches of each it has enqueued so far (every launch site of the
 * set counts, the measurement entries included): what a run launches can be asserted without a profiler */
enum {
    SHUD_OUT_K_ACCUMULATE = 0,   /* k_accumulate: one per export, over the plain controls                    */
    SHUD_OUT_K_SNAP,             /* k_snap: one per finished row of a control without a NetCDF sink          */
    SHUD_OUT_K_SNAP_NC,          /* k_snap_nc / k_snap_nc_sel: one per finished row of a control with a sink */
    SHUD_OUT_K_SNAP_NC_SEL,
    SHUD_OUT_K_ZONE_PARTIAL,     /* k_zone_partial, k_zone_final: one each per export of a set with zonal controls */
    SHUD_OUT_K_ZONE_FINAL,
    SHUD_OUT_K_SNAP_WMEAN,       /* k_snap_wmean: one per finished row of a SHUD_ZONE_WMEAN control          */
    SHUD_OUT_KERNELS
};
int shud_out_launches(shud_out_t o, int64_t counts[SHUD_OUT_KERNELS]);
/* the kernel's name as it appears in a trace, NULL outside the enum */
const char *shud_out_kernel_name(int which);
/* measurement only (tools/zonal_bench.py): device time [ms] of one export's per-step pass, averaged over `reps` passes
 * after a warm-up: which = 0 the two zonal launches, 1 k_accumulate over the plain controls.  The accumulators grow. */
int shud_out_time_pass(shud_out_t o, int which, int reps, double *ms_pass);
/* attaches the NetCDF file spec->kind describes (one per kind) to the output set; controls are then registered into
 * it with shud_out_add_nc.  Nothing is written yet; an OUT_DIR that exists and is no directory is refused here. */
int shud_out_attach_nc(shud_out_t o, const ShudNcSpec *spec);
/* shud_out_add / shud_out_add_mapped (col_src NULL / non-NULL) with a NetCDF sink in the attached file `kind`
 * (setSink, MD_initialize.cpp:348-356): the variable is named after the leaf of spec->basename past its last dot.
 * legacy != 0 (OUTPUT_MODE BOTH): the .dat / .csv of spec->binary / ascii are written too, from the same product;
 * legacy == 0 (NETCDF): neither is opened and no double snapshot is copied (MD_initialize.cpp:362-363).
 * A NetCDF header cannot grow after its first record: refused once the headers are final (shud_out_nc_begin). */
int shud_out_add_nc(shud_out_t o, const ShudPrintSpec *spec, const int32_t *col_src, int32_t kind, int32_t legacy);
/* writes the header and the fixed variables of every attached file that has a control; implied by the first
 * shud_out_export.  A file that never gets a record stays valid, with 0 records. */
int shud_out_nc_begin(shud_out_t o);
/* measurement only (tools/nc_bench.py): device time [ms] of one launch of control k's interval-end kernel (the mean,
 * the float slab, the snapshot in BOTH mode, the zeroing), averaged over `reps` back-to-back launches after a warm-up.
 * It zeroes the control's accumulator. */
int shud_out_time_nc(shud_out_t o, int k, int reps, double *ms_pass);
/* Control_Data::ExportResults(t): every control adds its source into its buffer; controls whose interval
 * ends at t (floor(t + 0.001) % Interval == 0) write the interval mean and reset.  Sources must hold the
 * values to export (shud_rhs_summary / shud_rhs_refresh_diagnostics first), stream-ordered.  The rows of a
 * finished interval reach the files asynchronously (copy stream + writer thread; same bytes, same order):
 * shud_out_flush / shud_out_rows / shud_out_destroy wait for them. */
int shud_out_export(shud_out_t o, double t);
/* wait until every exported row is written to the files (fflush'ed).  Returns the first failure of the
 * asynchronous writer (a failed snapshot copy: that row is not written; a file write / flush error) */
int shud_out_flush(shud_out_t o);
/* number of rows written so far by control k (tests; waits for the writer); a writer failure returns its
 * negative SHUD_ERR_* code */
int64_t shud_out_rows(shud_out_t o, int k);
/* flushes and closes the files, frees the buffers; returns the writer's first failure, if any */
int shud_out_destroy(shud_out_t o);

#ifdef __cplusplus
}
#endif
#endif /* SHUD_OUT_H */
