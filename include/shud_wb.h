/* shud_wb.h — C-ABI of the water-balance diagnostics on the device (the reference's WaterBalanceDiag,
 * src/Model/WaterBalanceDiag.cpp, switched by SHUD_WB_DIAG; hooks in src/Model/shud.cpp:70-75,110-112,137-152).
 *
 * Everything the diagnostic reads already lives in HBM (the flux arrays of the last f(), DY, the step inputs,
 * the summary arrays, the boundary-condition rows), so the diagnostic does too:
 *   WaterBalanceDiag::onETUpdate   :399-408 -> shud_wb_on_et_update (device copy of the carried qEleE_IC)
 *   WaterBalanceDiag::sample       :410-529 -> shud_wb_sample       (one fused per-element pass + a deterministic
 *                                              basin reduction; nothing crosses PCIe)
 *   WaterBalanceDiag::maybeWrite   :531-636 -> shud_wb_maybe_write  (residual pass at interval ends; only then the
 *                                              four residual arrays and the nine basin values come to the host)
 *   openFiles / writeDatHeader / writeDatRecord :90-150,258-369 -> shud_wb_create / shud_wb_maybe_write
 *   SHUD_WB_DIAG_QUAD: openFiles :271,315,326-338,359-364 -> shud_wb_quad_enable (the sixth file,
 *                                              <prefix>.basinwbfull_quad.dat); the basin rates of f()
 *                                              (MD_f.cpp:57-86,115-128,193-213) and onCvodeMonitorStep :681-717
 *                                              -> shud_wb_quad_step (a rates-only pass + the same reduction; the
 *                                              trapezoid at the solver's own dt on device scalars); the quad row
 *                                              of maybeWrite :597-623 -> shud_wb_maybe_write
 * Unsupported handles (SHUD_ERR_UNSUPPORTED): OMP semantics (the per-element ET terms exist only in the serial
 * path), lake models (the reference's diagnostic ignores lake storage), partitioned handles.
 *
 * Call order per solver step (the reference's loop; include/shud_out.h for the first and third call):
 *   shud_rhs_summary, [shud_rhs_eval: the reference's extra, stateful f()], shud_rhs_refresh_diagnostics,
 *   shud_ode_get_dky(k = 1), shud_wb_sample, shud_wb_maybe_write, shud_out_export;
 * and shud_wb_on_et_update after every shud_et_step / shud_rhs_set_step_inputs that sets e_ic.
 * With the quad monitor (shud.cpp:113-135) the integrator runs to tout one internal step at a time:
 *   shud_ode_set_stop_time(tout); while (t + ZERO < tout) { shud_ode_solve(.., SHUD_ODE_ONE_STEP),
 *   shud_rhs_eval (stateful, on the returned state), shud_rhs_refresh_diagnostics, shud_wb_quad_step(t) }
 * and the per-solver-step calls above follow unchanged.
 */
#ifndef SHUD_WB_H
#define SHUD_WB_H

#include <stdint.h>

#include "shud_rhs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a diagnostic file could not be opened, written, flushed or closed (full disk, ...): returned by shud_wb_create,
 * shud_wb_maybe_write and shud_wb_destroy beside the SHUD_ERR_* codes of shud_rhs.h */
#define SHUD_WB_ERR_IO -6

/* the seven basin rates / accumulators, in the order of the basin row's columns 2..8 */
enum { SHUD_WB_P = 0, SHUD_WB_ET, SHUD_WB_QOUT, SHUD_WB_QEDGE, SHUD_WB_QBC, SHUD_WB_QSS, SHUD_WB_NONCONS,
       SHUD_WB_NBASIN };

typedef struct ShudWbOptions {
    double  start_time;            /* CS.StartTime [min]: the first sample's dt is t - start_time          */
    int32_t interval_min;          /* output interval [min] (shud_project_wb_interval)                     */
    int32_t trapz;                 /* SHUD_WB_DIAG_TRAPZ: 0.5*(prev + rate)*dt once a previous rate exists */
    int64_t forc_start_time;       /* ForcStartTime, written into the header as a double                   */
    int32_t radiation_input_mode;  /* header: 0 SWDOWN, 1 SWNET                                             */
    int32_t terrain_radiation;     /* header: TSR ON/OFF                                                    */
    const char *solar_lonlat_mode; /* header: SolarLonLatModeName(...)                                      */
    double  solar_lon_deg, solar_lat_deg;
    const char *prefix;            /* <outpath>/<prj><suffix>: the five files are <prefix>.elewb3_resid.dat ...;
                                      NULL = no files (shud_wb_read only)                                   */
} ShudWbOptions;

/* host copies for shud_wb_read; any pointer may be NULL; arrays hold num_ele values */
typedef struct ShudWbOut {
    double *acc3, *accfull, *acc3_budget, *accfull_budget;         /* the four accumulators as they stand    */
    double *resid3, *residfull, *resid3_budget, *residfull_budget; /* residuals of the last written row      */
    double basin_acc[SHUD_WB_NBASIN];   /* basin accumulators [m3] as they stand                            */
    double basin_rate[SHUD_WB_NBASIN];  /* basin rates [m3/min] of the last sample that integrated           */
    double basin_row[9];                /* last written basin row: dS, P, ET, Qout, Qedge, Qbc, Qss, noncons, resid */
    double storage[2];                  /* basin element / river storage [m3] of the last snapshot           */
    double last_t;                      /* time of the last sample                                           */
    int64_t rows;                       /* rows written so far                                               */
    int32_t n_outlets;                  /* reaches in the outlet list                                        */
} ShudWbOut;

typedef struct shud_wb *shud_wb_t;

/* openFiles: uploads area, Sy and the per-element flags (domain-boundary edges, iBC, iSS), builds the outlet
 * list, takes the initial storage snapshots from the handle's SHUD_ARR_Y_* arrays (run shud_rhs_summary on y0
 * first; yEleIS / yEleSnow read as 0.0 without an ET prelude) and writes the five headers. */
int shud_wb_create(shud_rhs_t h, const ShudMeshSoA *mesh, const ShudParamsSoA *par, const ShudWbOptions *opt,
                   shud_wb_t *out);
/* onETUpdate: ic_raw = the carried qEleE_IC the next RHS call will read (stream-ordered) */
int shud_wb_on_et_update(shud_wb_t wb);
/* sample(t, DY): d_dy is the device vector [sf|us|gw|riv] of CVodeGetDky(k = 1); the handle's diagnostic arrays
 * must hold the last f() (shud_rhs_refresh_diagnostics).  Stream-ordered on the handle's stream, no host
 * synchronisation.  A non-positive dt only records t. */
int shud_wb_sample(shud_wb_t wb, double t, const double *d_dy);
/* maybeWrite(t): 1 = a row was written (residuals formed, snapshots rolled, accumulators zeroed), 0 = not an
 * interval end, < 0 = error (SHUD_ERR_*).  Reads the handle's SHUD_ARR_Y_* arrays (shud_rhs_summary first).
 * With the quad monitor enabled the quad row (the basin row's dS and time) follows the basin row and the quad
 * accumulators are zeroed; the previous quad rates and quad_last_t are kept. */
int shud_wb_maybe_write(shud_wb_t wb, double t);
/* host copies of the diagnostic's state (tests; synchronises the stream) */
int shud_wb_read(shud_wb_t wb, ShudWbOut *out);
/* flushes and closes the files, frees the device arrays; returns the first write error (SHUD_WB_ERR_IO), if any */
int shud_wb_destroy(shud_wb_t wb);
/* ---- measurement helper (tools/wb_sample_time.py), not part of the supported interface ----
 * `reps` sample passes with dt = 1 min between HIP events on the handle's stream; *ms_sample = milliseconds per
 * sample.  It integrates like shud_wb_sample (accumulators, sample time and previous rates move): use it on a
 * diagnostic made for timing only. */
int shud_wb_time_samples(shud_wb_t wb, const double *d_dy, int reps, double *ms_sample);

/* ---- SHUD_WB_DIAG_QUAD: the CV_ONE_STEP monitor ----
 * Call once, after shud_wb_create and before the first shud_wb_sample / shud_wb_quad_step (otherwise SHUD_ERR_ARG):
 * allocates the quad scalars (seven rates, previous rates and accumulators, all 0; quad_last_t = start_time), opens
 * <prefix>.basinwbfull_quad.dat and writes its header (no file with a NULL prefix; SHUD_WB_ERR_IO if it cannot). */
int shud_wb_quad_enable(shud_wb_t wb);
/* onCvodeMonitorStep(t) on the flux arrays of the monitor's f() (shud_rhs_eval + shud_rhs_refresh_diagnostics
 * first; SHUD_ERR_ARG on a handle that has no evaluation to replay or never refreshed): the seven basin rates, Qout
 * as the sum of QrivDown over the outlet list, then acc += rate*dt on the first integrating step and
 * acc += 0.5*(prev + rate)*dt on every later one, whatever ShudWbOptions.trapz says.  A non-positive dt only records
 * t.  Stream-ordered, no host synchronisation; leaves the sample's accumulators and previous rates alone. */
int shud_wb_quad_step(shud_wb_t wb, double t);
/* host copies of the quad state (tests; synchronises the stream); any pointer may be NULL.  row: the last written
 * quad row {dS, P, ET, Qout, Qedge, Qbc, Qss, noncons, resid}; last_t: quad_last_t */
int shud_wb_read_quad(shud_wb_t wb, double acc[7], double rate[7], double row[9], double *last_t);
/* measurement helper like shud_wb_time_samples: `reps` monitor passes (element pass, reach pass, finalize) with
 * dt = 1 min; the quad accumulators, previous rates and quad_last_t move */
int shud_wb_time_quad(shud_wb_t wb, int reps, double *ms_pass);

#ifdef __cplusplus
}
#endif
#endif /* SHUD_WB_H */
