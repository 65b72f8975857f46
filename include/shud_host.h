/* shud_host.h — C-ABI of the C++ host that feeds the device path from a SHUD project directory
 * (SURVEY §8f f4 readers, f1 host side).  libshud_host.so is plain C++ (no HIP); the driver shud_gpu
 * (shud-up_amd/host/shud_gpu.cpp) and the Python tests sit on top of it.
 *
 * It replaces, for the device path, the host half of the reference's setup and time loop:
 *   FileIn paths                       src/classes/IO.cpp:53-91        (input/<prj>/<prj>.<ext>)
 *   Control_Data::read (.cfg.para)     src/classes/Model_Control.cpp:141-502
 *   globalCal::read/push (.cfg.calib)  src/classes/ModelConfigure.cpp:443-459, 109-262
 *   Model_Data::loadinput readers      src/ModelData/MD_readin.cpp:106-363 (mesh, att, soil, geol, lc,
 *                                      riv, rivseg), :555-729 (tsd.forc + forcing csv), :942-951 (lai, mf)
 *   TabularData::read                  src/classes/TabularData.cpp:27-55 (strtold per token)
 *   _TimeSeriesData read_csv/movePointer/getX  src/classes/TimeSeriesData.cpp (zero-order hold)
 *   Model_Data::initialize             src/ModelData/MD_initialize.cpp:168-245 (geometry, calibration,
 *                                      InitElement, rmSinks, applyNabor, rivers, segments)
 *   Model_Data::LoadIC (INIT_MODE 0-3) src/ModelData/MD_initialize.cpp:66-135
 *   Model_Data::initialize_output      src/ModelData/MD_initialize.cpp:246-345 (print controls)
 *   tReadForcing's shared TSR bucket   src/ModelData/MD_ET.cpp:60-136 + solarPosition
 *                                      (src/Equations/SolarRadiation.cpp:92-176, TimeContext.cpp)
 * All returned pointers are owned by the project and stay valid until shud_project_free (forcing rows:
 * until the next shud_project_forcing call).  Errors: non-zero return, message in shud_project_error().
 */
#ifndef SHUD_HOST_H
#define SHUD_HOST_H

#include <stdint.h>

#include "shud_et.h"
#include "shud_rhs.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct shud_project *shud_project_t;

/* Control_Data after read() (Model_Control.hpp:150-232 defaults; Model_Control.cpp:132-137, 502) */
typedef struct {
    double start_time, end_time;         /* CS.StartTime, CS.EndTime [min]                            */
    int64_t num_steps;                   /* CS.NumSteps = (EndTime - StartTime) / SolverStep          */
    double solver_step, et_step;         /* SolverStep (= MAX_SOLVER_STEP), ETStep (LSM_STEP/ET_STEP)  */
    double reltol, abstol, init_step, max_step;
    int32_t init_type, close_boundary, ascii, binary, cryosphere, verbose;
    int32_t terrain_radiation, radiation_input_mode, solar_lonlat_mode;   /* 0 FORCING_FIRST, 1 MEAN, 2 FIXED */
    double solar_lon_deg, solar_lat_deg;  /* selected after the forcing list is read (MD_readin.cpp:645-690) */
    double rad_factor_cap, rad_cosz_min;
    int32_t tsr_integration_step_min;
    int64_t forc_start_time;             /* ForcStartTime (yyyymmdd of the forcing list header)        */
    int32_t num_forc, lakeon, num_lake;
} ShudControl;

/* one print control of initialize_output (MD_initialize.cpp:246-345), in the reference's order */
typedef struct {
    const char *basename;                /* <outdir>/<prj>.<suffix> without extension                 */
    int32_t array;                       /* SHUD_ARR_* of shud_out.h                                   */
    int32_t column;                      /* InitIJ column (QeleSurf/QeleSub j) or -1                   */
    int32_t n_all;                       /* NumEle / NumRiv / NumLake                                  */
    int32_t interval, iflux;             /* Interval [min], 1 = flux (tau 1440)                        */
    const int32_t *flag_io;              /* io_ele / io_riv / io_lake of <prj>.cfg.output (read_cfgout,
                                            MD_readin.cpp:25-104); NULL = every column                   */
} ShudOutputDecl;

/* reads <indir>/<prj>.* and runs the reference's initialisation; `cwd` resolves the forcing csv paths
 * the way the reference (run from its repository root) does; NULL = the process cwd.  end_day >= 0
 * overrides END (days).  The forcing csv files are read in full at load. */
int shud_project_load(const char *indir, const char *prj, const char *cwd, double end_day, shud_project_t *out);
const char *shud_project_error(void);
void shud_project_free(shud_project_t p);

int shud_project_control(shud_project_t p, ShudControl *c);
/* the RHS handle inputs (pointers into the project) */
int shud_project_mesh(shud_project_t p, ShudMeshSoA *mesh, ShudParamsSoA *par);
/* the ET prelude statics and parameters (shud_et_attach) */
int shud_project_et(shud_project_t p, ShudEtMeshSoA *mesh, ShudEtParams *par);
/* named host arrays (tests, driver): "y0" (NY), "y_is", "y_snow" (NE; LoadIC), "x", "y" (centroids),
 * "slope_angle", "aspect" (applyGeometry), "albedo", "fix_pressure", "nx", "ny", "nz".  NULL if unknown. */
const double *shud_project_array(shud_project_t p, const char *name, int64_t *n);
/* print controls for output directory `outdir` (created by the caller); returns the count, fills up to max */
int shud_project_outputs(shud_project_t p, const char *outdir, ShudOutputDecl *decl, int max);
/* output interval [min] of the water-balance diagnostics (include/shud_wb.h): dt_qe_ET if positive, else
 * dt_ye_SURF if positive, else 1440 (choose_interval_min, src/Model/WaterBalanceDiag.cpp:10-19); -1 for NULL */
int shud_project_wb_interval(shud_project_t p);
/* CS.UpdateICStep [min]: Update_IC_STEP of <prj>.cfg.para (Model_Control.cpp:189; default 1440,
 * Model_Control.hpp:181), the schedule of the .cfg.ic.update snapshots (include/shud_mon.h); -1 for NULL */
int shud_project_update_ic_step(shud_project_t p);
/* OUTPUT_MODE and NCOUTPUT_CFG of <prj>.cfg.para (Model_Control.cpp:229-266: LEGACY / NETCDF / BOTH or 0 / 1 / 2; an
 * invalid value fails the load, a key without a value is LEGACY with the reference's warning) with the checks of
 * :591-634 (NETCDF / BOTH without NCOUTPUT_CFG, or with an unreadable one, fail the load; a relative path resolves
 * against the .cfg.para's directory), and the KEY VALUE ncoutput cfg (NetcdfOutputContext.cpp:1093-1153): OUT_DIR,
 * CRS_WKT (a file, read as text), SCHEMA (ignored with the reference's warning).  Relative values of that cfg resolve
 * against the run directory: the parent of the parent of the cfg's directory. */
typedef struct {
    int32_t output_mode;                 /* 0 LEGACY (.dat / .csv), 1 NETCDF, 2 BOTH                             */
    const char *ncoutput_cfg;            /* resolved path of the ncoutput cfg; "" in LEGACY mode                 */
    const char *out_dir;                 /* OUT_DIR, resolved; "" = beside the legacy files                      */
    const char *crs_wkt;                 /* text of the CRS_WKT file; "" = none                                  */
    const char *schema;                  /* SCHEMA, resolved (not used); "" = none                               */
    const char *warnings;                /* the reference's warnings for these keys (also on stderr), '\n'-ended */
} ShudNcOutputCfg;
int shud_project_ncoutput(shud_project_t p, ShudNcOutputCfg *c);
/* the mesh as <prj>.ele.nc describes it: node x (which = 0) / y (1) by node index, n = NumNode; the element node
 * indices [NumEle][3], 1-based as in <prj>.sp.mesh, n = NumEle (centroids: shud_project_array "x" / "y") */
const double *shud_project_node_xy(shud_project_t p, int which, int64_t *n);
const int32_t *shud_project_ele_nodes(shud_project_t p, int64_t *n);
/* Riv[i].type of <prj>.sp.riv, 1-based as in the file (the Type column of <prj>.flood.csv); n = NumRiv */
const int32_t *shud_project_riv_type(shud_project_t p, int64_t *n);
/* a zone table for the zonal outputs (include/shud_out.h, shud_out_add_zonal): one SHUD table (TabularData layout:
 * "nrow ncol", a header line, the rows) of NumEle rows with the columns index and zone; a zone id is an integer >= 0
 * (0: the element is in no zone).  *zone: NumEle ids in the file's element numbering, owned by the project and valid
 * until the next call; *n_zone: the largest id.  Non-zero with shud_project_error's message: a file that cannot be
 * read, a row count that is not NumEle, an id that is not integral, a negative id. */
int shud_project_zones(shud_project_t p, const char *path, const int32_t **zone, int32_t *n_zone);

/* Per ET step [t, tout): updateAllTimeSeries(t) (movePointer of every forcing / LAI / MF series) and the
 * inputs of tReadForcing + ET for shud_et_step: the current station rows, LAI and MF rows, and the TSR
 * bucket decision with the solar samples of a new forcing interval (MD_ET.cpp:60-136).  Errors as the
 * reference's movePointer (missing forcing data -> message, code ERRFileIO). */
int shud_project_forcing(shud_project_t p, double t, double tout, ShudEtForcing *f);

/* Boundary-condition rows at the current ET step (after shud_project_forcing): the rows of <prj>.tsd.ebc1 /
 * .ebc2 / .rbc1 / .rbc2 that f_update reads through getX (MD_update.cpp:114-125, 145-160), as the ele_ybc /
 * ele_qbc / riv_ybc / riv_qbc fields (n_* = data columns) of `in`; the other fields are left untouched.
 * Returns 1 when the model has boundary conditions (pass `in` to shud_rhs_set_step_inputs), 0 otherwise. */
int shud_project_bc_rows(shud_project_t p, ShudStepInputs *in);

/* solarPosition(t_min, lat, lon, Time, tz) (SolarRadiation.cpp:92-176) with the project's ForcStartTime as
 * the base date: out[0..4] = cosZ, zenith, azimuth, declination, hourAngle (KAT tests) */
int shud_project_solar(shud_project_t p, double t_min, double lat_deg, double lon_deg, double tz_hours,
                       double *out5);

#ifdef __cplusplus
}
#endif
#endif /* SHUD_HOST_H */
