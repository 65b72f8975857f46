/* shud_mon.h — C-ABI of the run monitors on the device: flood alerts and restart (initial-condition) snapshots.
 *
 * Replaces, for a model whose state and fluxes live in HBM (shud_rhs.h / shud_out.h), the reference's
 *   FloodAlert::InitAlert/InitPointer/InitPara/InitFile   src/classes/FloodAlert.cpp:9-69    -> shud_mon_add_flood
 *   FloodAlert::FloodWarning(t)                           src/classes/FloodAlert.cpp:71-87   -> shud_mon_flood
 *   Model_Data::PrintInit(fn, t)                          src/ModelData/MD_update.cpp:268-299 -> shud_mon_add_ic,
 *                                                          shud_mon_ic_update, shud_mon_write_ic_host
 * (called at src/Model/shud.cpp:76,97,154,157; file names src/classes/IO.cpp:185-186: <prj>.cfg.ic.update,
 * <prj>.cfg.ic.bak, <prj>.flood.csv).  A monitor set is independent of the RHS handle: it takes plain device
 * pointers and sizes.  Reaches above their bank are selected and packed on the device (order-preserving stream
 * compaction) and only the packed records cross PCIe; a due snapshot is packed into row-major records on the
 * device and copied on a copy stream into one of two pinned banks; one writer thread formats both files off the
 * caller's critical path.  The bytes are the reference's.  Deviation: a snapshot is written to <path>.tmp and
 * renamed over <path>, so a killed run never leaves a truncated restart file (the final bytes are the same).
 * Arrays of a partitioned handle are in local numbering: a caller would need its permutation (not provided).
 */
#ifndef SHUD_MON_H
#define SHUD_MON_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* file open / write / rename failure (beside the SHUD_ERR_* codes of shud_rhs.h; errno holds the cause) */
#define SHUD_MON_ERR_IO -6

typedef struct shud_mon *shud_mon_t;

/* a monitor set on `stream` (hipStream_t; NULL = the default stream) of `device` */
int shud_mon_create(int device, void *stream, shud_mon_t *out);

typedef struct {
    const char *path;            /* <outdir>/<prj>.flood.csv: created/truncated, header written at add          */
    const double *d_stage;       /* device, n_riv: yRivStg  (SHUD_ARR_Y_RIV_STG)                                */
    const double *d_qdown;       /* device, n_riv: QrivDown (SHUD_ARR_QRIV_DOWN)                                */
    int32_t n_riv;
    const double *riv_depth;     /* host, n_riv: para[itype[i]].depth (ShudMeshSoA.riv_depth); copied            */
    const int32_t *riv_type;     /* host, n_riv: Riv[i].type, 1-based, printed as is; copied                     */
} ShudFloodSpec;
/* FloodAlert::Init*: once per monitor set */
int shud_mon_add_flood(shud_mon_t m, const ShudFloodSpec *s);
/* on != 0, before shud_mon_add_flood: the flood file of an earlier run is kept (include/shud_ckpt.h) — opened
 * without truncation, its header line compared, positioned at its end; shud_ckpt_restore then cuts it back to its
 * length at the checkpoint and sets the row and snapshot counters. */
int shud_mon_resume(shud_mon_t m, int on);
/* FloodWarning(t) on the current contents of d_stage / d_qdown (stream-ordered): reach i gets a row iff
 * stage[i] > depth[i] (strict: a NaN stage gives no row, +inf does), rows in ascending i, calls in call order.
 * Returns after enqueue; waits only when both banks are still with the writer. */
int shud_mon_flood(shud_mon_t m, double t);
/* total rows written so far; waits for the writer; a writer failure returns its negative error code */
int64_t shud_mon_flood_rows(shud_mon_t m);
/* FloodWarning's return value for the last shud_mon_flood call (1 = flood, 0 = none); waits; < 0 = error */
int shud_mon_flood_last(shud_mon_t m);

typedef struct {
    const char *path_update;     /* <outdir>/<prj>.cfg.ic.update                                                 */
    int32_t update_ic_step;      /* CS.UpdateICStep [min], >= 1 (0 divides by zero in the reference: SHUD_ERR_ARG) */
    int32_t n_ele, n_riv, n_lake;
    const double *d_is, *d_snow, *d_surf, *d_unsat, *d_gw;   /* device, n_ele: yEleIS, yEleSnow, yEleSurf/Unsat/GW */
    const double *d_riv;         /* device, n_riv: yRivStg                                                       */
    const double *d_lake;        /* device, n_lake: yLakeStg (NULL when n_lake == 0)                             */
} ShudIcSpec;
/* PrintInit's sources and schedule: once per monitor set */
int shud_mon_add_ic(shud_mon_t m, const ShudIcSpec *s);
/* The element arrays of the snapshot are in an internal numbering (include/shud_order.h): perm[k] (host, n_ele) is
 * the caller's index of source element k, and the file lists the elements in the caller's order.  After
 * shud_mon_add_ic; applies to every later snapshot. */
int shud_mon_set_ic_order(shud_mon_t m, const int32_t *perm);
/* PrintInit(Init_update, t): a snapshot is due iff ((unsigned long)(long)t) % update_ic_step == 0.  Returns 1 when
 * a snapshot of the arrays' current contents (stream-ordered) was queued, 0 when not due, < 0 on error.  Every
 * snapshot replaces the previous file. */
int shud_mon_ic_update(shud_mon_t m, double t);
/* snapshots written so far; waits for the writer; a writer failure returns its negative error code */
int64_t shud_mon_ic_snapshots(shud_mon_t m);

/* waits until every queued row / snapshot is in its file; returns the writer's first failure (a failed copy:
 * that call's rows / that snapshot are not written; a file error) */
int shud_mon_flush(shud_mon_t m);
/* seconds the writer thread has spent formatting and writing so far (waits for the writer) */
double shud_mon_writer_seconds(shud_mon_t m);
/* flushes, closes the files, frees the buffers; returns the writer's first failure, if any */
int shud_mon_destroy(shud_mon_t m);
/* measurement helper like shud_wb_time_samples: `reps` flood passes (count, scan, scatter and the copy of the
 * count word) timed with HIP events; nothing is written */
int shud_mon_time_flood(shud_mon_t m, int reps, double *ms_pass);

/* ---- device-free formatters (shud_mon_fmt.cpp: what the writer thread calls; also the host path for values that
 * never were on the device, e.g. <prj>.cfg.ic.bak from LoadIC's arrays) ---- */
/* PrintInit's file without the schedule test, through <path>.tmp + rename; lake may be NULL when n_lake == 0 */
int shud_mon_write_ic_host(const char *path, double t, int32_t n_ele, int32_t n_riv, int32_t n_lake,
                           const double *is, const double *snow, const double *surf, const double *unsat,
                           const double *gw, const double *riv, const double *lake);
/* the header line of <prj>.flood.csv */
const char *shud_mon_flood_header(void);
/* FloodWarning's rows for n packed records: record k is reach idx[k] (0-based; NULL = k) with stage[k] and q[k];
 * type and depth are per-reach arrays looked up by the reach index.  Writes at most cap bytes (NUL-terminated when
 * cap > 0) into buf and returns the length of the full text, so (NULL, 0) sizes a buffer. */
int64_t shud_mon_format_flood_rows(char *buf, int64_t cap, double t, const int32_t *idx, const int32_t *type,
                                   const double *stage, const double *depth, const double *q, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* SHUD_MON_H */
