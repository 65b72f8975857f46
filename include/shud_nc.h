/* shud_nc.h — C-ABI of the classic-NetCDF writer behind OUTPUT_MODE NETCDF / BOTH (device-free; exported from
 * libshud_rhs.so, where the writer threads of the output path call it, and usable from plain host code).
 *
 * Restates, without libnetcdf, the files of
 *   NetcdfElementFile   src/classes/NetcdfOutputContext.cpp:314-718   <out_dir>/<prefix>.ele.nc  (UGRID mesh)
 *   NetcdfSimpleFile    src/classes/NetcdfOutputContext.cpp:720-951   <prefix>.riv.nc / <prefix>.lake.nc
 *   Netcdf*VarSink      src/classes/NetcdfOutputContext.cpp:953-1085  (mask, variable, record slab)
 * with the same dimensions, variables, types and attributes.  The container differs: the reference creates
 * NetCDF-4 classic-model files (HDF5); this writer emits the classic 64-bit-offset format (magic "CDF\x02"), which
 * holds the classic data model in full and which every netCDF library reads.
 *
 * The classic header cannot grow once data follows it: every variable of a file is registered before the first
 * record, and registration after that is SHUD_ERR_ARG.  A file is a valid NetCDF after every put.
 * Errors: a negative SHUD_ERR_* code (include/shud_rhs.h), message in shud_nc_last_error() (per thread).
 */
#ifndef SHUD_NC_H
#define SHUD_NC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SHUD_NC_ELE = 0, SHUD_NC_RIV = 1, SHUD_NC_LAKE = 2, SHUD_NC_KINDS = 3 };

/* _FillValue of every data variable (9.96921e36f, NetcdfOutputContext.cpp:688), as its IEEE bits */
#define SHUD_NC_FILL_BITS 0x7cf00000u

typedef struct shud_nc *shud_nc_t;

typedef struct {
    int32_t kind;                /* SHUD_NC_ELE / _RIV / _LAKE                                               */
    int32_t n_all;               /* mesh_face / river / lake dimension (every control must have this NumAll)  */
    const char *out_dir;         /* OUT_DIR of the ncoutput cfg; NULL or "" = directory of the first basename */
    int64_t forc_start_time;     /* ForcStartTime yyyymmdd: "minutes since YYYY-MM-DD 00:00:00 UTC"           */
    const char *history;         /* whole `history` attribute; NULL = "<UTC now>: created by SHUD"            */
    /* element file only (ignored otherwise) */
    const char *crs_wkt;         /* text of the CRS_WKT file; NULL or "" = no crs variable                    */
    int32_t num_node;            /* mesh_node                                                                 */
    const double *node_x, *node_y;   /* [num_node], by node index                                             */
    const int32_t *face_nodes;   /* [n_all][3], 1-based node indices as in .sp.mesh                           */
    const double *face_x, *face_y;   /* [n_all] element centroids                                             */
} ShudNcSpec;

/* a file description; nothing touches the disk yet.  The mesh arrays are copied.  Refuses what the format cannot
 * hold: a fixed variable or a record slab of 4 GiB or more. */
int shud_nc_create(const ShudNcSpec *spec, shud_nc_t *out);
/* Netcdf*VarSink::onInit: registers the control `basename` (= <dir>/<prefix>.<varname>) with its selected columns
 * icol (1-based, nsel entries; entries outside [1, n_all] are kept and skipped by every put, :996-999).  The first
 * registration fixes the file's path and its output mask.  Two controls with the same derived variable name share
 * one variable (ensureVar).  *ctrl receives the control's id (0.. in registration order).  SHUD_ERR_ARG after the
 * first record. */
int shud_nc_add_var(shud_nc_t nc, const char *basename, int32_t n_all, int64_t forc_start_time, const int32_t *icol,
                    int32_t nsel, int32_t *ctrl);
/* creates out_dir and the file and writes the header and the fixed variables (idempotent; implied by the first
 * record and by close) */
int shud_nc_begin(shud_nc_t nc);
/* ensureTimeIndex: the record of llround(t_quantized); a new time takes the next index (first appearance).  The
 * record and every reserved one before it are created in index order (a record's time value, a fill slab for every
 * data variable, then numrecs in the header); creation and lookup run under the file's lock */
int shud_nc_record(shud_nc_t nc, double t_quantized, int64_t *rec);
/* the index part of shud_nc_record alone (no I/O): lets one thread fix the record order while others write */
int shud_nc_reserve(shud_nc_t nc, double t_quantized, int64_t *rec);
/* one positioned write of control `ctrl`'s finished slab into an existing record: n_all big-endian float words
 * (fill at unselected positions) */
int shud_nc_put_slab(shud_nc_t nc, int32_t ctrl, int64_t rec, const void *be_words);
/* Netcdf*VarSink::onWrite on the host: the selected doubles of control `ctrl` are converted (float), stored
 * big-endian at icol[j] - 1, the rest fill; then record + slab */
int shud_nc_put(shud_nc_t nc, int32_t ctrl, double t_quantized, const double *selected, int32_t nsel);
/* the conversion of shud_nc_put alone: slab[n_all] words as they go to disk */
int shud_nc_convert(const double *selected, int32_t nsel, const int32_t *icol, int32_t n_icol, int32_t n_all,
                    uint32_t *slab);
int32_t shud_nc_num_ctrl(shud_nc_t nc);
/* index of the data variable control `ctrl` writes (definition order; shared names share one) */
int32_t shud_nc_ctrl_var(shud_nc_t nc, int32_t ctrl);
int64_t shud_nc_num_records(shud_nc_t nc);
/* the file's path ("" before the first registration) */
const char *shud_nc_path(shud_nc_t nc);
/* writes the header if no record ever did (a valid file with 0 records), closes and frees.  A description with
 * no registered control leaves no file, as the reference opens a file in its first sink's onInit. */
int shud_nc_close(shud_nc_t nc);
const char *shud_nc_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SHUD_NC_H */
