// shud_mon_fmt.cpp — device-free formatters of the run monitors (include/shud_mon.h): the bytes of
// <prj>.flood.csv (FloodAlert::InitFile / FloodWarning, src/classes/FloodAlert.cpp:62-87) and of
// <prj>.cfg.ic.update / .cfg.ic.bak (Model_Data::PrintInit, src/ModelData/MD_update.cpp:268-299).  Plain C++
// (no HIP include): links into libshud_rhs.so, where the writer thread of shud_mon.hip calls it, and compiles
// into a stand-alone host program.  The format strings are the reference's, character for character.
#include "shud_mon_fmt.h"

#include <string>

#include "shud_mon.h"

static const char kFloodHeader[] = "time\tID\tType\tStage_m\tBank_m\tDischarge_m3/day\n";
#define FLOOD_ROW "%.1f\t%d\t%d\t%f\t%f\t%f\n"

int shud_mon_fmt_flood_file(FILE *fp, double t, const ShudFloodRec *rec, int64_t n, const int32_t *type,
                            const double *depth) {
    for (int64_t k = 0; k < n; k++) {
        const int32_t i = rec[k].idx;
        if (fprintf(fp, FLOOD_ROW, t, i + 1, type[i], rec[k].stage, depth[i], rec[k].qdown) < 0) return SHUD_MON_ERR_IO;
    }
    return ferror(fp) ? SHUD_MON_ERR_IO : 0;
}

int shud_mon_fmt_write_ic(const char *path, double t, int32_t n_ele, int32_t n_riv, int32_t n_lake,
                          const double *const col[5], int stride, const double *riv, const double *lake) {
    const std::string tmp = std::string(path) + ".tmp";
    FILE *fp = fopen(tmp.c_str(), "w");
    if (!fp) return SHUD_MON_ERR_IO;
    /************* Element status **************/
    fprintf(fp, "%d\t %d \t%lf\n", n_ele, 6, t);
    fprintf(fp, "%s\t%s\t%s\t%s\t%s\t%s\n", "Index", "Canopy", "Snow", "Surface", "Unsat", "GW");
    for (int32_t i = 0; i < n_ele; i++) {
        const size_t o = (size_t)i * stride;
        fprintf(fp, "%d\t%lf\t%lf\t%lf\t%lf\t%lf\n", i + 1, col[0][o], col[1][o], col[2][o], col[3][o], col[4][o]);
    }
    /************* River Reach status **************/
    fprintf(fp, "%d\t%d\n", n_riv, 2);
    fprintf(fp, "%s\t%s\n", "Index", "Stage");
    for (int32_t i = 0; i < n_riv; i++) fprintf(fp, "%d\t%lf\n", i + 1, riv[i]);
    /************* Lake status **************/
    if (n_lake > 0) {
        fprintf(fp, "%d\t%d\n", n_lake, 2);
        fprintf(fp, "%s\t%s\n", "Index", "LakeStage");
        for (int32_t i = 0; i < n_lake; i++) fprintf(fp, "%d\t%lf\n", i + 1, lake[i]);
    }
    const bool bad = ferror(fp) != 0;
    if (fclose(fp) != 0 || bad || rename(tmp.c_str(), path) != 0) {
        remove(tmp.c_str());
        return SHUD_MON_ERR_IO;
    }
    return 0;
}

extern "C" int shud_mon_write_ic_host(const char *path, double t, int32_t n_ele, int32_t n_riv, int32_t n_lake,
                                      const double *is, const double *snow, const double *surf, const double *unsat,
                                      const double *gw, const double *riv, const double *lake) {
    if (!path || n_ele < 0 || n_riv < 0 || n_lake < 0) return -2;                       // SHUD_ERR_ARG
    if ((n_ele > 0 && (!is || !snow || !surf || !unsat || !gw)) || (n_riv > 0 && !riv) || (n_lake > 0 && !lake))
        return -2;
    const double *const col[5] = {is, snow, surf, unsat, gw};
    return shud_mon_fmt_write_ic(path, t, n_ele, n_riv, n_lake, col, 1, riv, lake);
}

extern "C" const char *shud_mon_flood_header(void) { return kFloodHeader; }

extern "C" int64_t shud_mon_format_flood_rows(char *buf, int64_t cap, double t, const int32_t *idx,
                                              const int32_t *type, const double *stage, const double *depth,
                                              const double *q, int64_t n) {
    if (n < 0 || cap < 0 || (n > 0 && (!type || !stage || !depth || !q))) return -2;
    int64_t len = 0;
    if (buf && cap > 0) buf[0] = '\0';
    for (int64_t k = 0; k < n; k++) {
        const int64_t i = idx ? idx[k] : k;
        const bool room = buf && len < cap;
        const int w = snprintf(room ? buf + len : nullptr, room ? (size_t)(cap - len) : 0, FLOOD_ROW, t, (int)(i + 1),
                               type[i], stage[k], depth[i], q[k]);
        if (w < 0) return SHUD_MON_ERR_IO;
        len += w;
    }
    return len;
}
