// shud_nc.cpp — device-free writer of the NetCDF outputs (include/shud_nc.h): the files of NetcdfElementFile and
// NetcdfSimpleFile (src/classes/NetcdfOutputContext.cpp:314-951) and the record slabs of their sinks (:953-1085), in
// the classic 64-bit-offset container ("CDF\x02") written by hand.  Plain C++ (no HIP include): links into
// libshud_rhs.so, where the writer threads of shud_out.hip call it, and compiles into a stand-alone host program.
//
// Layout (NetCDF classic format specification):
//   header  = "CDF\2" numrecs dim_list gatt_list var_list         every integer big-endian, names / values padded to 4
//   var     = name ndims dimid.. vatt_list nc_type vsize(4) begin(8)
//   data    = the fixed variables in definition order from the end of the header, then the records; a record is the
//             slab of every record variable in definition order (time, then one float slab per data variable)
// Definition order is the reference's own (openIfNeeded, then ensureVar per registered control).
#include "shud_nc.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "shud_rhs.h"

namespace {

thread_local std::string g_nc_err;
int nc_fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_nc_err = buf;
    return code;
}

enum { NC_CHAR = 2, NC_INT = 4, NC_FLOAT = 5, NC_DOUBLE = 6, NC_DIMENSION = 10, NC_VARIABLE = 11, NC_ATTRIBUTE = 12 };
constexpr uint32_t kFillInt = 0x80000001u;       // NC_FILL_INT (-2147483647): what an unwritten int variable holds
constexpr uint64_t kLimit = 1ull << 32;          // a vsize field is 4 bytes

struct Bytes {
    std::string b;
    void u32(uint32_t v) {
        const char c[4] = {(char)(v >> 24), (char)(v >> 16), (char)(v >> 8), (char)v};
        b.append(c, 4);
    }
    void u64(uint64_t v) { u32((uint32_t)(v >> 32)); u32((uint32_t)v); }
    void f64(double d) { uint64_t v; memcpy(&v, &d, 8); u64(v); }
    // arrays: one resize, then swapped words stored in place (the fixed variables of a large mesh are tens of MB)
    void i32s(const int32_t *v, size_t n) {
        const size_t o = b.size();
        b.resize(o + 4 * n);
        for (size_t i = 0; i < n; i++) {
            const uint32_t w = __builtin_bswap32((uint32_t)v[i]);
            memcpy(&b[o + 4 * i], &w, 4);
        }
    }
    void f64s(const double *v, size_t n) {
        const size_t o = b.size();
        b.resize(o + 8 * n);
        for (size_t i = 0; i < n; i++) {
            uint64_t w;
            memcpy(&w, &v[i], 8);
            w = __builtin_bswap64(w);
            memcpy(&b[o + 8 * i], &w, 8);
        }
    }
    void padded(const std::string &s) { b += s; b.append((4 - s.size() % 4) % 4, '\0'); }
    void name(const std::string &s) { u32((uint32_t)s.size()); padded(s); }
};

struct Att {
    std::string name;
    int type;                 // NC_CHAR: text; NC_INT / NC_FLOAT: one value in `word`
    std::string text;
    uint32_t word;
};
Att att_text(const char *n, const std::string &v) { return Att{n, NC_CHAR, v, 0}; }
Att att_int(const char *n, int32_t v) { return Att{n, NC_INT, "", (uint32_t)v}; }
Att att_fill() { return Att{"_FillValue", NC_FLOAT, "", SHUD_NC_FILL_BITS}; }

struct Var {
    std::string name;
    std::vector<int> dims;
    std::vector<Att> atts;
    int type;
    bool record;
    uint64_t vsize, begin;
};

void put_atts(Bytes &h, const std::vector<Att> &a) {
    if (a.empty()) { h.u32(0); h.u32(0); return; }
    h.u32(NC_ATTRIBUTE);
    h.u32((uint32_t)a.size());
    for (const Att &x : a) {
        h.name(x.name);
        h.u32((uint32_t)x.type);
        if (x.type == NC_CHAR) { h.u32((uint32_t)x.text.size()); h.padded(x.text); }
        else { h.u32(1); h.u32(x.word); }
    }
}

// lookupVarMeta (NetcdfOutputContext.cpp:200-265)
struct Meta { const char *name, *units, *long_name; };
const Meta kMeta[] = {
    {"eleyic", "m", "interception storage"}, {"eleysnow", "m", "snow depth"}, {"eleysurf", "m", "surface water depth"},
    {"eleyunsat", "m", "unsaturated zone storage depth"}, {"eleygw", "m", "groundwater head"},
    {"elevprcp", "m/day", "precipitation to land"}, {"elevnetprcp", "m/day", "net precipitation"},
    {"elevetp", "m/day", "potential evapotranspiration"}, {"eleveta", "m/day", "actual evapotranspiration"},
    {"elevrech", "m/day", "recharge"}, {"elevinfil", "m/day", "infiltration"}, {"elevexfil", "m/day", "exfiltration"},
    {"elevetic", "m/day", "evapotranspiration: interception"}, {"elevettr", "m/day", "evapotranspiration: transpiration"},
    {"elevetev", "m/day", "evapotranspiration: evaporation"},
    {"eleqrsurf", "m3/day", "element to river surface flow"}, {"eleqrsub", "m3/day", "element to river subsurface flow"},
    {"eleqsub", "m3/day", "subsurface flow: total"}, {"eleqsub1", "m3/day", "subsurface flow: direction 1"},
    {"eleqsub2", "m3/day", "subsurface flow: direction 2"}, {"eleqsub3", "m3/day", "subsurface flow: direction 3"},
    {"eleqsurf", "m3/day", "surface flow: total"}, {"eleqsurf1", "m3/day", "surface flow: direction 1"},
    {"eleqsurf2", "m3/day", "surface flow: direction 2"}, {"eleqsurf3", "m3/day", "surface flow: direction 3"},
    {"rivqdown", "m3/day", "river downstream discharge"}, {"rivqup", "m3/day", "river upstream discharge"},
    {"rivqsurf", "m3/day", "river surface discharge"}, {"rivqsub", "m3/day", "river subsurface discharge"},
    {"rivystage", "m", "river stage"},
    {"lakystage", "m", "lake stage"}, {"lakatop", "m2", "lake top area"}, {"lakvevap", "m/day", "lake evaporation"},
    {"lakvprcp", "m/day", "lake precipitation"}, {"lakqrivin", "m3/day", "lake river inflow"},
    {"lakqrivout", "m3/day", "lake river outflow"}, {"lakqsurf", "m3/day", "lake surface discharge"},
    {"lakqsub", "m3/day", "lake subsurface discharge"},
    {"rn_h", "W m-2", "shortwave radiation on horizontal surface"},
    {"rn_t", "W m-2", "terrain-corrected shortwave radiation"}, {"rn_factor", "1", "terrain radiation correction factor"},
};

std::string dirname_of(const std::string &p) {
    const size_t pos = p.find_last_of("/\\");
    if (pos == std::string::npos) return ".";
    if (pos == 0) return "/";
    return p.substr(0, pos);
}
std::string basename_of(const std::string &p) {
    const size_t pos = p.find_last_of("/\\");
    return pos == std::string::npos ? p : p.substr(pos + 1);
}
std::string join_path(const std::string &a, const std::string &b) {
    if (a.empty()) return b;
    if (b.empty()) return a;
    return a.back() == '/' ? a + b : a + "/" + b;
}
int mkdir_p(const std::string &d) {
    std::string cur;
    for (size_t i = 0; i <= d.size(); i++) {
        if ((i == d.size() || d[i] == '/') && !cur.empty()) mkdir(cur.c_str(), 0777);
        if (i < d.size()) cur += d[i];
    }
    struct stat st;
    return stat(d.c_str(), &st) == 0 && S_ISDIR(st.st_mode) ? 0 : -1;
}
std::string iso_date(int64_t ymd) {               // isoDateFromYYYYMMDD (:172-183)
    const int y = (int)(ymd / 10000), m = (int)((ymd / 100) % 100), d = (int)(ymd % 100);
    if (ymd <= 0 || m < 1 || m > 12 || d < 1 || d > 31) return "0000-00-00";
    char buf[32];
    snprintf(buf, sizeof buf, "%04d-%02d-%02d", y, m, d);
    return buf;
}
std::string now_utc() {                           // nowUtcIso8601 (:185-193)
    std::time_t t = std::time(nullptr);
    std::tm tm{};
    gmtime_r(&t, &tm);
    char buf[32];
    std::strftime(buf, sizeof buf, "%Y-%m-%dT%H:%M:%SZ", &tm);
    return buf;
}

int pwrite_all(int fd, const void *p, size_t n, uint64_t off) {
    const char *c = (const char *)p;
    while (n > 0) {
        const ssize_t w = pwrite(fd, c, n, (off_t)off);
        if (w < 0) {
            if (errno == EINTR) continue;
            return -1;
        }
        c += w;
        off += (uint64_t)w;
        n -= (size_t)w;
    }
    return 0;
}

inline uint32_t be32(uint32_t v) { return __builtin_bswap32(v); }
inline uint32_t f32_be(double d) {
    const float f = (float)d;                     // out[idx0] = (float)buffer[j] (:1000)
    uint32_t u;
    memcpy(&u, &f, 4);
    return be32(u);
}

struct Ctrl {
    int var;                                      // index into data variables
    std::vector<int32_t> icol;
};

}  // namespace

struct shud_nc {
    int kind = 0, n_all = 0, num_node = 0;
    int64_t forc_start = 0;
    std::string out_dir, crs_wkt, history, path, prefix;
    bool have_history = false;
    std::vector<double> node_x, node_y, face_x, face_y;
    std::vector<int32_t> face_nodes;
    std::vector<std::string> data_names;          // data variables, in definition order
    std::vector<Ctrl> ctrls;
    std::vector<int32_t> mask;                    // writeOutputMask: from the first registered control
    // file state
    int fd = -1;
    bool begun = false;
    uint64_t rec_begin = 0, rec_size = 0;
    std::mutex mu;                                // record creation and lookup
    std::map<long long, int64_t> time_to_idx;     // every reserved record
    std::vector<long long> times;                 // their times, by index (first appearance)
    int64_t numrecs = 0;                          // records in the file: created in index order
};

static const char *obj_dim(int kind) { return kind == SHUD_NC_RIV ? "river" : "lake"; }

// the whole header and the fixed variables' bytes; fills rec_begin / rec_size
static int build_image(shud_nc *nc, std::string *image) {
    const uint64_t n = (uint64_t)nc->n_all, nn = (uint64_t)nc->num_node;
    const bool ele = nc->kind == SHUD_NC_ELE;
    // dimensions: time (unlimited, id 0), then the object dimensions
    std::vector<std::pair<std::string, uint32_t>> dims;
    dims.push_back({"time", 0});
    if (ele) {
        dims.push_back({"mesh_face", (uint32_t)n});
        dims.push_back({"mesh_node", (uint32_t)nn});
        dims.push_back({"max_face_nodes", 3});
    } else {
        dims.push_back({obj_dim(nc->kind), (uint32_t)n});
    }
    std::vector<Var> vars;
    const std::string tunits = "minutes since " + iso_date(nc->forc_start) + " 00:00:00 UTC";
    vars.push_back({"time", {0}, {att_text("units", tunits), att_text("calendar", "standard")}, NC_DOUBLE, true, 8, 0});
    const bool crs = ele && !nc->crs_wkt.empty();
    if (ele) {
        const char *xn = "projection_x_coordinate", *yn = "projection_y_coordinate";
        vars.push_back({"mesh_node_x", {2}, {att_text("standard_name", xn), att_text("units", "m")}, NC_DOUBLE, false, 8 * nn, 0});
        vars.push_back({"mesh_node_y", {2}, {att_text("standard_name", yn), att_text("units", "m")}, NC_DOUBLE, false, 8 * nn, 0});
        vars.push_back({"mesh_face_nodes", {1, 3}, {att_int("start_index", 1)}, NC_INT, false, 12 * n, 0});
        vars.push_back({"mesh_face_x", {1}, {att_text("standard_name", xn), att_text("units", "m")}, NC_DOUBLE, false, 8 * n, 0});
        vars.push_back({"mesh_face_y", {1}, {att_text("standard_name", yn), att_text("units", "m")}, NC_DOUBLE, false, 8 * n, 0});
        if (crs)
            vars.push_back({"crs", {}, {att_text("long_name", "coordinate reference system"),
                                        att_text("spatial_ref", nc->crs_wkt), att_text("crs_wkt", nc->crs_wkt)},
                            NC_INT, false, 4, 0});
        vars.push_back({"mesh", {}, {att_text("cf_role", "mesh_topology"), att_int("topology_dimension", 2),
                                     att_text("node_coordinates", "mesh_node_x mesh_node_y"),
                                     att_text("face_node_connectivity", "mesh_face_nodes"),
                                     att_text("face_coordinates", "mesh_face_x mesh_face_y")},
                        NC_INT, false, 4, 0});
        vars.push_back({"element_id", {1}, {att_int("start_index", 1)}, NC_INT, false, 4 * n, 0});
        vars.push_back({"element_output_mask", {1}, {}, NC_INT, false, 4 * n, 0});
    } else {
        vars.push_back({std::string(obj_dim(nc->kind)) + "_id", {1}, {att_int("start_index", 1)}, NC_INT, false, 4 * n, 0});
        vars.push_back({std::string(obj_dim(nc->kind)) + "_output_mask", {1}, {}, NC_INT, false, 4 * n, 0});
    }
    for (const std::string &name : nc->data_names) {          // ensureVar (:570-613, :833-858)
        Var v{name, {0, 1}, {att_fill()}, NC_FLOAT, true, 4 * n, 0};
        if (ele) {
            v.atts.push_back(att_text("mesh", "mesh"));
            v.atts.push_back(att_text("location", "face"));
            v.atts.push_back(att_text("coordinates", "mesh_face_x mesh_face_y"));
            if (crs) v.atts.push_back(att_text("grid_mapping", "crs"));
        }
        const Meta *m = nullptr;                               // applyVarMetadata (:267-282)
        for (const Meta &k : kMeta)
            if (name == k.name) m = &k;
        v.atts.push_back(att_text("long_name", m ? std::string(m->long_name) : "SHUD output variable: " + name));
        if (m && m->units[0]) v.atts.push_back(att_text("units", m->units));
        vars.push_back(v);
    }
    const std::vector<Att> gatts = {
        att_text("Conventions", ele ? "CF-1.10 UGRID-1.0" : "CF-1.10"), att_text("title", "SHUD output: " + nc->prefix),
        att_text("source", "SHUD"),
        att_text("history", nc->have_history ? nc->history : now_utc() + ": created by SHUD")};
    // two passes: the header's length does not depend on the offsets it holds
    std::string hdr;
    for (int pass = 0; pass < 2; pass++) {
        Bytes h;
        h.b = "CDF\x02";
        h.u32(0);                                             // numrecs
        h.u32(NC_DIMENSION);
        h.u32((uint32_t)dims.size());
        for (auto &d : dims) { h.name(d.first); h.u32(d.second); }
        put_atts(h, gatts);
        h.u32(NC_VARIABLE);
        h.u32((uint32_t)vars.size());
        for (const Var &v : vars) {
            h.name(v.name);
            h.u32((uint32_t)v.dims.size());
            for (int d : v.dims) h.u32((uint32_t)d);
            put_atts(h, v.atts);
            h.u32((uint32_t)v.type);
            h.u32((uint32_t)v.vsize);
            h.u64(v.begin);
        }
        if (pass == 0) {
            uint64_t off = h.b.size();
            for (Var &v : vars)
                if (!v.record) { v.begin = off; off += v.vsize; }
            nc->rec_begin = off;
            nc->rec_size = 0;
            for (Var &v : vars)
                if (v.record) { v.begin = off; off += v.vsize; nc->rec_size += v.vsize; }
        }
        hdr.swap(h.b);
    }
    // fixed variables
    Bytes d;
    d.b.swap(hdr);
    d.b.reserve((size_t)nc->rec_begin);
    if (ele) {
        d.f64s(nc->node_x.data(), nn);
        d.f64s(nc->node_y.data(), nn);
        d.i32s(nc->face_nodes.data(), 3 * n);
        d.f64s(nc->face_x.data(), n);
        d.f64s(nc->face_y.data(), n);
        if (crs) d.u32(kFillInt);
        d.u32(kFillInt);
    }
    {
        std::vector<int32_t> ids(n);
        for (uint64_t i = 0; i < n; i++) ids[i] = (int32_t)(i + 1);
        d.i32s(ids.data(), n);
    }
    d.i32s(nc->mask.data(), n);
    if (d.b.size() != nc->rec_begin) return nc_fail(SHUD_ERR_ARG, "%s: internal layout error", nc->path.c_str());
    image->swap(d.b);
    return SHUD_OK;
}

extern "C" const char *shud_nc_last_error(void) { return g_nc_err.c_str(); }

extern "C" int shud_nc_create(const ShudNcSpec *s, shud_nc_t *out) {
    if (!s || !out) return nc_fail(SHUD_ERR_ARG, "shud_nc_create: null argument");
    *out = nullptr;
    if (s->kind < 0 || s->kind >= SHUD_NC_KINDS) return nc_fail(SHUD_ERR_ARG, "shud_nc_create: unknown kind %d", s->kind);
    if (s->kind == SHUD_NC_ELE ? s->n_all < 0 : s->n_all <= 0)     // NetcdfSimpleFile::openIfNeeded (:749-753)
        return nc_fail(SHUD_ERR_ARG, "Invalid output dimension for NetCDF output (%s): n_all %d",
                       s->kind == SHUD_NC_ELE ? "mesh_face" : obj_dim(s->kind), s->n_all);
    const uint64_t n64 = (uint64_t)s->n_all, nn64 = (uint64_t)(s->num_node > 0 ? s->num_node : 0);
    if (4 * n64 >= kLimit)
        return nc_fail(SHUD_ERR_ARG, "NetCDF output: a record slab of %llu values is 4 GiB or more: the classic "
                       "64-bit-offset format cannot hold it", (unsigned long long)n64);
    if (s->kind == SHUD_NC_ELE && (12 * n64 >= kLimit || 8 * nn64 >= kLimit))
        return nc_fail(SHUD_ERR_ARG, "NetCDF output: a mesh variable (%llu faces, %llu nodes) is 4 GiB or more: the "
                       "classic 64-bit-offset format cannot hold it", (unsigned long long)n64, (unsigned long long)nn64);
    shud_nc *nc = new shud_nc;
    nc->kind = s->kind;
    nc->n_all = s->n_all;
    nc->forc_start = s->forc_start_time;
    if (s->out_dir) nc->out_dir = s->out_dir;
    if (s->history) { nc->history = s->history; nc->have_history = true; }
    if (s->kind == SHUD_NC_ELE) {
        const size_t n = (size_t)s->n_all, nn = (size_t)(s->num_node > 0 ? s->num_node : 0);
        if ((nn && (!s->node_x || !s->node_y)) || (n && (!s->face_nodes || !s->face_x || !s->face_y))) {
            delete nc;
            return nc_fail(SHUD_ERR_ARG, "mesh nodes / elements are not available for NetCDF output");
        }
        for (size_t i = 0; i < 3 * n; i++)
            if (s->face_nodes[i] < 1 || (size_t)s->face_nodes[i] > nn) {
                delete nc;
                return nc_fail(SHUD_ERR_ARG, "invalid element node index %d (NumNode=%zu)", s->face_nodes[i], nn);
            }
        if (s->crs_wkt) nc->crs_wkt = s->crs_wkt;
        nc->num_node = (int)nn;
        nc->node_x.assign(s->node_x, s->node_x + nn);
        nc->node_y.assign(s->node_y, s->node_y + nn);
        nc->face_nodes.assign(s->face_nodes, s->face_nodes + 3 * n);
        nc->face_x.assign(s->face_x, s->face_x + n);
        nc->face_y.assign(s->face_y, s->face_y + n);
    }
    *out = nc;
    return SHUD_OK;
}

extern "C" int shud_nc_add_var(shud_nc_t nc, const char *basename, int32_t n_all, int64_t forc_start,
                               const int32_t *icol, int32_t nsel, int32_t *ctrl) {
    if (!nc || !basename || !basename[0] || nsel < 0 || (nsel > 0 && !icol))
        return nc_fail(SHUD_ERR_ARG, "shud_nc_add_var: null / empty argument");
    std::lock_guard<std::mutex> lk(nc->mu);
    if (nc->begun || !nc->times.empty())
        return nc_fail(SHUD_ERR_ARG, "%s: a variable cannot be registered after the first record (the classic header "
                       "cannot grow once data follows it)", nc->path.c_str());
    if (n_all != nc->n_all || forc_start != nc->forc_start)       // openIfNeeded (:337-353, :739-746)
        return nc_fail(SHUD_ERR_ARG, "Inconsistent NetCDF output context for %s: file n_all=%d ForcStartTime=%lld, "
                       "control n_all=%d ForcStartTime=%lld", basename, nc->n_all, (long long)nc->forc_start, n_all,
                       (long long)forc_start);
    // deriveVarName / derivePrefixLeaf (:284-312)
    const std::string leaf = basename_of(basename);
    const size_t dot = leaf.find_last_of('.');
    if (dot == std::string::npos || dot == 0 || dot + 1 >= leaf.size())
        return nc_fail(SHUD_ERR_ARG, "Cannot derive NetCDF prefix / variable name from legacy basename %s "
                       "(expected <prefix>.<varname>, e.g. qhh.eleygw)", basename);
    const std::string name = leaf.substr(dot + 1);
    if (nc->ctrls.empty()) {
        static const char *sfx[SHUD_NC_KINDS] = {".ele.nc", ".riv.nc", ".lake.nc"};
        nc->prefix = leaf.substr(0, dot);
        std::string dir = nc->out_dir.empty() ? dirname_of(basename) : nc->out_dir;
        if (dir.empty()) dir = ".";
        nc->out_dir = dir;
        nc->path = join_path(dir, nc->prefix + sfx[nc->kind]);
        nc->mask.assign((size_t)nc->n_all, 0);                    // writeOutputMask (:615-638)
        for (int32_t j = 0; j < nsel; j++)
            if (icol[j] >= 1 && icol[j] <= nc->n_all) nc->mask[(size_t)icol[j] - 1] = 1;
    }
    int var = -1;
    for (size_t k = 0; k < nc->data_names.size(); k++)
        if (nc->data_names[k] == name) var = (int)k;
    if (var < 0) {
        var = (int)nc->data_names.size();
        nc->data_names.push_back(name);
    }
    nc->ctrls.push_back(Ctrl{var, std::vector<int32_t>(icol, icol + nsel)});
    if (ctrl) *ctrl = (int32_t)nc->ctrls.size() - 1;
    return SHUD_OK;
}

static int begin_locked(shud_nc *nc) {
    if (nc->begun) return SHUD_OK;
    if (nc->ctrls.empty()) return nc_fail(SHUD_ERR_ARG, "shud_nc_begin: no variable registered");
    std::string image;
    int rc = build_image(nc, &image);
    if (rc) return rc;
    if (mkdir_p(nc->out_dir))
        return nc_fail(SHUD_ERR_ARG, "NetCDF output: cannot create the directory %s for %s (%s)", nc->out_dir.c_str(),
                       nc->path.c_str(), strerror(errno));
    nc->fd = open(nc->path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (nc->fd < 0) return nc_fail(SHUD_ERR_ARG, "NetCDF output: cannot create %s (%s)", nc->path.c_str(), strerror(errno));
    if (pwrite_all(nc->fd, image.data(), image.size(), 0)) {
        close(nc->fd);
        nc->fd = -1;
        return nc_fail(SHUD_ERR_ARG, "NetCDF output: write error on %s (%s)", nc->path.c_str(), strerror(errno));
    }
    nc->begun = true;
    return SHUD_OK;
}

extern "C" int shud_nc_begin(shud_nc_t nc) {
    if (!nc) return nc_fail(SHUD_ERR_ARG, "shud_nc_begin: null argument");
    std::lock_guard<std::mutex> lk(nc->mu);
    return begin_locked(nc);
}

// index of llround(tq) in first-appearance order (no I/O)
static int reserve_locked(shud_nc *nc, double tq, int64_t *rec) {
    const long long t_min = (long long)llround(tq);
    const auto it = nc->time_to_idx.find(t_min);
    if (it != nc->time_to_idx.end()) {
        *rec = it->second;
        return SHUD_OK;
    }
    if (nc->ctrls.empty()) return nc_fail(SHUD_ERR_ARG, "shud_nc_record: no variable registered");
    const int64_t idx = (int64_t)nc->times.size();
    if (idx + 1 >= (int64_t)0x7fffffffll) return nc_fail(SHUD_ERR_ARG, "%s: too many records", nc->path.c_str());
    nc->times.push_back(t_min);
    nc->time_to_idx[t_min] = idx;
    *rec = idx;
    return SHUD_OK;
}

extern "C" int shud_nc_reserve(shud_nc_t nc, double tq, int64_t *rec) {
    if (!nc || !rec) return nc_fail(SHUD_ERR_ARG, "shud_nc_reserve: null argument");
    std::lock_guard<std::mutex> lk(nc->mu);
    return reserve_locked(nc, tq, rec);
}

extern "C" int shud_nc_record(shud_nc_t nc, double tq, int64_t *rec) {
    if (!nc || !rec) return nc_fail(SHUD_ERR_ARG, "shud_nc_record: null argument");
    std::lock_guard<std::mutex> lk(nc->mu);
    int rc = reserve_locked(nc, tq, rec);
    if (!rc) rc = begin_locked(nc);
    if (rc) return rc;
    // records are created in index order: a record's time, a fill slab for every data variable, then numrecs
    while (nc->numrecs <= *rec) {
        const int64_t idx = nc->numrecs;
        const uint64_t base = nc->rec_begin + (uint64_t)idx * nc->rec_size;
        Bytes tv;
        tv.f64((double)nc->times[(size_t)idx]);
        bool bad = pwrite_all(nc->fd, tv.b.data(), 8, base) != 0;
        const uint64_t nfill = nc->rec_size - 8;
        const size_t chunk = (size_t)std::min<uint64_t>(nfill, 1u << 20);
        std::vector<uint32_t> fill(chunk / 4, be32(SHUD_NC_FILL_BITS));
        for (uint64_t o = 0; o < nfill && !bad; o += chunk)
            bad = pwrite_all(nc->fd, fill.data(), (size_t)std::min<uint64_t>(chunk, nfill - o), base + 8 + o) != 0;
        Bytes nr;
        nr.u32((uint32_t)(idx + 1));
        bad = bad || pwrite_all(nc->fd, nr.b.data(), 4, 4) != 0;
        if (bad) return nc_fail(SHUD_ERR_ARG, "NetCDF output: write error on %s (%s)", nc->path.c_str(), strerror(errno));
        nc->numrecs = idx + 1;
    }
    return SHUD_OK;
}

extern "C" int shud_nc_put_slab(shud_nc_t nc, int32_t ctrl, int64_t rec, const void *be_words) {
    if (!nc || !be_words || ctrl < 0 || ctrl >= (int32_t)nc->ctrls.size())
        return nc_fail(SHUD_ERR_ARG, "shud_nc_put_slab: bad argument");
    uint64_t off;
    {
        std::lock_guard<std::mutex> lk(nc->mu);
        if (!nc->begun || rec < 0 || rec >= nc->numrecs)
            return nc_fail(SHUD_ERR_ARG, "shud_nc_put_slab: record %lld does not exist", (long long)rec);
        off = nc->rec_begin + (uint64_t)rec * nc->rec_size + 8 + (uint64_t)nc->ctrls[ctrl].var * 4 * (uint64_t)nc->n_all;
    }
    if (pwrite_all(nc->fd, be_words, 4 * (size_t)nc->n_all, off))
        return nc_fail(SHUD_ERR_ARG, "NetCDF output: write error on %s (%s)", nc->path.c_str(), strerror(errno));
    return SHUD_OK;
}

extern "C" int shud_nc_convert(const double *sel, int32_t nsel, const int32_t *icol, int32_t n_icol, int32_t n_all,
                               uint32_t *slab) {
    if (!slab || n_all < 0 || nsel < 0 || n_icol < 0 || (nsel > 0 && n_icol > 0 && (!sel || !icol)))
        return nc_fail(SHUD_ERR_ARG, "shud_nc_convert: bad argument");
    const uint32_t fill = be32(SHUD_NC_FILL_BITS);
    for (int32_t i = 0; i < n_all; i++) slab[i] = fill;           // std::vector<float> out(n_all, fill_value_)
    const int32_t n = nsel < n_icol ? nsel : n_icol;
    for (int32_t j = 0; j < n; j++) {
        const int64_t idx0 = (int64_t)icol[j] - 1;
        if (idx0 < 0 || idx0 >= n_all) continue;
        slab[idx0] = f32_be(sel[j]);
    }
    return SHUD_OK;
}

extern "C" int shud_nc_put(shud_nc_t nc, int32_t ctrl, double tq, const double *sel, int32_t nsel) {
    if (!nc || ctrl < 0 || ctrl >= (int32_t)nc->ctrls.size()) return nc_fail(SHUD_ERR_ARG, "shud_nc_put: bad argument");
    const Ctrl &c = nc->ctrls[ctrl];
    std::vector<uint32_t> slab((size_t)nc->n_all);
    int rc = shud_nc_convert(sel, nsel, c.icol.data(), (int32_t)c.icol.size(), nc->n_all, slab.data());
    int64_t rec = 0;
    if (!rc) rc = shud_nc_record(nc, tq, &rec);
    if (!rc) rc = shud_nc_put_slab(nc, ctrl, rec, slab.data());
    return rc;
}

extern "C" int32_t shud_nc_num_ctrl(shud_nc_t nc) { return nc ? (int32_t)nc->ctrls.size() : -1; }
extern "C" int32_t shud_nc_ctrl_var(shud_nc_t nc, int32_t ctrl) {
    return nc && ctrl >= 0 && ctrl < (int32_t)nc->ctrls.size() ? nc->ctrls[ctrl].var : -1;
}
extern "C" int64_t shud_nc_num_records(shud_nc_t nc) {
    if (!nc) return -1;
    std::lock_guard<std::mutex> lk(nc->mu);
    return nc->numrecs;
}
extern "C" const char *shud_nc_path(shud_nc_t nc) { return nc ? nc->path.c_str() : ""; }

extern "C" int shud_nc_close(shud_nc_t nc) {
    if (!nc) return SHUD_OK;
    int rc = SHUD_OK;
    if (!nc->ctrls.empty()) rc = shud_nc_begin(nc);
    if (nc->fd >= 0 && close(nc->fd) != 0 && !rc)
        rc = nc_fail(SHUD_ERR_ARG, "NetCDF output: close error on %s (%s)", nc->path.c_str(), strerror(errno));
    delete nc;
    return rc;
}
