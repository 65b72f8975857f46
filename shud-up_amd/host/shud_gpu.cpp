// shud_gpu.cpp — C++ host of the device path: SHUD() (src/Model/shud.cpp:32-170) with the RHS, the ET-step
// prelude, the integrator and the outputs on one MI355X, driven through the C-ABIs of include/.
//
//   shud_gpu [-o outdir] [-e end_day] [-n num_steps] [-C cwd] [-q] [--flood] [--ic-snapshots] [--reorder bfs|tiles]
//            [--checkpoint PATH [--checkpoint-every N]] [--resume PATH] [--zones FILE] <input_dir> <project>
//   shud_gpu --rhs-check K | --rhs-bench [--evals N] ...   partitioned RHS modes (shud_gpu_part.cpp)
//
// input_dir/<project>.* are the reference's input files (FileIn, IO.cpp:53-91); forcing csv paths in
// <project>.tsd.forc resolve against -C (default: the process cwd, as the reference runs from its repository
// root), then against input_dir.  Outputs: <outdir>/<project>.<suffix>.dat in Print_Ctrl's byte layout
// (default outdir: output/<project>.out, IO.cpp:54).  Exit codes: 0, or the reference's myexit codes for
// physics errors (10/13) and 1 for input / solver / device errors.
//
// The loop below is shud.cpp:86-140 line by line:
//   for i < NumSteps:  tnext += SolverStep
//     while t + ZERO < tnext:  tout = ET sub-step ? min(t + ETStep, tnext) : tnext
//        updateAllTimeSeries(t); updateforcing(t); ET(t, tout)   -> shud_project_forcing + shud_et_step
//        [CVodeSetStopTime(tout)]; CVode(mem, tout, udata, &t, CV_NORMAL)  -> shud_ode_solve (y in HBM)
//     summary(udata); ExportResults(t)   -> shud_rhs_summary + shud_rhs_refresh_diagnostics + shud_out_export
// With SHUD_WB_DIAG set (env_truthy, WaterBalanceDiag.cpp:21-36, after shud.cpp:72's test) the water-balance
// diagnostics of shud.cpp:70-75,110-112,137-152 run on the device (include/shud_wb.h): onETUpdate after every ET
// step; after summary the extra, stateful f() on the accepted state, CVodeGetDky(k = 1), sample and maybeWrite,
// then ExportResults.  SHUD_WB_DIAG_TRAPZ selects the trapezoid rule.  SHUD_WB_DIAG_QUAD (read only when
// SHUD_WB_DIAG is on) runs the monitor of shud.cpp:113-135: the stop time is always set and the integrator goes to
// tout one internal step at a time (CV_ONE_STEP), each followed by a stateful f() on the returned state, its flux
// arrays and shud_wb_quad_step; <prj>.basinwbfull_quad.dat is written beside basinwbfull.dat.  These f() calls move
// the carried state, so the trajectory differs from a run without QUAD, as in the reference.  Without
// SHUD_WB_DIAG the loop makes exactly the calls it made before, and without SHUD_WB_DIAG_QUAD exactly those of
// SHUD_WB_DIAG alone.
// --flood and --ic-snapshots run the reference's run monitors on the device (include/shud_mon.h).  The reference
// always writes their files; here both are off by default, and without the flags the loop makes exactly the calls
// it made before.  --ic-snapshots: <prj>.cfg.ic.bak before the loop with header time 0 (shud.cpp:76),
// PrintInit(Init_update, t) at the top of every solver step (shud.cpp:97) and once after the loop (shud.cpp:157).
// The .bak file and any snapshot taken before the first step come from LoadIC's host arrays: the pre-loop
// shud_rhs_summary has already put boundary heads into the device arrays, which the reference's arrays do not hold
// at that point.  --flood: FloodWarning(t) after ExportResults (shud.cpp:154) on the arrays summary and the
// diagnostics replay have just filled, into <prj>.flood.csv.
// --reorder bfs | tiles runs the whole device side in a planned element order of include/shud_order.h (bfs: breadth-
// first; tiles: breadth-first pockets that stop at the borders of the 256-element sharing tile): the mesh, the
// parameters, the ET mesh and the initial state (y, IS, snow) are carried into it by the appliers and the handles are
// plain ones (the device ET prelude writes the step inputs straight into the handle, so the device side shares one
// numbering).  Every file stays in the input's numbering: element outputs are registered with shud_out_add_mapped,
// restart snapshots with shud_mon_set_ic_order, .cfg.ic.bak comes from the input's own arrays; flood alerts are
// per reach.  SHUD_WB_DIAG with --reorder is refused (its basin sums would run in another order), and so are lake
// models.  Without the flag the program makes exactly the calls it made before.
// OUTPUT_MODE NETCDF / BOTH of <prj>.cfg.para (with NCOUTPUT_CFG): the NetCDF outputs of MD_initialize.cpp:346-371 on the
// device (include/shud_out.h, include/shud_nc.h).  <prj>.ele.nc / .riv.nc / .lake.nc go to OUT_DIR of the ncoutput cfg,
// else beside the .dat files; every print control whose NumAll is NumEle gets an element sink, else NumRiv a river
// sink, else NumLake a lake sink (the reference's rule, in its order); NETCDF writes no .dat / .csv.  The files are in
// the classic 64-bit-offset container (the reference: NetCDF-4 classic model), same names, types and attributes.  The
// environment variable SHUD_NC_HISTORY replaces the whole `history` attribute ("<UTC now>: created by SHUD"), so that
// files are reproducible.  With --reorder the slab is built from the control's buffer, which is in the input's column
// order already.  A project without the key makes exactly the calls it made before.
// Not restated (out of the device path's scope): the screen print, NetCDF forcing, the uncoupled -g mode.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "shud_et.h"
#include "shud_gpu_util.hpp"
#include "shud_host.h"
#include "shud_ckpt.h"
#include "shud_mon.h"
#include "shud_ode.h"
#include "shud_order.h"
#include "shud_out.h"
#include "shud_rhs.h"
#include "shud_wb.h"

static constexpr double kZero = 1.0e-10;          // ZERO (Macros.hpp:32)

static void usage() {
    fprintf(stderr, "usage: shud_gpu [-o outdir] [-e end_day] [-n num_steps] [-C cwd] [-q] [--flood] [--ic-snapshots]\n"
                    "                [--reorder bfs|tiles] [--checkpoint PATH [--checkpoint-every N]] [--resume PATH]\n"
                    "                [--zones FILE] <input_dir> <project>\n"
                    "       shud_gpu --rhs-check K | --rhs-bench [--evals N] [-o outdir] [-C cwd] <input_dir> <project>\n"
                    "  --flood         write <outdir>/<project>.flood.csv (reaches above their bank after each solver step)\n"
                    "  --ic-snapshots  write <outdir>/<project>.cfg.ic.bak and, every Update_IC_STEP minutes and at the\n"
                    "                  end, <outdir>/<project>.cfg.ic.update (restart file for INIT_MODE 3)\n"
                    "  Both are off by default (the reference always writes these files).\n"
                    "  --checkpoint PATH  write an exact checkpoint of the device run to PATH at the end of the run and,\n"
                    "                  with --checkpoint-every N, after every N solver steps (the run goes on while it drains)\n"
                    "  --resume PATH   continue from a checkpoint into the same outdir: -n and -e count from the original\n"
                    "                  start, the files are cut back to the checkpoint and end up those of one straight run.\n"
                    "                  Neither with SHUD_WB_DIAG nor with OUTPUT_MODE NETCDF | BOTH.\n"
                    "  --zones FILE    a zone table (NumEle rows: index, zone; 0 = in no zone): every element output also gets\n"
                    "                  <outdir>/<project>.zone.<name> with one column per zone, reduced on the device at every\n"
                    "                  step: the zone's sum for eleq* (m3/day), the area-weighted mean for every other one.\n"
                    "                  Legacy files only: not with OUTPUT_MODE NETCDF.\n"
                    "  --reorder ORDER run the device side in a planned element order (neighbours close in memory);\n"
                    "                  every file stays in the input's element numbering.  Not with SHUD_WB_DIAG or lakes.\n"
                    "                  tiles: breadth-first pockets that each fill one 256-element sharing tile;\n"
                    "                  the faster one at every mesh size measured (prefer it).  bfs: plain breadth-first.\n"
                    "  OUTPUT_MODE NETCDF | BOTH with NCOUTPUT_CFG in <project>.cfg.para writes <project>.ele.nc, .riv.nc and\n"
                    "                  .lake.nc (classic 64-bit-offset NetCDF); the environment variable SHUD_NC_HISTORY\n"
                    "                  replaces their `history` attribute (default: \"<UTC now>: created by SHUD\").\n");
}

int shud_gpu_rhs_partition(shud_project_t p, int nparts_check, bool bench, int nevals, const std::string &outdir,
                           bool quiet);

// the SHUD_ARR_* arrays indexed by element (the others are per reach or per lake)
static bool arr_is_ele(int a) {
    switch (a) {
        case SHUD_ARR_Y_RIV_STG: case SHUD_ARR_Y_LAKE_STG: case SHUD_ARR_QRIV_DOWN: case SHUD_ARR_QRIV_UP:
        case SHUD_ARR_QRIV_SURF: case SHUD_ARR_QRIV_SUB: case SHUD_ARR_LAKE_TOPAREA: case SHUD_ARR_Q_LAKE_EVAP:
        case SHUD_ARR_Q_LAKE_PRCP: case SHUD_ARR_Q_LAKE_RIVIN: case SHUD_ARR_Q_LAKE_RIVOUT: case SHUD_ARR_Q_LAKE_SURF:
        case SHUD_ARR_Q_LAKE_SUB:
            return false;
        default:
            return true;
    }
}

static const char *lonlat_name(int m) { return m == 1 ? "FORCING_MEAN" : (m == 2 ? "FIXED" : "FORCING_FIRST"); }

// One run: what main() held as locals.  The stages below are main()'s blocks, in its order, under the names of their
// Python counterparts (shud_rhs/driver.py); a stage that fails has printed its message and returns the exit code, and
// main() returns it as it did before: nothing is torn down on a failure path.
struct Run {
    // ---- the command line ----
    std::string outdir, cwd, reorder, ckpt_path, resume_path, zones_path;
    const char *indir = nullptr, *prj = nullptr;
    double end_day = -1.0;
    long long max_steps = -1, ckpt_every = 0;
    bool quiet = false, rhs_bench = false, want_flood = false, want_ic = false, want_ckpt = false;
    int rhs_check = 0, evals = 0;
    std::chrono::steady_clock::time_point wall0, loop0;
    // ---- the project, and with --reorder the planned element order ----
    shud_project_t p = nullptr;
    ShudControl c;
    ShudMeshSoA mesh;
    ShudParamsSoA par;
    int64_t ny = 0;
    const double *y0 = nullptr, *y_is = nullptr, *y_snow = nullptr;              // in the device side's order
    // the input's own arrays: what .cfg.ic.bak and the first snapshot are written from, in the input's numbering
    const double *y0_in = nullptr, *y_is_in = nullptr, *y_snow_in = nullptr;
    std::vector<int32_t> perm, inv;
    shud_ordered_t ordered = nullptr;
    std::vector<std::vector<int32_t>> o_int;
    std::vector<std::vector<double>> o_dbl;
    // ---- the device side ----
    shud_rhs_t h = nullptr;
    ShudEtMeshSoA etm;
    ShudEtParams etp;
    shud_ode_t ode = nullptr;
    double *d_y = nullptr, *d_du = nullptr;
    shud_out_t out = nullptr;
    ShudNcOutputCfg ncc;
    std::vector<ShudOutputDecl> decl;
    int nprint = 0;
    shud_wb_t wb = nullptr;
    bool quad = false;
    long long quad_steps = 0;
    shud_mon_t mon = nullptr;
    std::string ic_update;
    long long ic_snaps = 0;
    std::thread ic0;
    int ic0_rc = 0;
    shud_ckpt_t ckpt = nullptr;
    // ---- the loop: the loop index, -n and -e count from the original start ----
    long long i0 = 0, nsteps = 0;
    double t = 0.0, tnext = 0.0;
    int rc = 0;
    // wall time per phase of the loop (host view: includes waiting on the device where a phase synchronizes)
    // forcing+BC rows, ET step, CVode, summary+diagnostics, export, wb diag, quad monitor (its f(), replay and pass)
    // run monitors (their enqueue; the writer thread's own time is reported beside it)
    double ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::chrono::steady_clock::time_point tick;

    int parse_args(int argc, char **argv);
    int load_project();
    int device_model();
    int add_outputs();
    int water_balance();
    int monitors();
    int checkpoint_resume();
    void time_loop();
    int report();

    void gather_i(const int32_t *&a);
    void gather_d(const double *&a, int planes, size_t tail);
    int ic_from_host(const std::string &fn, double th);
    int ic0_join();
    int ic_update_at(double tt, bool stepped);
    int checkpoint(long long step);
    void lap(int k) {
        const auto now = std::chrono::steady_clock::now();
        ph[k] += std::chrono::duration<double>(now - tick).count();
        tick = now;
    }
};

// ---- argument parsing and refusals -> -1 to go on, else the exit code ----
int Run::parse_args(int argc, char **argv) {
    std::vector<const char *> pos;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "-o" && i + 1 < argc) outdir = argv[++i];
        else if (a == "-e" && i + 1 < argc) end_day = atof(argv[++i]);
        else if (a == "-n" && i + 1 < argc) max_steps = atoll(argv[++i]);
        else if (a == "-C" && i + 1 < argc) cwd = argv[++i];
        else if (a == "-q") quiet = true;
        else if (a == "--rhs-check" && i + 1 < argc) rhs_check = atoi(argv[++i]);
        else if (a == "--rhs-bench") rhs_bench = true;
        else if (a == "--flood") want_flood = true;
        else if (a == "--ic-snapshots") want_ic = true;
        else if (a == "--reorder" && i + 1 < argc) reorder = argv[++i];
        else if (a == "--evals" && i + 1 < argc) evals = atoi(argv[++i]);
        else if (a == "--checkpoint" && i + 1 < argc) ckpt_path = argv[++i];
        else if (a == "--checkpoint-every" && i + 1 < argc) ckpt_every = atoll(argv[++i]);
        else if (a == "--resume" && i + 1 < argc) resume_path = argv[++i];
        else if (a == "--zones" && i + 1 < argc) zones_path = argv[++i];
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else pos.push_back(argv[i]);
    }
    if (pos.size() != 2) { usage(); return 1; }
    indir = pos[0];
    prj = pos[1];
    if (outdir.empty()) outdir = std::string("output/") + prj + ".out";
    if (!reorder.empty() && reorder != "bfs" && reorder != "tiles") {
        fprintf(stderr, "--reorder: unknown order '%s' (bfs, tiles)\n", reorder.c_str());
        return 1;
    }
    if (!reorder.empty() && env_truthy(getenv("SHUD_WB_DIAG"))) {
        fprintf(stderr, "--reorder cannot be combined with SHUD_WB_DIAG: the water-balance sums over the basin would "
                        "run in another element order\n");
        return 1;
    }
    want_ckpt = !ckpt_path.empty() || !resume_path.empty();
    if (ckpt_every < 0 || (ckpt_every > 0 && ckpt_path.empty())) {
        fprintf(stderr, "--checkpoint-every N needs N >= 1 and --checkpoint PATH\n");
        return 1;
    }
    if (want_ckpt && env_truthy(getenv("SHUD_WB_DIAG"))) {
        fprintf(stderr, "--checkpoint / --resume cannot be combined with SHUD_WB_DIAG: the water-balance object keeps "
                        "accumulators of its own, which a checkpoint does not hold\n");
        return 1;
    }
    wall0 = std::chrono::steady_clock::now();
    return -1;
}

// a per-element host array (then `tail` more values, copied) carried into the planned order
void Run::gather_i(const int32_t *&a) {
    if (!a) return;
    o_int.emplace_back(perm.size());
    shud_order_gather_host(perm.data(), (int32_t)perm.size(), sizeof(int32_t), 1, a, o_int.back().data());
    a = o_int.back().data();
}

void Run::gather_d(const double *&a, int planes, size_t tail) {
    if (!a) return;
    const size_t n = (size_t)planes * perm.size();
    o_dbl.emplace_back(n + tail);
    shud_order_gather_host(perm.data(), (int32_t)perm.size(), sizeof(double), planes, a, o_dbl.back().data());
    std::copy(a + n, a + n + tail, o_dbl.back().begin() + n);
    a = o_dbl.back().data();
}

// ---- the loaded project (loadinput + initialize + LoadIC, shud.cpp:49-64) and --reorder ----
int Run::load_project() {
    shud_project_control(p, &c);
    shud_project_mesh(p, &mesh, &par);
    y0_in = y0 = shud_project_array(p, "y0", &ny);
    y_is_in = y_is = shud_project_array(p, "y_is", nullptr);
    y_snow_in = y_snow = shud_project_array(p, "y_snow", nullptr);
    // ---- --reorder: the model, the ET mesh and the initial state in the planned element order ----
    if (!reorder.empty()) {
        const int ne = mesh.num_ele;
        perm.resize((size_t)ne);
        inv.resize((size_t)ne);
        ShudMeshSoA pm;
        ShudParamsSoA pp;
        if (shud_order_plan(&mesh, reorder == "tiles" ? SHUD_ORDER_TILES : SHUD_ORDER_BFS, nullptr, perm.data()) ||
            shud_order_apply(&mesh, &par, perm.data(), &ordered, &pm, &pp))
            return fail("--reorder");
        mesh = pm;
        par = pp;
        for (int k = 0; k < ne; k++) inv[perm[k]] = k;
        gather_d(y0, 3, (size_t)(ny - 3 * (int64_t)ne));
        gather_d(y_is, 1, 0);
        gather_d(y_snow, 1, 0);
    }
    if (!quiet)
        printf("* \t Project: %s  NumEle %d  NumRiv %d  NumSeg %d  NumLake %d  NY %lld\n"
               "* \t StartTime %.1f  EndTime %.1f [min]  SolverStep %.1f  ETStep %.1f  NumSteps %lld\n",
               prj, mesh.num_ele, mesh.num_riv, mesh.num_seg, mesh.num_lake, (long long)ny, c.start_time,
               c.end_time, c.solver_step, c.et_step, (long long)c.num_steps);
    return 0;
}

// ---- the device side: RHS handle, ET prelude, integrator (SetCVODE, cvode_config.cpp:149-197) ----
int Run::device_model() {
    ShudRhsOptions ro = {SHUD_MODE_SERIAL, 0, nullptr, 1};
    if (shud_rhs_create(&mesh, &par, &ro, &h)) return fail("shud_rhs_create");
    shud_project_et(p, &etm, &etp);
    if (!perm.empty()) {
        gather_i(etm.iforc); gather_i(etm.ilc); gather_i(etm.imf); gather_i(etm.ilake);
        gather_d(etm.z_surf, 1, 0); gather_d(etm.albedo, 1, 0); gather_d(etm.fix_pressure, 1, 0);
        gather_d(etm.wind_h, 1, 0); gather_d(etm.veg_frac, 1, 0); gather_d(etm.nx, 1, 0); gather_d(etm.ny, 1, 0);
        gather_d(etm.nz, 1, 0);
    }
    if (shud_et_attach(h, &etm, &etp) || shud_et_set_state(h, y_is, y_snow)) return fail("shud_et_attach");
    // carried u_satn before the first RHS: updateforcing's updateElement on f_update's globals, which are
    // freshly allocated (zero) before the first f() call -> u_satn = 0 (satn of an empty column)
    std::vector<double> zeros(mesh.num_ele, 0.0);
    ShudStepInputs si = {};
    si.u_satn = zeros.data();
    if (shud_rhs_set_step_inputs(h, &si)) return fail("shud_rhs_set_step_inputs");
    ShudOdeOptions oo = {c.reltol, c.abstol, c.init_step, c.max_step, 1e-6, 1000000, 0, 0};
    if (shud_ode_create(h, c.start_time, y0, SHUD_WHERE_HOST, &oo, &ode)) return fail("shud_ode_create");
    if (shud_rhs_device_alloc(h, (size_t)ny * sizeof(double), (void **)&d_y) ||
        shud_rhs_memcpy(h, d_y, y0, (size_t)ny * sizeof(double), 1))
        return fail("device alloc");
    return 0;
}

// ---- initialize_output (MD_initialize.cpp:246-345) with device sources ----
int Run::add_outputs() {
    if (mkdirs(outdir)) {
        fprintf(stderr, "cannot create output directory %s\n", outdir.c_str());
        return 1;
    }
    shud_rhs_prepare_outputs(h);
    shud_rhs_summary(h, d_y);
    shud_out_create(0, shud_rhs_stream(h), &out);
    // ---- NetcdfOutputContext (MD_initialize.cpp:346-347): the three files, attached when the mode asks for them ----
    shud_project_ncoutput(p, &ncc);
    static const char *mode_name[3] = {"LEGACY", "NETCDF", "BOTH"};
    if (!quiet) printf("* \t OUTPUT_MODE: %s\n", mode_name[ncc.output_mode]);      // Model_Control.cpp:641-643
    if (want_ckpt && ncc.output_mode != 0) {
        fprintf(stderr, "--checkpoint / --resume cannot be combined with OUTPUT_MODE %s: a NetCDF record file has no "
                        "reopen path, so a resumed run could not continue it\n", mode_name[ncc.output_mode]);
        return 1;
    }
    if (!zones_path.empty() && ncc.output_mode == 1) {
        fprintf(stderr, "--zones cannot be combined with OUTPUT_MODE NETCDF: the zonal outputs are legacy files "
                        "(.dat / .csv), which that mode does not write\n");
        return 1;
    }
    // --resume: the controls keep the files of the run that wrote the checkpoint (cut back at the restore below)
    if (!resume_path.empty()) shud_out_resume(out, 1);
    if (ncc.output_mode != 0) {
        int64_t nnode = 0;
        const double *node_x = shud_project_node_xy(p, 0, &nnode), *node_y = shud_project_node_xy(p, 1, nullptr);
        const char *hist = getenv("SHUD_NC_HISTORY");
        const int n_of[SHUD_NC_KINDS] = {mesh.num_ele, mesh.num_riv, mesh.num_lake};
        for (int k = 0; k < SHUD_NC_KINDS; k++) {
            if (k != SHUD_NC_ELE && n_of[k] <= 0) continue;
            ShudNcSpec ns = {k, n_of[k], ncc.out_dir, (int64_t)c.forc_start_time, hist && hist[0] ? hist : nullptr,
                             ncc.crs_wkt, (int32_t)nnode, node_x, node_y, shud_project_ele_nodes(p, nullptr),
                             shud_project_array(p, "x", nullptr), shud_project_array(p, "y", nullptr)};
            if (shud_out_attach_nc(out, &ns)) return fail("shud_out_attach_nc");
        }
    }
    const int nd = shud_project_outputs(p, outdir.c_str(), nullptr, 0);
    decl.resize(nd);
    shud_project_outputs(p, outdir.c_str(), decl.data(), nd);
    for (const auto &d : decl) {
        int64_t n = 0;
        const double *src = shud_rhs_device_array(h, d.array, &n);
        if (!src) {
            fprintf(stderr, "no device source for %s\n", d.basename);
            return 1;
        }
        if (d.column >= 0) src += (size_t)d.column * mesh.num_ele;
        ShudPrintSpec ps = {d.basename, src, d.n_all, d.flag_io, d.interval, d.iflux, (int64_t)c.forc_start_time,
                            c.binary, c.ascii, c.radiation_input_mode, c.terrain_radiation,
                            lonlat_name(c.solar_lonlat_mode), c.solar_lon_deg, c.solar_lat_deg};
        // --reorder: column c of an element output reads the internal element inv[c]
        const bool mapped = !inv.empty() && arr_is_ele(d.array) && d.n_all == mesh.num_ele;
        if (!inv.empty() && arr_is_ele(d.array) && !mapped) {
            fprintf(stderr, "--reorder: element output %s has %d columns, mesh %d elements\n", d.basename, d.n_all,
                    mesh.num_ele);
            return 1;
        }
        // setSink (MD_initialize.cpp:348-356): by NumAll, elements first, then reaches, then lakes
        int kind = -1;
        if (ncc.output_mode != 0) {
            if (d.n_all == mesh.num_ele) kind = SHUD_NC_ELE;
            else if (mesh.num_riv > 0 && d.n_all == mesh.num_riv) kind = SHUD_NC_RIV;
            else if (mesh.num_lake > 0 && d.n_all == mesh.num_lake) kind = SHUD_NC_LAKE;
        }
        if (ncc.output_mode == 1) ps.binary = ps.ascii = 0;          // open_file(0, 0, ...) (:362-363)
        if (kind >= 0 ? shud_out_add_nc(out, &ps, mapped ? inv.data() : nullptr, kind, ncc.output_mode == 2)
                      : (mapped ? shud_out_add_mapped(out, &ps, inv.data()) : shud_out_add(out, &ps))) {
            fprintf(stderr, "shud_out_add(%s): %s\n", d.basename, shud_rhs_last_error_string());
            return 1;
        }
        nprint++;
    }
    // ---- --zones: the zonal twin of every element control (shud_rhs/driver.py: add_zonal_outputs) ----
    if (!zones_path.empty()) {
        const int32_t *zone = nullptr;
        int32_t nz = 0;
        if (shud_project_zones(p, zones_path.c_str(), &zone, &nz)) {
            fprintf(stderr, "--zones: %s\n", shud_project_error());
            return 1;
        }
        // the weights by the file's element numbering, like the zone ids: element c is the internal inv[c]
        std::vector<double> area((size_t)mesh.num_ele);
        for (int k = 0; k < mesh.num_ele; k++) area[(size_t)k] = mesh.area[inv.empty() ? k : inv[(size_t)k]];
        for (const auto &d : decl) {
            if (!arr_is_ele(d.array) || d.n_all != mesh.num_ele) continue;
            const double *src = shud_rhs_device_array(h, d.array, nullptr);
            if (d.column >= 0) src += (size_t)d.column * mesh.num_ele;
            const std::string base(d.basename);
            const size_t dot = base.rfind('.');
            const std::string leaf = base.substr(dot + 1), name = base.substr(0, dot) + ".zone." + leaf;
            const bool total = leaf.compare(0, 4, "eleq") == 0;
            ShudPrintSpec ps = {name.c_str(), src, d.n_all, nullptr, d.interval, d.iflux, (int64_t)c.forc_start_time,
                                c.binary, c.ascii, c.radiation_input_mode, c.terrain_radiation,
                                lonlat_name(c.solar_lonlat_mode), c.solar_lon_deg, c.solar_lat_deg};
            ShudZoneSpec zs = {nz, zone, total ? nullptr : area.data(), total ? SHUD_ZONE_SUM : SHUD_ZONE_WMEAN};
            if (shud_out_add_zonal(out, &ps, inv.empty() ? nullptr : inv.data(), &zs)) {
                fprintf(stderr, "shud_out_add_zonal(%s): %s\n", name.c_str(), shud_rhs_last_error_string());
                return 1;
            }
            nprint++;
        }
    }
    // the NetCDF headers and fixed variables (the mesh): before the time loop, not inside its first export
    if (ncc.output_mode != 0 && shud_out_nc_begin(out)) return fail("shud_out_nc_begin");
    return 0;
}

// ---- WaterBalanceDiag::enable (shud.cpp:70-75): shud.cpp:72's test, then openFiles' env_truthy ----
int Run::water_balance() {
    const char *wb_env = getenv("SHUD_WB_DIAG");
    if (wb_env != nullptr && wb_env[0] != '\0' && strcmp(wb_env, "0") != 0 && env_truthy(wb_env)) {
        quad = env_truthy(getenv("SHUD_WB_DIAG_QUAD"));       // read only when the diagnostic is on (:271)
        const std::string prefix = outdir + "/" + prj;
        ShudWbOptions wo = {c.start_time, shud_project_wb_interval(p), env_truthy(getenv("SHUD_WB_DIAG_TRAPZ")) ? 1 : 0,
                            (int64_t)c.forc_start_time, c.radiation_input_mode, c.terrain_radiation,
                            lonlat_name(c.solar_lonlat_mode), c.solar_lon_deg, c.solar_lat_deg, prefix.c_str()};
        if (shud_wb_create(h, &mesh, &par, &wo, &wb) ||
            shud_rhs_device_alloc(h, (size_t)ny * sizeof(double), (void **)&d_du))
            return fail("shud_wb_create");
        if (quad && shud_wb_quad_enable(wb)) return fail("shud_wb_quad_enable");
    }
    return 0;
}

// LoadIC's values through the device-free formatter (what the reference's arrays hold before the first step)
int Run::ic_from_host(const std::string &fn, double th) {
    const int NE = mesh.num_ele, NR = mesh.num_riv, NL = mesh.num_lake;
    return shud_mon_write_ic_host(fn.c_str(), th, NE, NR, NL, y_is_in, y_snow_in, y0_in, y0_in + NE,
                                  y0_in + 2 * (size_t)NE, y0_in + 3 * (size_t)NE,
                                  NL ? y0_in + 3 * (size_t)NE + NR : nullptr);
}

// ---- PrintInit(Init_bak, 0) and InitFloodAlert (shud.cpp:76-77), only with --ic-snapshots / --flood ----
int Run::monitors() {
    ic_update = outdir + "/" + prj + ".cfg.ic.update";
    const int NE = mesh.num_ele, NR = mesh.num_riv, NL = mesh.num_lake;
    if (want_flood || want_ic) {
        if (shud_mon_create(0, shud_rhs_stream(h), &mon)) return fail("shud_mon_create");
        if (!resume_path.empty()) shud_mon_resume(mon, 1);
        if (want_ic) {
            const std::string bak = outdir + "/" + prj + ".cfg.ic.bak";
            if (ic_from_host(bak, 0)) {
                fprintf(stderr, "cannot write %s\n", bak.c_str());
                return 1;
            }
            ShudIcSpec is = {ic_update.c_str(), shud_project_update_ic_step(p), NE, NR, NL,
                             shud_rhs_device_array(h, SHUD_ARR_Y_ELE_IS, nullptr),
                             shud_rhs_device_array(h, SHUD_ARR_Y_ELE_SNOW, nullptr),
                             shud_rhs_device_array(h, SHUD_ARR_Y_ELE_SURF, nullptr),
                             shud_rhs_device_array(h, SHUD_ARR_Y_ELE_UNSAT, nullptr),
                             shud_rhs_device_array(h, SHUD_ARR_Y_ELE_GW, nullptr),
                             shud_rhs_device_array(h, SHUD_ARR_Y_RIV_STG, nullptr),
                             NL ? shud_rhs_device_array(h, SHUD_ARR_Y_LAKE_STG, nullptr) : nullptr};
            if (shud_mon_add_ic(mon, &is) || (!perm.empty() && shud_mon_set_ic_order(mon, perm.data())))
                return fail("shud_mon_add_ic");
        }
        if (want_flood) {
            const std::string fcsv = outdir + "/" + prj + ".flood.csv";
            ShudFloodSpec fs = {fcsv.c_str(), shud_rhs_device_array(h, SHUD_ARR_Y_RIV_STG, nullptr),
                                shud_rhs_device_array(h, SHUD_ARR_QRIV_DOWN, nullptr), NR, mesh.riv_depth,
                                shud_project_riv_type(p, nullptr)};
            if (shud_mon_add_flood(mon, &fs)) return fail("shud_mon_add_flood");
        }
    }
    return 0;
}

// PrintInit(Init_update, t): LoadIC's values until the first step has run (formatted on a thread of its own,
// joined before anything else may write the file), the device arrays afterwards
int Run::ic0_join() {
    if (ic0.joinable()) ic0.join();
    return ic0_rc;
}

int Run::ic_update_at(double tt, bool stepped) {
    int due = ic0_join() ? -1 : 0;
    if (due == 0 && stepped) {
        due = shud_mon_ic_update(mon, tt);
    } else if (due == 0) {
        const int ustep = shud_project_update_ic_step(p);
        due = ((unsigned long)(long)tt) % (unsigned long)ustep == 0;
        if (due) ic0 = std::thread([this, tt] { ic0_rc = ic_from_host(ic_update, tt); });
    }
    if (due < 0) {
        fprintf(stderr, "restart snapshot at t = %f: %s\n", tt, shud_rhs_last_error_string());
        return 1;
    }
    ic_snaps += due;
    return 0;
}

// ---- --checkpoint / --resume (include/shud_ckpt.h), inside the timed part of the run ----
int Run::checkpoint_resume() {
    t = c.start_time, tnext = t;
    nsteps = max_steps >= 0 && max_steps < c.num_steps ? max_steps : c.num_steps;
    if (!resume_path.empty()) {
        const ShudCkptParts parts = {h, ode, out, mon, wb};
        int64_t step = 0;
        if (shud_ckpt_restore(resume_path.c_str(), &parts, &t, &step)) {
            fprintf(stderr, "--resume %s: %s\n", resume_path.c_str(), shud_rhs_last_error_string());
            return 1;
        }
        i0 = (long long)step;
        tnext = t;
        if (!quiet) printf("* \t resumed from %s: solver step %lld, t = %.3f min\n", resume_path.c_str(), i0, t);
    }
    if (!ckpt_path.empty() && shud_ckpt_create(0, shud_rhs_stream(h), &ckpt)) return fail("shud_ckpt_create");
    return 0;
}

int Run::checkpoint(long long step) {
    const ShudCkptParts parts = {h, ode, out, mon, wb};
    if (shud_ckpt_snapshot(ckpt, &parts, t, step, ckpt_path.c_str())) {
        fprintf(stderr, "--checkpoint %s: %s\n", ckpt_path.c_str(), shud_rhs_last_error_string());
        return 1;
    }
    return 0;
}

// ---- the time loop (shud.cpp:86-140), the final checkpoint and the restart snapshot after it (shud.cpp:157) ----
void Run::time_loop() {
    const bool et_sub = c.et_step > kZero && c.et_step + kZero < c.solver_step;
    tick = std::chrono::steady_clock::now();
    for (long long i = i0; i < nsteps && !rc; i++) {
        if (want_ic) {                            // MD->PrintInit(fout->Init_update, t)
            if (ic_update_at(t, i > 0)) {
                rc = 1;
                break;
            }
            lap(7);
        }
        tnext += c.solver_step;
        while (t + kZero < tnext) {
            const double tout = et_sub ? std::fmin(t + c.et_step, tnext) : tnext;
            ShudEtForcing f;
            if (shud_project_forcing(p, t, tout, &f)) {
                fprintf(stderr, "%s\n", shud_project_error());
                rc = 1;
                break;
            }
            ShudStepInputs bc = {};                 // tsd_eyBC .. tsd_rqBC rows (f_update's getX)
            if (shud_project_bc_rows(p, &bc) == 1 && shud_rhs_set_step_inputs(h, &bc)) {
                fprintf(stderr, "shud_rhs_set_step_inputs (BC rows): %s\n", shud_rhs_last_error_string());
                rc = 1;
                break;
            }
            lap(0);
            if (shud_et_step(h, &f)) {
                ShudErr e;
                shud_rhs_get_error(h, &e);
                fprintf(stderr, "%s\n", e.message[0] ? e.message : shud_rhs_last_error_string());
                rc = e.exit_code ? e.exit_code : 1;
                break;
            }
            lap(1);
            if (wb) {                               // wbdiag->onETUpdate()
                if (shud_wb_on_et_update(wb)) {
                    fprintf(stderr, "shud_wb_on_et_update: %s\n", shud_rhs_last_error_string());
                    rc = 1;
                    break;
                }
                lap(5);
            }
            if (et_sub || quad) shud_ode_set_stop_time(ode, tout);
            int flag = 0;
            if (quad) {
                // shud.cpp:121-129: CV_ONE_STEP to tout; after every internal step f(t, udata, du, MD) on the
                // returned state (stateful, like the sample's extra f()), its flux arrays, onCvodeMonitorStep(t)
                while (t + kZero < tout) {
                    flag = shud_ode_solve(ode, tout, d_y, SHUD_WHERE_DEVICE, &t, SHUD_ODE_ONE_STEP);
                    if (flag < 0) break;
                    lap(2);
                    int qrc = shud_rhs_eval(h, t, d_y, d_du, SHUD_WHERE_DEVICE);
                    if (!qrc) qrc = shud_rhs_refresh_diagnostics(h);
                    if (!qrc) qrc = shud_wb_quad_step(wb, t);
                    if (qrc) {
                        fprintf(stderr, "quad monitor: %s (code %d)\n", shud_rhs_last_error_string(), qrc);
                        rc = 1;
                        break;
                    }
                    quad_steps++;
                    lap(6);
                }
                if (rc) break;
            } else {
                flag = shud_ode_solve(ode, tout, d_y, SHUD_WHERE_DEVICE, &t, SHUD_ODE_NORMAL);
            }
            if (flag < 0) {
                ShudErr e;
                shud_rhs_get_error(h, &e);
                if (flag == SHUD_ODE_RHSFUNC_FAIL && e.exit_code) {
                    printf("\n%s\n", e.message);
                    fprintf(stderr, "\nEXIT with error code %d\n", e.exit_code);
                    rc = e.exit_code;
                } else {
                    fprintf(stderr, "CVode failed with flag %d at t = %f (%s)\n", flag, t, shud_rhs_last_error_string());
                    rc = 1;
                }
                break;
            }
            lap(2);
        }
        if (rc) break;
        shud_rhs_summary(h, d_y);                 // Model_Data::summary(udata)
        if (wb) {
            lap(3);
            // f(t, udata, du, MD) on the accepted state (stateful: advances qEleE_IC and the carried u_satn, as in
            // the reference), its flux arrays, CVodeGetDky(mem, t, 1, du), sample(t, du), maybeWrite(t)
            int wrc = shud_rhs_eval(h, t, d_y, d_du, SHUD_WHERE_DEVICE);
            if (!wrc) wrc = shud_rhs_refresh_diagnostics(h);
            if (!wrc) wrc = shud_ode_get_dky(ode, t, 1, d_du, SHUD_WHERE_DEVICE);
            if (!wrc) wrc = shud_wb_sample(wb, t, d_du);
            if (!wrc && shud_wb_maybe_write(wb, t) < 0) wrc = 1;
            if (wrc) {
                fprintf(stderr, "water-balance diagnostics: %s (code %d)\n", shud_rhs_last_error_string(), wrc);
                rc = 1;
            }
            lap(5);
        } else {
            shud_rhs_refresh_diagnostics(h);      // the flux arrays of CVODE's last f() call
            lap(3);
        }
        if (shud_out_export(out, t)) {            // Control_Data::ExportResults(t)
            fprintf(stderr, "shud_out_export: %s\n", shud_rhs_last_error_string());
            rc = 1;
        }
        lap(4);
        if (want_flood) {                         // MD->flood->FloodWarning(t)
            if (shud_mon_flood(mon, t)) {
                fprintf(stderr, "shud_mon_flood: %s\n", shud_rhs_last_error_string());
                rc = 1;
            }
            lap(7);
        }
        if (!quiet && c.verbose) printf("step %lld  t = %.3f min\n", i + 1, t);
        // stepping goes on while the checkpoint drains; the one after the last step is written below
        if (ckpt && !rc && ckpt_every > 0 && (i + 1) % ckpt_every == 0 && i + 1 < nsteps) rc = checkpoint(i + 1);
    }
    if (ckpt) {                                   // the state at the end of the run: --resume continues from here
        if (!rc && nsteps >= i0) rc = checkpoint(nsteps > i0 ? nsteps : i0);
        if (shud_ckpt_destroy(ckpt)) {            // waits for the file
            fprintf(stderr, "--checkpoint %s: %s\n", ckpt_path.c_str(), shud_rhs_last_error_string());
            if (!rc) rc = 1;
        }
    }
    if (want_ic && !rc) {                         // MD->PrintInit(fout->Init_update, t) after the loop
        if (ic_update_at(t, nsteps > 0 || i0 > 0)) rc = 1;
        lap(7);
    }
}

// ---- the final report and the JSON line; everything is flushed and torn down -> the exit code ----
int Run::report() {
    shud_rhs_synchronize(h);
    const double loop_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - loop0).count();
    // what the output set launched (include/shud_out.h: shud_out_launches), for the machine-readable line
    int64_t launches[SHUD_OUT_KERNELS] = {};
    shud_out_launches(out, launches);
    std::string launch_txt;
    for (int k = 0; k < SHUD_OUT_KERNELS; k++)
        launch_txt += std::string(k ? ", \"" : "\"") + shud_out_kernel_name(k) + "\": " + std::to_string((long long)launches[k]);
    shud_out_destroy(out);
    long long flood_rows = 0;
    double mon_writer_s = 0.0;
    if (mon) {
        if (ic0_join()) {
            fprintf(stderr, "cannot write %s\n", ic_update.c_str());
            if (!rc) rc = 1;
        }
        if (shud_mon_flush(mon)) {
            fprintf(stderr, "shud_mon_flush: %s\n", shud_rhs_last_error_string());
            if (!rc) rc = 1;
        } else {
            if (want_flood) flood_rows = (long long)shud_mon_flood_rows(mon);
            mon_writer_s = shud_mon_writer_seconds(mon);
        }
        if (shud_mon_destroy(mon)) {
            fprintf(stderr, "shud_mon_destroy: %s\n", shud_rhs_last_error_string());
            if (!rc) rc = 1;
        }
    }
    if (wb && shud_wb_destroy(wb)) {
        fprintf(stderr, "shud_wb_destroy: %s\n", shud_rhs_last_error_string());
        if (!rc) rc = 1;
    }
    ShudOdeStats st;
    shud_ode_get_stats(ode, &st);
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count();
    if (!quiet)
        printf("* \t t = %.3f min  steps %lld  RHS %lld  Newton %lld  Krylov %lld  err-test fails %lld  "
               "%d outputs  wall %.2f s (time loop %.2f s)\n",
               t, (long long)st.nst, (long long)(st.nfe + st.nfe_ls), (long long)st.nni, (long long)st.nli,
               (long long)st.netf, nprint, wall, loop_s);
    // one machine-readable line (tools/e2e.sh); the quad monitor's phase and step count appear only
    // when it ran, and so do the run monitors' phase, writer time and counts
    char quad_txt[48] = "", quad_n[48] = "", mon_txt[48] = "", mon_n[128] = "";
    if (mon) {
        snprintf(mon_txt, sizeof(mon_txt), ", \"monitors\": %.4f", ph[7]);
        snprintf(mon_n, sizeof(mon_n), "\"flood_rows\": %lld, \"ic_snapshots\": %lld, \"monitors_writer_s\": %.4f, ",
                 flood_rows, ic_snaps, mon_writer_s);
    }
    if (quad) {
        snprintf(quad_txt, sizeof(quad_txt), ", \"wb_quad\": %.4f", ph[6]);
        snprintf(quad_n, sizeof(quad_n), "\"quad_steps\": %lld, ", quad_steps);
    }
    printf("{\"shud_gpu\": {\"num_ele\": %d, \"t_end_min\": %.6f, \"solver_steps\": %lld, \"cvode_steps\": %lld, "
           "\"rhs_evals\": %lld, \"newton_iters\": %lld, \"krylov_iters\": %lld, \"outputs\": %d, "
           "\"wall_s\": %.4f, \"loop_s\": %.4f, \"loop_phases_s\": {\"forcing\": %.4f, \"et_step\": %.4f, "
           "\"cvode\": %.4f, \"summary_diag\": %.4f, \"export\": %.4f, \"wb_diag\": %.4f%s%s}, \"host_syncs\": %lld, "
           "%s%s\"out_launches\": {%s}, \"exit\": %d}}\n",
           mesh.num_ele, t, nsteps, (long long)st.nst, (long long)(st.nfe + st.nfe_ls), (long long)st.nni,
           (long long)st.nli, nprint, wall, loop_s, ph[0], ph[1], ph[2], ph[3], ph[4], ph[5], quad_txt, mon_txt,
           (long long)st.n_sync, quad_n, mon_n, launch_txt.c_str(), rc);
    shud_ode_destroy(ode);
    shud_rhs_device_free(h, d_y);
    if (d_du) shud_rhs_device_free(h, d_du);
    shud_rhs_destroy(h);
    if (ordered) shud_order_free(ordered);
    shud_project_free(p);
    return rc;
}

int main(int argc, char **argv) {
    Run r;
    const int arc = r.parse_args(argc, argv);
    if (arc >= 0) return arc;
    // ---- loadinput + initialize + LoadIC (shud.cpp:49-64) ----
    if (shud_project_load(r.indir, r.prj, r.cwd.empty() ? nullptr : r.cwd.c_str(), r.end_day, &r.p)) {
        fprintf(stderr, "%s\n", shud_project_error());
        return 1;
    }
    if (r.rhs_check > 0 || r.rhs_bench) {
        const int rc = shud_gpu_rhs_partition(r.p, r.rhs_check, r.rhs_bench,
                                              r.evals > 0 ? r.evals : (r.rhs_bench ? 100 : 6), r.outdir, r.quiet);
        shud_project_free(r.p);
        return rc;
    }
    if (r.load_project() || r.device_model() || r.add_outputs() || r.water_balance() || r.monitors()) return 1;
    shud_rhs_synchronize(r.h);
    r.loop0 = std::chrono::steady_clock::now();
    if (r.checkpoint_resume()) return 1;
    r.time_loop();
    return r.report();
}
