/* shud_ref_driver.cpp — test driver of the REFERENCE model's own code (this file is ours; the reference's units
 * are compiled in place from a reference checkout by `make -C oracle ref`, never copied or committed).
 *
 * It follows SHUD()'s sequence (src/Model/shud.cpp) without the CVODE solver: CommandIn::parse / setFileIO,
 * new Model_Data, loadinput, initialize, CheckInputData, LoadIC, SetIC2Y, then per ET step
 * updateAllTimeSeries(t), updateforcing(t), ET(t, t + ETStep), and calls of the reference's f(t, u, du, MD).
 *
 *   shud_ref_f f  OUT STATES N_ET THREADS <reference arguments>   RHS mode
 *       runs N_ET >= 1 ET steps from StartTime (t advances by ETStep between them), dumps the step inputs the
 *       reference then holds, reads STATES (raw float64, K vectors of NumY) and evaluates f() on them in order
 *       in this one process (so the carried qEleE_IC / u_satn / uYgw advance as in a run), dumping DY per call.
 *   shud_ref_f et OUT -      N_ET THREADS <reference arguments>   ET-prelude mode
 *       runs N_ET ET steps and dumps the per-element prelude results after each.
 *   shud_ref_f w  OUT SCRIPT 0    THREADS <reference arguments>   writers mode
 *       SHUD()'s whole sequence (shud.cpp:69-157) with CVODE taken out: initialize_output, WaterBalanceDiag
 *       (enabled by SHUD_WB_DIAG as there), PrintInit, InitFloodAlert, the loop over NumSteps / SolverStep with
 *       the ET sub-step rule, summary, sample / maybeWrite, ExportResults, FloodWarning.  A CVode(...) call is
 *       replaced by the next record of SCRIPT: the state is read into u, t is set to the record's time, and the
 *       reference's f(t, u, du, MD) is called, so its flux arrays hold that call as after CVODE's last RHS
 *       evaluation.  After the inner loop the next record is read into u (y(tout), as CVode returns it); with the
 *       water balance on, the DY of the f() call shud.cpp makes there stands in for CVodeGetDky.  SCRIPT is a
 *       sequence of records (kind, t, y[NumY]) of float64: kind 0 a CVode return, 2 a CV_ONE_STEP return
 *       (SHUD_WB_DIAG_QUAD), 1 the state returned to summary (its t is not used).  The files the reference
 *       writes into its output directory are the recording; every restart file is copied aside
 *       (<name>.<k>) when PrintInit wrote it.  OUT gets the events in order: "ev_et" (step inputs after ET()),
 *       "ev_f" (t of an f() call, BC rows), "ev_x" (the arrays the reference holds at ExportResults).
 *
 * THREADS: the OpenMP build's team size.  The reference takes max(NUM_OPENMP of <prj>.cfg.para, -n) and passes it
 * to every loop of MD_f_omp.cpp as num_threads(CS.num_threads), so neither OMP_NUM_THREADS nor -n can lower it;
 * the driver therefore sets CS.num_threads itself after loadinput(), and dumps the team size a parallel region
 * with that clause really gets ("threads"; 1 in the serial build).
 * OUT is a sequence of records: 16-byte zero-padded name, int64 count, count float64 values
 * (oracle/ref/refio.py reads it).  Built twice: plain (serial f) and -D_OPENMP_ON -fopenmp (f_*_omp).
 * Some members needed here are private in the reference (t_lai, t_temp, ...): this one unit is compiled with
 * `private`/`protected` read as `public`, after the standard headers; the reference's units are untouched. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <queue>
#include <sstream>
#include <string>
#include <vector>
#ifdef _OPENMP_ON
#include <omp.h>
#endif
#define private public
#define protected public
#include "f.hpp"
#include "IO.hpp"
#include "Model_Data.hpp"
#include "CommandIn.hpp"
#include "FloodAlert.hpp"
#include "WaterBalanceDiag.hpp"
#undef private
#undef protected

/* the globals src/Model/shud.cpp defines */
double *uYsf, *uYus, *uYgw, *uYriv, *uYlake, *globalY;
double timeNow;
int dummy_mode = 0, global_fflush_mode = 0, global_implicit_mode = 1, global_verbose_mode = 1, lakeon = 0;

#ifdef _OPENMP_ON
#define REF_DATA(v) NV_DATA_OMP(v)
static N_Vector new_vec(int n) {
    return new _generic_N_Vector{new _N_VectorContent_OpenMP{n, 1, new double[n](), 1}};
}
#else
#define REF_DATA(v) NV_DATA_S(v)
static N_Vector new_vec(int n) { return new _generic_N_Vector{new _N_VectorContent_Serial{n, 1, new double[n]()}}; }
#endif

static FILE *g_out;
static void rec(const char *name, const double *p, long n) {
    char nm[16];
    memset(nm, 0, sizeof nm);
    strncpy(nm, name, 15);
    long long cnt = n;
    fwrite(nm, 1, 16, g_out);
    fwrite(&cnt, sizeof cnt, 1, g_out);
    if (n > 0) fwrite(p, sizeof(double), (size_t)n, g_out);
}
static void rec_tsd(const char *name, _TimeSeriesData &ts, double t) {
    std::vector<double> row((size_t)ts.get_Ncol());
    for (int c = 0; c < ts.get_Ncol(); c++) row[(size_t)c] = ts.getX(t, c);
    rec(name, row.data(), (long)row.size());
}

static int g_ic_copies;
static int print_init(Model_Data *MD, const char *fn, double t) {
    const int wrote = MD->PrintInit(fn, t);
    if (wrote) {                                       /* the file is overwritten by the next one: keep a copy */
        std::ifstream src(fn, std::ios::binary);
        std::ofstream dst(std::string(fn) + "." + std::to_string(g_ic_copies++), std::ios::binary);
        dst << src.rdbuf();
    }
    return wrote;
}
static void rec_step_inputs(Model_Data *MD, double t, std::vector<double> &tmp) {
    const int NE = MD->NumEle;
    rec("ev_et", &t, 1);
    rec("net_prep", MD->qEleNetPrep, NE);
    rec("pot_evap", MD->qPotEvap, NE);
    rec("pot_tran", MD->qPotTran, NE);
    rec("etp", MD->qEleETP, NE);
    rec("lai", MD->t_lai, NE);
    rec("fu_surf", MD->fu_Surf, NE);
    rec("fu_sub", MD->fu_Sub, NE);
    rec("e_ic", MD->qEleE_IC, NE);
    for (int i = 0; i < NE; i++) tmp[(size_t)i] = MD->Ele[i].u_satn;
    rec("u_satn", tmp.data(), NE);
    rec("ugw_stale", uYgw, NE);
    rec("prcp", MD->qElePrep, NE);
    rec("y_is", MD->yEleIS, NE);
    rec("y_snow", MD->yEleSnow, NE);
}
static void rec_f(Model_Data *MD, double t) {
    rec("ev_f", &t, 1);
    if (MD->ieBC1 && MD->NumBCEle1 > 0) rec_tsd("ele_ybc", MD->tsd_eyBC, t);
    if (MD->ieBC2 && MD->NumBCEle2 > 0) rec_tsd("ele_qbc", MD->tsd_eqBC, t);
    if (MD->irBC1 && MD->NumBCRiv1 > 0) rec_tsd("riv_ybc", MD->tsd_ryBC, t);
    if (MD->irBC2 && MD->NumBCRiv2 > 0) rec_tsd("riv_qbc", MD->tsd_rqBC, t);
}
static void rec_summary(Model_Data *MD) {
    rec("y_surf", MD->yEleSurf, MD->NumEle);
    rec("y_unsat", MD->yEleUnsat, MD->NumEle);
    rec("y_gw", MD->yEleGW, MD->NumEle);
    rec("y_riv", MD->yRivStg, MD->NumRiv);
    rec("y_lake", MD->yLakeStg, MD->NumLake);
}
static void rec_export(Model_Data *MD, double t, std::vector<double> &tmp) {
    const int NE = MD->NumEle, NR = MD->NumRiv, NL = MD->NumLake;
    rec("ev_x", &t, 1);
    rec_summary(MD);
    std::vector<double> e3((size_t)(3 * NE));
    for (int j = 0; j < 3; j++)
        for (int i = 0; i < NE; i++) e3[(size_t)(j * NE + i)] = MD->QeleSurf[i][j];
    rec("qele_surf", e3.data(), 3 * NE);
    for (int j = 0; j < 3; j++)
        for (int i = 0; i < NE; i++) e3[(size_t)(j * NE + i)] = MD->QeleSub[i][j];
    rec("qele_sub", e3.data(), 3 * NE);
    rec("qele_surf_tot", MD->QeleSurfTot, NE);
    rec("qele_sub_tot", MD->QeleSubTot, NE);
    rec("q_infil", MD->qEleInfil, NE);
    rec("q_exfil", MD->qEleExfil, NE);
    rec("q_recharge", MD->qEleRecharge, NE);
    rec("q_es", MD->qEs, NE);
    rec("q_eu", MD->qEu, NE);
    rec("q_eg", MD->qEg, NE);
    rec("q_tu", MD->qTu, NE);
    rec("q_tg", MD->qTg, NE);
    rec("q_eta", MD->qEleETA, NE);
    rec("q_trans", MD->qEleTrans, NE);
    rec("q_evapo", MD->qEleEvapo, NE);
    rec("e_ic_f", MD->qEleE_IC, NE);
    for (int i = 0; i < NE; i++) tmp[(size_t)i] = MD->Ele[i].u_satn;
    rec("u_satn_f", tmp.data(), NE);
    rec("qe2r_surf", MD->Qe2r_Surf, NE);
    rec("qe2r_sub", MD->Qe2r_Sub, NE);
    rec("qriv_down", MD->QrivDown, NR);
    rec("qriv_up", MD->QrivUp, NR);
    rec("qriv_surf", MD->QrivSurf, NR);
    rec("qriv_sub", MD->QrivSub, NR);
    rec("q_lake_surf", MD->QLakeSurf, NL);
    rec("q_lake_sub", MD->QLakeSub, NL);
    rec("q_lake_rivin", MD->QLakeRivIn, NL);
    rec("q_lake_rivout", MD->QLakeRivOut, NL);
    rec("q_lake_evap", MD->qLakeEvap, NL);
    rec("q_lake_prcp", MD->qLakePrcp, NL);
    rec("lake_toparea", MD->y2LakeArea, NL);
    rec("rn_h", MD->ele_rn_h_wm2, MD->ele_rn_h_wm2 ? NE : 0);
    rec("rn_t", MD->ele_rn_t_wm2, MD->ele_rn_t_wm2 ? NE : 0);
    rec("rn_factor", MD->ele_rn_factor, MD->ele_rn_factor ? NE : 0);
}
/* the next record of the script: kind, t, y -> u */
static int next_state(FILE *fs, N_Vector u, int NY, double *t) {
    double head[2];
    if (fread(head, sizeof(double), 2, fs) != 2 || fread(REF_DATA(u), sizeof(double), (size_t)NY, fs) != (size_t)NY) {
        fprintf(stderr, "shud_ref_f w: the script ended early\n");
        exit(3);
    }
    *t = head[1];
    return (int)head[0];
}
static void expect(int kind, int want) {
    if (kind != want) {
        fprintf(stderr, "shud_ref_f w: script record of kind %d where %d is due\n", kind, want);
        exit(3);
    }
}

/* SHUD() of src/Model/shud.cpp from initialize_output() on, CVODE replaced by the script */
static int run_writers(Model_Data *MD, FileOut *fout, N_Vector u, N_Vector du, const char *script) {
    const int NY = MD->NumY, NE = MD->NumEle;
    std::vector<double> tmp((size_t)NE);
    FILE *fs = fopen(script, "rb");
    if (!fs) { perror(script); return 2; }
    MD->initialize_output();
    WaterBalanceDiag wbdiag(MD);
    const char *shud_wb_diag = getenv("SHUD_WB_DIAG");
    if (shud_wb_diag != nullptr && shud_wb_diag[0] != '\0' && strcmp(shud_wb_diag, "0") != 0) {
        wbdiag.enable();
        MD->wbdiag = &wbdiag;
    }
    double flags[3] = {(double)wbdiag.isEnabled(), (double)wbdiag.quadEnabled(), (double)MD->CS.NumPrint};
    rec("wb_flags", flags, 3);
    double ctl[4] = {(double)MD->CS.NumSteps, MD->CS.SolverStep, MD->CS.ETStep, (double)MD->CS.UpdateICStep};
    rec("control", ctl, 4);
    rec("ev_x0", &MD->CS.StartTime, 1);
    rec_summary(MD);
    print_init(MD, fout->Init_bak, 0);
    MD->InitFloodAlert(fout->floodout);
    double t = MD->CS.StartTime, tnext = t;
    const bool etSubstepEnabled = (MD->CS.ETStep > ZERO && MD->CS.ETStep + ZERO < MD->CS.SolverStep);
    for (int i = 0; i < MD->CS.NumSteps; i++) {
        print_init(MD, fout->Init_update, t);
        tnext += MD->CS.SolverStep;
        while (t + ZERO < tnext) {
            double tout = tnext;
            if (etSubstepEnabled) tout = min(t + MD->CS.ETStep, tnext);
            MD->updateAllTimeSeries(t);
            MD->updateforcing(t);
            MD->ET(t, tout);
            if (MD->wbdiag != nullptr) MD->wbdiag->onETUpdate();
            rec_step_inputs(MD, t, tmp);
            const bool wbdiagOneStepEnabled = (MD->wbdiag != nullptr && MD->wbdiag->quadEnabled());
            if (wbdiagOneStepEnabled) {
                while (t + ZERO < tout) {
                    expect(next_state(fs, u, NY, &t), 2);          /* CVode(mem, tout, udata, &t, CV_ONE_STEP) */
                    f(t, u, du, MD);
                    rec_f(MD, t);
                    MD->wbdiag->onCvodeMonitorStep(t);
                }
            } else {
                expect(next_state(fs, u, NY, &t), 0);              /* CVode(mem, tout, udata, &t, CV_NORMAL) */
                f(t, u, du, MD);
                rec_f(MD, t);
            }
        }
        double unused;
        expect(next_state(fs, u, NY, &unused), 1);                 /* udata as CVode returned it */
        MD->summary(u);
        if (MD->wbdiag != nullptr) {
            f(t, u, du, MD);
            rec_f(MD, t);
            MD->wbdiag->sample(t, REF_DATA(du));
        }
        if (MD->wbdiag != nullptr) MD->wbdiag->maybeWrite(t);
        MD->CS.ExportResults(t);
        const double flood = MD->flood->FloodWarning(t);
        rec_export(MD, t, tmp);
        rec("flood", &flood, 1);
    }
    print_init(MD, fout->Init_update, t);
    fclose(fs);
    double n_ic = g_ic_copies;
    rec("ic_copies", &n_ic, 1);
    fclose(g_out);
    fflush(MD->flood->fid);
    for (int i = 0; i < MD->CS.NumPrint; i++) MD->CS.PCtrl[i].close_file();
    return 0;                                                    /* wbdiag's destructor closes its files */
}

int main(int argc, char **argv) {
    if (argc < 7) {
        fprintf(stderr, "usage: %s f|et|w OUT STATES|- N_ET THREADS <reference arguments>\n", argv[0]);
        return 2;
    }
    const std::string mode = argv[1];
    const char *out_path = argv[2], *states_path = argv[3];
    const int n_et = atoi(argv[4]);
    const int threads = atoi(argv[5]) > 0 ? atoi(argv[5]) : 1;
    argv[5] = argv[0];
    CommandIn CLI;
    FileIn *fin = new FileIn;
    FileOut *fout = new FileOut;
    CLI.parse(argc - 5, argv + 5);
    CLI.setFileIO(fin, fout);
    Model_Data *MD = new Model_Data(fin, fout);
    MD->loadinput();
    MD->CS.num_threads = threads;          /* loadinput() left max(NUM_OPENMP, -n) here */
    MD->initialize();
    MD->CheckInputData();
    fout->updateFilePath();
    const int NY = MD->NumY, NE = MD->NumEle, NR = MD->NumRiv, NL = MD->NumLake;
    globalY = new double[NY];
    double team = 1.;
#ifdef _OPENMP_ON
    omp_set_num_threads(MD->CS.num_threads);
    {
        const int want = MD->CS.num_threads;      /* the clause MD_f_omp.cpp's loops carry */
        int got = 0;
#pragma omp parallel num_threads(want)
        {
#pragma omp single
            got = omp_get_num_threads();
        }
        team = got;
    }
#endif
    N_Vector u = new_vec(NY), du = new_vec(NY);
    MD->LoadIC();
    MD->SetIC2Y(u);

    g_out = fopen(out_path, "wb");
    if (!g_out) { perror(out_path); return 2; }
    double dims[6] = {(double)NY, (double)NE, (double)NR, (double)NL, MD->CS.StartTime, MD->CS.ETStep};
    rec("dims", dims, 6);
    rec("threads", &team, 1);
    rec("y0", REF_DATA(u), NY);
    rec("ic_is", MD->yEleIS, NE);
    rec("ic_snow", MD->yEleSnow, NE);

    if (mode == "w") return run_writers(MD, fout, u, du, states_path);
    double t = MD->CS.StartTime;
    std::vector<double> tmp((size_t)NE);
    for (int s = 0; s < n_et; s++) {
        if (s) t += MD->CS.ETStep;
        MD->updateAllTimeSeries(t);
        MD->updateforcing(t);
        MD->ET(t, t + MD->CS.ETStep);
        if (mode == "et") {
            rec("t", &t, 1);
            rec("t_prcp", MD->t_prcp, NE);
            rec("t_temp", MD->t_temp, NE);
            rec("t_rn", MD->t_rn, NE);
            rec("rn_factor", MD->ele_rn_factor, MD->ele_rn_factor ? NE : 0);
            rec("qEleNetPrep", MD->qEleNetPrep, NE);
            rec("qPotEvap", MD->qPotEvap, NE);
            rec("qPotTran", MD->qPotTran, NE);
            rec("qEleETP", MD->qEleETP, NE);
            rec("t_lai", MD->t_lai, NE);
            rec("fu_surf", MD->fu_Surf, NE);
            rec("fu_sub", MD->fu_Sub, NE);
            rec("yEleIS", MD->yEleIS, NE);
            rec("yEleSnow", MD->yEleSnow, NE);
            rec("qEleE_IC", MD->qEleE_IC, NE);
        }
    }
    if (mode == "f") {
        rec("t", &t, 1);
        rec("net_prep", MD->qEleNetPrep, NE);
        rec("pot_evap", MD->qPotEvap, NE);
        rec("pot_tran", MD->qPotTran, NE);
        rec("etp", MD->qEleETP, NE);
        rec("lai", MD->t_lai, NE);
        rec("fu_surf", MD->fu_Surf, NE);
        rec("fu_sub", MD->fu_Sub, NE);
        rec("e_ic", MD->qEleE_IC, NE);
        for (int i = 0; i < NE; i++) tmp[(size_t)i] = MD->Ele[i].u_satn;
        rec("u_satn", tmp.data(), NE);
        rec("ugw_stale", uYgw, NE);
        rec("prcp", MD->qElePrep, NE);
        if (MD->ieBC1 && MD->NumBCEle1 > 0) rec_tsd("ele_ybc", MD->tsd_eyBC, t);
        if (MD->ieBC2 && MD->NumBCEle2 > 0) rec_tsd("ele_qbc", MD->tsd_eqBC, t);
        if (MD->irBC1 && MD->NumBCRiv1 > 0) rec_tsd("riv_ybc", MD->tsd_ryBC, t);
        if (MD->irBC2 && MD->NumBCRiv2 > 0) rec_tsd("riv_qbc", MD->tsd_rqBC, t);
        FILE *fs = fopen(states_path, "rb");
        if (!fs) { perror(states_path); return 2; }
        int k = 0;
        char name[16];
        while (fread(REF_DATA(u), sizeof(double), (size_t)NY, fs) == (size_t)NY) {
            f(t, u, du, MD);
            snprintf(name, sizeof name, "dy%d", k++);
            rec(name, REF_DATA(du), NY);
        }
        fclose(fs);
        double kk = k;
        rec("ncalls", &kk, 1);
    }
    fclose(g_out);
    return 0;
}
