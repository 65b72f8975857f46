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

int main(int argc, char **argv) {
    if (argc < 7) {
        fprintf(stderr, "usage: %s f|et OUT STATES|- N_ET THREADS <reference arguments>\n", argv[0]);
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
