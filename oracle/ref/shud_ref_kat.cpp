/* shud_ref_kat.cpp — ref_kat(which, x, n, out): the REFERENCE model's own leaf functions on n input tuples, with
 * oracle_kat()'s signature, ids and argument order (oracle/shud_oracle.c, tests/kat_grids.py).  This file is ours
 * and only dispatches; the functions are the reference's, compiled in place by `make -C oracle ref` into
 * oracle/_ref/libshud_ref_kat.so.  The reference's leaves may call exit() on out-of-range values, so the library
 * is loaded in a child process only (oracle/ref/refio.py).
 * WeirFlow_jtoi is a private member of Model_Data that reads no member: this unit alone is compiled with
 * `private` read as `public`.  The river geometry goes through _River::updateRiver, as f_update calls it. */
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
#define private public
#define protected public
#include "Model_Data.hpp"
#include "Equations.hpp"
#include "functions.hpp"
#include "is_sm_et.hpp"
#include "Flux_RiverElement.hpp"
#include "River.hpp"
#undef private
#undef protected

double *uYsf, *uYus, *uYgw, *uYriv, *uYlake, *globalY;
double timeNow;
int dummy_mode = 0, global_fflush_mode = 0, global_implicit_mode = 1, global_verbose_mode = 1, lakeon = 0;

static const int nin_tab[11] = {4, 6, 8, 8, 2, 3, 3, 4, 4, 4, 4};

extern "C" int ref_kat_nin(int fn) {
    if (fn >= 0 && fn < 11) return nin_tab[fn];
    return fn == 100 ? 6 : fn == 101 ? 8 : fn == 102 ? 4 : -1;
}

extern "C" int ref_kat(int fn, const double *in, int n, double *out) {
    const int k = ref_kat_nin(fn);
    if (k < 0) return -1;
    static Model_Data *md = new Model_Data();      /* empty: WeirFlow_jtoi reads no member */
    for (int t = 0; t < n; t++) {
        const double *x = in + (size_t)t * k;
        double r = 0.;
        if (fn >= 7 && fn <= 10) {
            _River rv;
            rv.BottomWidth = x[0];
            rv.bankslope = x[1];
            rv.Length = x[2];
            rv.updateRiver(x[3]);
            r = fn == 7 ? rv.u_CSarea : fn == 8 ? rv.u_CSperem : fn == 9 ? rv.u_topWidth : rv.u_TopArea;
        } else {
            switch (fn) {
                case 0: r = ManningEquation(x[0], x[1], x[2], x[3]); break;
                case 1: r = effKH(x[0], x[1], x[2], x[3], x[4], x[5]); break;
                case 2: r = md->WeirFlow_jtoi(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]); break;
                case 3: r = flux_R2E_GW(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]); break;
                case 4: r = satKfun(x[0], x[1]); break;
                case 5: r = SoilMoistureStress(x[0], x[1], x[2]); break;
                case 6: r = fun_dAtodY(x[0], x[1], x[2]); break;
                case 100: r = PET_PM_openwater(x[0], x[1], x[2], x[3], x[4], x[5]); break;
                case 101: r = PET_Penman_Monteith(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]); break;
                case 102: r = AerodynamicResistance(x[0], x[1], x[2], x[3]); break;
            }
        }
        out[t] = r;
    }
    return 0;
}
