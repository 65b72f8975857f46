// shud_wb.hip — water-balance diagnostics on the device (include/shud_wb.h): the reference's WaterBalanceDiag
// (src/Model/WaterBalanceDiag.cpp) over the arrays the RHS handle already keeps in HBM.
//
// sample (:410-529) is one fused pass, one lane per element: it loads DY, Sy, area, the step inputs, ic_raw, the ET
// components, the lateral totals and the six edge-major flux planes, forms the four per-element rates in the
// reference's operation order and read-modify-writes the four accumulators (the previous-rate arrays exist only
// in trapezoid mode).  The basin sums go through the project's one two-level deterministic reduction, shared with
// the integrator: shud_reduce.h is the single statement of the summation order (block_partial per workgroup and
// quantity, ordered_total per quantity in the one-block finalize), pinned for these sums bit for bit by
// tests/test_gpu_wb.py::test_reduction_edges and tests/test_gpu_wb_quad.py::test_rates_reduction_edges against
// tests/ode_kernels_py.py device_order_sum.  The finalize then applies acc += rate*dt (or the trapezoid rule) to
// the seven basin accumulators on the device.  A pass over the reaches gives the outlet discharge (:197-230), the
// reach boundary-condition inflow and the river storage (:183-195) the same way.
// maybeWrite (:531-636) runs a residual pass at interval ends (four residual arrays, storage snapshots rolled,
// accumulators zeroed, basin element storage reduced); only then do 4 NE + 9 doubles cross PCIe, synchronously
// (once per output interval), and are written in the reference's byte layout (:90-150).
//
// Bytes per element of the sample pass, counted from its loads and stores: DY 24, Sy + area 16, qElePrep +
// qEleNetPrep 16, ic_raw 8, qEs..qTg 40, QeleSurfTot + QeleSubTot 16, flags 4, QeleSurf + QeleSub 48, four
// accumulators read and written 64 = 236 B (trapezoid mode: + 64 for the four previous rates).
//
// The quad monitor (SHUD_WB_DIAG_QUAD; onCvodeMonitorStep :681-717 on the basin rates f() forms, MD_f.cpp:57-86,
// 115-128,193-213) is a rates-only pass after every internal step of the integrator: k_wb_quad loads area, the
// flag word, qElePrep, ic_raw, qEs..qTg and the six edge planes (8 + 4 + 8 + 8 + 40 + 48 = 116 B per element,
// nothing stored per element), k_wb_quad_river copies QrivDown at the outlets and the reach boundary inflow (no
// geometry, no Manning), both through block_partial into the sample's partial buffers (stream-ordered), and
// finalize mode 3 forms the seven rates in the sample's order and applies Euler on the first integrating step, the
// trapezoid on every later one, to device scalars of its own (d_qs).  Finalize mode 1 forms the quad row beside
// the basin row and zeroes the quad accumulators.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "shud_diag_host.h"
#include "shud_handle.h"
#include "shud_out.h"
#include "shud_physics.h"
#include "shud_reduce.h"
#include "shud_wb.h"

namespace {

using namespace shud::red;           // every element / reach pass: one entry per thread on its kRedThreads grid
// element-pass partials, reach-pass partials
enum { EQ_P = 0, EQ_ET, EQ_QBC, EQ_QSS, EQ_NONCONS, EQ_QEDGE, EQ_N };
enum { RQ_QOUT = 0, RQ_RBC, RQ_STOR, RQ_N };
// device scalars
enum { S_RATE = 0, S_PREV = S_RATE + SHUD_WB_NBASIN, S_ACC = S_PREV + SHUD_WB_NBASIN, S_ROW = S_ACC + SHUD_WB_NBASIN,
       S_STOR_PREV = S_ROW + 9, S_STOR = S_STOR_PREV + 2, S_COUNT = S_STOR + 2 };
// device scalars of the quad monitor (an array of their own, allocated by shud_wb_quad_enable)
enum { Q_RATE = 0, Q_PREV = Q_RATE + SHUD_WB_NBASIN, Q_ACC = Q_PREV + SHUD_WB_NBASIN, Q_ROW = Q_ACC + SHUD_WB_NBASIN,
       Q_COUNT = Q_ROW + 9 };
// element flags word: bits 0-15 iBC (int16), bits 16-18 edge j has no neighbour (domain boundary), bit 19 iSS != 0
constexpr int kFlagEdge = 16, kFlagSS = 19;
// reach flags: bit 0 outlet (down < 0, not into a lake), bit 1 critical-depth outlet (down == -4)
constexpr int kRivOutlet = 1, kRivCrit = 2;

// the element's six basin terms (sample :472-489; the monitor's f(), MD_f.cpp:57-86,115-128), one place as in the
// reference: qe[j] is QeleSurf + QeleSub of edge j, eqbc the element's boundary-condition flux (0.0 unless iBC < 0)
__device__ __forceinline__ void basin_terms(double area, int fl, double prcp, double ic, double es, double eu,
                                            double eg, double tu, double tg, const double (&qe)[3], double eqbc,
                                            double (&v)[EQ_N]) {
    v[EQ_P] = prcp * area;
    v[EQ_ET] = (ic + es + eu + eg + tu + tg) * area;
    v[EQ_QBC] = eqbc;
    v[EQ_QSS] = 0.0;                                                   // QSS where iSS != 0: always 0.0
    double nc = 0.0, qedge = 0.0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        if ((fl >> (kFlagEdge + j)) & 1) qedge += qe[j];
        else nc += qe[j];
    }
    v[EQ_NONCONS] = nc;
    v[EQ_QEDGE] = qedge;
}

struct SampleArgs {
    int n;
    const double *dy, *sy, *area;
    const int *flags;
    const double *prcp, *netp, *ic, *es, *eu, *eg, *tu, *tg, *stot, *btot, *qs, *qb, *eqbc;
    double *acc[4], *prev[4];        // net3, netfull, net3_budget, netfull_budget; prev: trapezoid mode only
    double dt;
    int trapz, has_prev;             // prev arrays exist (stored every sample); and hold a previous rate
    double *part;
    int nblk;
};

// WaterBalanceDiag::sample, the per-element loop (:425-463) and the element half of the basin loop (:472-489)
__global__ void __launch_bounds__(kRedThreads) k_wb_sample(SampleArgs a) {
    const int i = blockIdx.x * kRedThreads + threadIdx.x;
    double v[EQ_N] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < a.n) {
        const size_t n = (size_t)a.n;
        const double dsf = ldn(a.dy + i), dus = ldn(a.dy + n + i), dgw = ldn(a.dy + 2 * n + i);
        const double sy = a.sy[i], area = a.area[i];
        const int fl = a.flags[i];
        const double prcp = a.prcp[i], netp = a.netp[i], ic = a.ic[i];
        const double es = ldn(a.es + i), eu = ldn(a.eu + i), eg = ldn(a.eg + i), tu = ldn(a.tu + i), tg = ldn(a.tg + i);
        const double stot = ldn(a.stot + i), btot = ldn(a.btot + i);
        double qe[3];
#pragma unroll
        for (int j = 0; j < 3; j++) qe[j] = ldn(a.qs + j * n + i) + ldn(a.qb + j * n + i);
        const int ibc = (int)(int16_t)(fl & 0xffff);
        const bool ss = (fl >> kFlagSS) & 1;
        const double QBC = ibc < 0 ? a.eqbc[-ibc] : 0.0;

        const double net3 = dsf + sy * dus + sy * dgw;
        const double netfull = net3 + (prcp - netp) - ic;
        const double et3 = es + eu + eg + tu + tg;
        const double qlat3 = (stot + btot) / area;
        const double qbc = ibc < 0 ? QBC / area : 0.0;
        const double qss = ss ? shud::zero_over(area) : 0.0;           // QSS is never assigned: 0.0 / area
        const double net3_b = netp - et3 - qlat3 + qbc + qss;
        const double netfull_b = prcp - (ic + et3) - qlat3 + qbc + qss;
        const double rate[4] = {net3, netfull, net3_b, netfull_b};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            double acc = ldn(a.acc[k] + i);
            if (a.trapz) {
                if (a.has_prev) acc += 0.5 * (ldn(a.prev[k] + i) + rate[k]) * a.dt;
                else acc += rate[k] * a.dt;
                stn(a.prev[k] + i, rate[k]);
            } else {
                acc += rate[k] * a.dt;
            }
            stn(a.acc[k] + i, acc);
        }
        basin_terms(area, fl, prcp, ic, es, eu, eg, tu, tg, qe, QBC, v);
    }
    block_partial<EQ_N>(v, 0u, a.part, a.nblk);
}

struct RivArgs {
    int nr;
    const double *stage;             // yRivStg (SHUD_ARR_Y_RIV_STG)
    const int *flags, *bc;
    const double *bw, *bs, *len, *slope, *rough, *rqbc;
    double *part;
    int nblk;
};

// basinOutletDischarge_m3min (:197-230), the reach half of the boundary-condition sum (:490-494) and
// basinRiverStorage_m3 (:183-195), one lane per reach
__global__ void __launch_bounds__(kRedThreads) k_wb_river(RivArgs a) {
    const int r = blockIdx.x * kRedThreads + threadIdx.x;
    double v[RQ_N] = {0.0, 0.0, 0.0};
    if (r < a.nr) {
        const double stage = a.stage[r], len = a.len[r];
        const shud::RivGeom g = shud::riv_geom(a.bw[r], a.bs[r], len, stage);     // updateRiver(stage), clamped at 0
        const int fl = a.flags[r];
        if (fl & kRivOutlet) {
            if (fl & kRivCrit) {
                v[RQ_QOUT] = g.csarea * sqrt(K_GRAV * stage) * 60.0;
            } else {
                const double R = (g.csperem <= 0.0) ? 0.0 : (g.csarea / g.csperem);
                const double s = a.slope[r] + stage * 2.0 / len;
                v[RQ_QOUT] = shud::manning(g.csarea, a.rough[r], R, s);
            }
        }
        const int bc = a.bc[r];
        if (bc < 0) v[RQ_RBC] = a.rqbc[-bc];
        v[RQ_STOR] = g.csarea * len;
    }
    block_partial<RQ_N>(v, 0u, a.part, a.nblk);
}

struct QuadArgs {
    int n;
    const double *area;
    const int *flags;
    const double *prcp, *ic, *es, *eu, *eg, *tu, *tg, *qs, *qb, *eqbc;
    double *part;
    int nblk;
};

// the element half of the basin rates f() forms for the monitor (MD_f.cpp:57-86,115-128): k_wb_sample's basin terms
// without its per-element rates and accumulators.  Lanes past n carry 0.0 to the barrier in block_partial.
__global__ void __launch_bounds__(kRedThreads) k_wb_quad(QuadArgs a) {
    const int i = blockIdx.x * kRedThreads + threadIdx.x;
    double v[EQ_N] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < a.n) {
        const size_t n = (size_t)a.n;
        const double area = a.area[i];
        const int fl = a.flags[i];
        const double prcp = a.prcp[i], ic = a.ic[i];
        const double es = ldn(a.es + i), eu = ldn(a.eu + i), eg = ldn(a.eg + i), tu = ldn(a.tu + i), tg = ldn(a.tg + i);
        double qe[3];
#pragma unroll
        for (int j = 0; j < 3; j++) qe[j] = ldn(a.qs + j * n + i) + ldn(a.qb + j * n + i);
        const int ibc = (int)(int16_t)(fl & 0xffff);
        basin_terms(area, fl, prcp, ic, es, eu, eg, tu, tg, qe, ibc < 0 ? a.eqbc[-ibc] : 0.0, v);
    }
    block_partial<EQ_N>(v, 0u, a.part, a.nblk);
}

struct QuadRivArgs {
    int nr;
    const int *flags, *bc;
    const double *qdown, *rqbc;      // QrivDown of the monitor's f() (DevDiag), the reach flux table
    double *part;
    int nblk;
};

// the reach half (MD_f.cpp:193-205): QrivDown as f() computed it where the reach is an outlet, qBC where BC < 0;
// partial slots RQ_QOUT and RQ_RBC
__global__ void __launch_bounds__(kRedThreads) k_wb_quad_river(QuadRivArgs a) {
    const int r = blockIdx.x * kRedThreads + threadIdx.x;
    double v[2] = {0.0, 0.0};
    if (r < a.nr) {
        if (a.flags[r] & kRivOutlet) v[RQ_QOUT] = ldn(a.qdown + r);
        const int bc = a.bc[r];
        if (bc < 0) v[RQ_RBC] = a.rqbc[-bc];
    }
    block_partial<2>(v, 0u, a.part, a.nblk);
}

struct ResidArgs {
    int n;
    const double *sy, *area, *ysf, *yus, *ygw, *snow, *is;   // snow / is: nullptr reads as 0.0
    double *acc[4], *res[4], *s3_prev, *sfull_prev;
    int init;                        // 1: only the snapshots (openFiles :297-302)
    double *part;
    int nblk;
};

// maybeWrite's element loop (:553-569) and basinElementStorageFull_m3 (:168-181)
__global__ void __launch_bounds__(kRedThreads) k_wb_resid(ResidArgs a) {
    const int i = blockIdx.x * kRedThreads + threadIdx.x;
    double v[1] = {0.0};
    if (i < a.n) {
        const double sy = a.sy[i];
        const double snow = a.snow ? a.snow[i] : 0.0, is = a.is ? a.is[i] : 0.0;
        const double s3 = a.ysf[i] + sy * a.yus[i] + sy * a.ygw[i];
        const double sfull = s3 + snow + is;
        if (!a.init) {
            const double p3 = a.s3_prev[i], pf = a.sfull_prev[i];
            stn(a.res[0] + i, s3 - p3 - ldn(a.acc[0] + i));
            stn(a.res[1] + i, sfull - pf - ldn(a.acc[1] + i));
            stn(a.res[2] + i, s3 - p3 - ldn(a.acc[2] + i));
            stn(a.res[3] + i, sfull - pf - ldn(a.acc[3] + i));
#pragma unroll
            for (int k = 0; k < 4; k++) stn(a.acc[k] + i, 0.0);
        }
        a.s3_prev[i] = s3;
        a.sfull_prev[i] = sfull;
        v[0] = sfull * a.area[i];                                      // depth * area, depth == sfull bit for bit
    }
    block_partial<1>(v, 0u, a.part, a.nblk);
}

__global__ void __launch_bounds__(256) k_wb_ic(int n, const double *__restrict__ src, int stride, double *__restrict__ ic) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ic[i] = src[(size_t)i * stride];
}

struct FinArgs {
    const double *epart, *rpart;
    int ne_q, nblk_e, nr_q, nblk_r;  // quantities and partials per quantity of the element / reach pass
    int mode;                        // 0 sample, 1 write, 2 initial snapshot, 3 quad monitor step
    int open, trapz, has_prev;
    double dt;
    double *s;                       // device scalars [S_COUNT]
    double *qs;                      // quad scalars [Q_COUNT]; nullptr: the monitor is off
};
static_assert(RQ_QOUT == 0 && RQ_RBC == 1, "k_wb_quad_river fills the first two reach partial slots");

// the total of every quantity by ordered_total (shud_reduce.h), then the scalar update by thread 0
__global__ void __launch_bounds__(kFinThreads) k_wb_finalize(FinArgs f) {
    __shared__ double sm[kFinThreads / 64];
    __shared__ double tot[EQ_N + RQ_N];
    const int nq = f.ne_q + f.nr_q;
    for (int q = 0; q < nq; ++q) {
        const bool ele = q < f.ne_q;
        const int nblk = ele ? f.nblk_e : f.nblk_r;
        const double *pp = ele ? f.epart + (size_t)q * nblk : f.rpart + (size_t)(q - f.ne_q) * nblk;
        const double y = ordered_total(pp, nblk, false, sm);
        if (threadIdx.x == 0) tot[q] = y;
    }
    if (threadIdx.x != 0) return;
    double *s = f.s;
    const double *rt = tot + f.ne_q;
    if (f.mode == 0 || f.mode == 3) {   // sample :496-524; the monitor's rates (MD_f.cpp:206-213) and step :702-715
        double rate[SHUD_WB_NBASIN];
        rate[SHUD_WB_P] = tot[EQ_P];
        rate[SHUD_WB_ET] = tot[EQ_ET];
        rate[SHUD_WB_QOUT] = rt[RQ_QOUT];
        rate[SHUD_WB_QEDGE] = f.open ? tot[EQ_QEDGE] : 0.0;           // 0 under CloseBoundary (:237-239)
        rate[SHUD_WB_QBC] = tot[EQ_QBC] + rt[RQ_RBC];
        rate[SHUD_WB_QSS] = tot[EQ_QSS];
        rate[SHUD_WB_NONCONS] = tot[EQ_NONCONS];
        if (f.mode == 3) {           // Euler on the first integrating step, then the trapezoid: no trapz switch here
            double *q = f.qs;
            for (int k = 0; k < SHUD_WB_NBASIN; k++) {
                if (f.has_prev) q[Q_ACC + k] += 0.5 * (q[Q_PREV + k] + rate[k]) * f.dt;
                else q[Q_ACC + k] += rate[k] * f.dt;
                q[Q_PREV + k] = rate[k];
                q[Q_RATE + k] = rate[k];
            }
            return;
        }
        for (int k = 0; k < SHUD_WB_NBASIN; k++) {
            if (f.trapz && f.has_prev) s[S_ACC + k] += 0.5 * (s[S_PREV + k] + rate[k]) * f.dt;
            else s[S_ACC + k] += rate[k] * f.dt;
            s[S_PREV + k] = rate[k];
            s[S_RATE + k] = rate[k];
        }
    } else {
        const double s_ele = tot[0], s_riv = rt[RQ_STOR];
        if (f.mode == 1) {           // maybeWrite :577-633
            const double ds_ele = s_ele - s[S_STOR_PREV], ds_riv = s_riv - s[S_STOR_PREV + 1];
            const double ds_total = ds_ele + ds_riv;
            const double *A = s + S_ACC;
            const double net = A[SHUD_WB_P] + A[SHUD_WB_QBC] + A[SHUD_WB_QSS] - A[SHUD_WB_ET] - A[SHUD_WB_QOUT] -
                               A[SHUD_WB_QEDGE];
            s[S_ROW] = ds_total;
            for (int k = 0; k < SHUD_WB_NBASIN; k++) s[S_ROW + 1 + k] = A[k];
            s[S_ROW + 8] = ds_total - net;
            for (int k = 0; k < SHUD_WB_NBASIN; k++) s[S_ACC + k] = 0.0;
            if (f.qs) {              // the quad row :597-623: the same ds_total; the previous quad rates are kept
                double *q = f.qs;
                const double *B = q + Q_ACC;
                const double qnet = B[SHUD_WB_P] + B[SHUD_WB_QBC] + B[SHUD_WB_QSS] - B[SHUD_WB_ET] - B[SHUD_WB_QOUT] -
                                    B[SHUD_WB_QEDGE];
                q[Q_ROW] = ds_total;
                for (int k = 0; k < SHUD_WB_NBASIN; k++) q[Q_ROW + 1 + k] = B[k];
                q[Q_ROW + 8] = ds_total - qnet;
                for (int k = 0; k < SHUD_WB_NBASIN; k++) q[Q_ACC + k] = 0.0;
            }
        }
        s[S_STOR_PREV] = s_ele;
        s[S_STOR_PREV + 1] = s_riv;
        s[S_STOR] = s_ele;
        s[S_STOR + 1] = s_riv;
    }
}

int blocks(int n) { return n > 0 ? (n + kRedThreads - 1) / kRedThreads : 0; }

}  // namespace

struct shud_wb {
    shud_rhs *h = nullptr;
    int NE = 0, NR = 0;
    bool open = false, trapz = false;
    int interval = 0;
    double last_t = 0.0;
    bool has_prev_rate = false;
    long long last_written_floor = -1;
    int64_t rows = 0;
    int n_outlets = 0;
    std::vector<void *> allocs;
    double *d_sy = nullptr, *d_area = nullptr, *d_ic = nullptr;
    int *d_flags = nullptr, *d_rflags = nullptr, *d_rbc = nullptr;
    double *d_rbw = nullptr, *d_rbs = nullptr, *d_rlen = nullptr, *d_rslope = nullptr, *d_rrough = nullptr;
    double *d_acc[4] = {}, *d_prev[4] = {}, *d_res[4] = {}, *d_s3 = nullptr, *d_sfull = nullptr;
    double *d_epart = nullptr, *d_rpart = nullptr, *d_s = nullptr;
    int nblk_e = 0, nblk_r = 0;
    double *h_row = nullptr;         // pinned: max(NE, S_COUNT) doubles (one residual array at a time, or the scalars)
    FILE *fp[6] = {};                // [5]: basinwbfull_quad.dat (shud_wb_quad_enable)
    std::string fname[6];
    int werr = 0;
    std::string werr_msg;
    // quad monitor: quad_enabled, quad_last_t, quad_has_prev_rate; the scalars [Q_COUNT]; what its header repeats
    bool quad = false, quad_has_prev = false, sampled = false;
    double quad_last_t = 0.0;
    double *d_qs = nullptr;
    ShudWbOptions hdr{};
    std::string hdr_mode, prefix;
    bool have_prefix = false;

    template <class T>
    int dalloc(T **p, size_t n, const T *src = nullptr) {
        void *q = nullptr;
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        HIP_TRY(hipMalloc(&q, bytes));
        allocs.push_back(q);
        *p = (T *)q;
        if (src && n) HIP_TRY(hipMemcpy(q, src, n * sizeof(T), hipMemcpyHostToDevice));
        else HIP_TRY(hipMemset(q, 0, bytes));
        return 0;
    }
};

static void wb_free(shud_wb *w) {
    for (FILE *f : w->fp)
        if (f) fclose(f);
    for (void *p : w->allocs) (void)hipFree(p);
    if (w->h_row) (void)hipHostFree(w->h_row);
    delete w;
}

static void wb_werr(shud_wb *w, const std::string &msg) {
    if (!w->werr) { w->werr = SHUD_WB_ERR_IO; w->werr_msg = msg; }
}

// writeDatHeader (:90-130)
static void wb_header(shud_wb *w, int k, const char *label, int num_var, const ShudWbOptions *o) {
    std::vector<double> icol((size_t)num_var);
    for (int i = 0; i < num_var; i++) icol[(size_t)i] = (double)(i + 1);
    if (!shud::write_dat_preamble(w->fp[k], label, o->radiation_input_mode, o->terrain_radiation, o->solar_lonlat_mode,
                                  o->solar_lon_deg, o->solar_lat_deg, (double)o->forc_start_time, num_var, icol.data()))
        wb_werr(w, "write error on " + w->fname[k]);
}

// writeDatRecord (:132-150)
static void wb_record(shud_wb *w, int k, double t, int num_var, const double *values) {
    FILE *fp = w->fp[k];
    if (!fp) return;
    bool ok = fwrite(&t, sizeof(double), 1, fp) == 1;
    if (num_var > 0) ok = ok && fwrite(values, sizeof(double), (size_t)num_var, fp) == (size_t)num_var;
    if (!ok) wb_werr(w, "write error on " + w->fname[k]);
}

static int wb_launch_river(shud_wb *w) {
    shud_rhs *h = w->h;
    if (w->NR <= 0) return 0;
    RivArgs a{w->NR, h->d_sum[3], w->d_rflags, w->d_rbc, w->d_rbw, w->d_rbs, w->d_rlen, w->d_rslope, w->d_rrough,
              h->dm.rqbc, w->d_rpart, w->nblk_r};
    hipLaunchKernelGGL(k_wb_river, dim3(w->nblk_r), dim3(kRedThreads), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the residual / snapshot pass, the reach pass and their finalize (mode 1 write, 2 initial snapshot)
static int wb_launch_storage(shud_wb *w, int mode) {
    shud_rhs *h = w->h;
    if (!h->d_sum[0] || !h->d_sum[1] || !h->d_sum[2] || (w->NR > 0 && !h->d_sum[3]))
        return shud_fail(SHUD_ERR_ARG, "shud_wb: the summary arrays are not filled (call shud_rhs_summary first)");
    ResidArgs a{};
    a.n = w->NE; a.sy = w->d_sy; a.area = w->d_area;
    a.ysf = h->d_sum[0]; a.yus = h->d_sum[1]; a.ygw = h->d_sum[2];
    a.snow = shud_et_array(h, SHUD_ARR_Y_ELE_SNOW); a.is = shud_et_array(h, SHUD_ARR_Y_ELE_IS);
    for (int k = 0; k < 4; k++) { a.acc[k] = w->d_acc[k]; a.res[k] = w->d_res[k]; }
    a.s3_prev = w->d_s3; a.sfull_prev = w->d_sfull;
    a.init = mode == 2;
    a.part = w->d_epart; a.nblk = w->nblk_e;
    hipLaunchKernelGGL(k_wb_resid, dim3(w->nblk_e), dim3(kRedThreads), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    int rc = wb_launch_river(w);
    if (rc) return rc;
    FinArgs f{w->d_epart, w->d_rpart, 1, w->nblk_e, RQ_N, w->nblk_r, mode, w->open ? 1 : 0, 0, 0, 0.0, w->d_s,
              w->quad ? w->d_qs : nullptr};
    hipLaunchKernelGGL(k_wb_finalize, dim3(1), dim3(kFinThreads), 0, h->stream, f);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int shud_wb_create(shud_rhs_t h, const ShudMeshSoA *m, const ShudParamsSoA *par, const ShudWbOptions *o,
                              shud_wb_t *out) {
    if (!h || !m || !par || !o || !out) return shud_fail(SHUD_ERR_ARG, "null argument");
    *out = nullptr;
    if (h->mode != SHUD_MODE_SERIAL)
        return shud_fail(SHUD_ERR_UNSUPPORTED, "shud_wb: OMP-semantics handles are not supported (the per-element ET "
                                               "terms exist only in the serial path)");
    if (h->ordered)
        return shud_fail(SHUD_ERR_UNSUPPORTED, "shud_wb: ordered handles are not supported (the basin sums would run in "
                                               "another element order, include/shud_order.h)");
    if (h->lakeon || m->num_lake > 0)
        return shud_fail(SHUD_ERR_UNSUPPORTED, "shud_wb: lake models are not supported (the reference's diagnostic "
                                               "ignores lake storage)");
    if (h->partitioned) return shud_fail(SHUD_ERR_UNSUPPORTED, "shud_wb: partitioned handles are not supported");
    if (m->num_ele != h->NE || m->num_riv != h->NR || m->num_ele < 1)
        return shud_fail(SHUD_ERR_ARG, "shud_wb: the mesh is not the handle's (%d / %d elements, %d / %d reaches)",
                         m->num_ele, h->NE, m->num_riv, h->NR);
    if (o->interval_min <= 0) return shud_fail(SHUD_ERR_ARG, "shud_wb: interval_min must be positive");
    if (!m->area || !m->nabr || !par->Sy) return shud_fail(SHUD_ERR_ARG, "shud_wb: mesh arrays missing");
    HIP_TRY(hipSetDevice(h->device));
    const int NE = m->num_ele, NR = m->num_riv;
    std::vector<int> flags((size_t)NE), rflags((size_t)std::max(NR, 1), 0), rbc((size_t)std::max(NR, 1), 0);
    for (int i = 0; i < NE; i++) {
        const int ibc = m->ibc ? m->ibc[i] : 0;
        if (ibc < -32768 || ibc > 32767) return shud_fail(SHUD_ERR_ARG, "shud_wb: iBC column %d out of range", ibc);
        if (ibc < 0 && -ibc > h->max_col[1])
            return shud_fail(SHUD_ERR_ARG, "shud_wb: iBC column %d beyond the handle's flux table", ibc);
        int f = ibc & 0xffff;
        for (int j = 0; j < 3; j++)
            if (m->nabr[(size_t)j * NE + i] < 0) f |= 1 << (kFlagEdge + j);
        if (m->iss && m->iss[i] != 0) f |= 1 << kFlagSS;
        flags[(size_t)i] = f;
    }
    std::vector<int> outlets;                                           // initBasinOutlets (:152-166)
    for (int r = 0; r < NR; r++) {
        if (m->riv_down[r] < 0) {
            outlets.push_back(r);
            rflags[(size_t)r] = kRivOutlet | (m->riv_down[r] == -4 ? kRivCrit : 0);
        }
        rbc[(size_t)r] = m->riv_bc ? m->riv_bc[r] : 0;
        if (rbc[(size_t)r] < 0 && -rbc[(size_t)r] > h->max_col[3])
            return shud_fail(SHUD_ERR_ARG, "shud_wb: reach BC column %d beyond the handle's flux table", rbc[(size_t)r]);
    }
    int rc = shud_ensure_diag(h);
    if (rc) return rc;
    shud_wb *w = new shud_wb;
    w->h = h; w->NE = NE; w->NR = NR;
    w->open = m->close_boundary == 0;
    w->trapz = o->trapz != 0;
    w->interval = o->interval_min;
    w->last_t = w->quad_last_t = o->start_time;
    w->hdr = *o;
    w->hdr_mode = o->solar_lonlat_mode ? o->solar_lonlat_mode : "";
    w->hdr.solar_lonlat_mode = w->hdr_mode.c_str();
    w->have_prefix = o->prefix != nullptr;
    w->prefix = o->prefix ? o->prefix : "";
    w->hdr.prefix = nullptr;
    w->n_outlets = (int)outlets.size();
    w->nblk_e = blocks(NE); w->nblk_r = blocks(NR);
    const size_t E = (size_t)NE, R = (size_t)NR;
    auto fail = [&](int code) { wb_free(w); return code; };
    if ((rc = w->dalloc(&w->d_sy, E, par->Sy)) || (rc = w->dalloc(&w->d_area, E, m->area)) ||
        (rc = w->dalloc(&w->d_flags, E, flags.data())) || (rc = w->dalloc(&w->d_ic, E)) ||
        (rc = w->dalloc(&w->d_rflags, R, rflags.data())) || (rc = w->dalloc(&w->d_rbc, R, rbc.data())) ||
        (rc = w->dalloc(&w->d_rbw, R, m->riv_bottom_width)) || (rc = w->dalloc(&w->d_rbs, R, m->riv_bankslope)) ||
        (rc = w->dalloc(&w->d_rlen, R, m->riv_length)) || (rc = w->dalloc(&w->d_rslope, R, m->riv_bed_slope)) ||
        (rc = w->dalloc(&w->d_rrough, R, m->riv_avg_rough)) || (rc = w->dalloc(&w->d_s3, E)) ||
        (rc = w->dalloc(&w->d_sfull, E)) || (rc = w->dalloc(&w->d_epart, (size_t)EQ_N * w->nblk_e)) ||
        (rc = w->dalloc(&w->d_rpart, (size_t)RQ_N * std::max(w->nblk_r, 1))) || (rc = w->dalloc(&w->d_s, (size_t)S_COUNT)))
        return fail(rc);
    for (int k = 0; k < 4; k++) {
        if ((rc = w->dalloc(&w->d_acc[k], E)) || (rc = w->dalloc(&w->d_res[k], E))) return fail(rc);
        if (w->trapz && (rc = w->dalloc(&w->d_prev[k], E))) return fail(rc);
    }
    if (hipHostMalloc((void **)&w->h_row, std::max<size_t>(o->prefix ? E : 1, S_COUNT) * sizeof(double),
                      hipHostMallocDefault) != hipSuccess) {
        w->h_row = nullptr;
        return fail(shud_fail(SHUD_ERR_HIP, "shud_wb: hipHostMalloc failed"));
    }
    // initial storage snapshots (:296-302, 341-342)
    if ((rc = wb_launch_storage(w, 2))) return fail(rc);
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(shud_fail(SHUD_ERR_HIP, "shud_wb: snapshot failed"));
    if (o->prefix) {
        static const char *ext[5] = {".elewb3_resid.dat", ".elewbfull_resid.dat", ".elewb3_budget_resid.dat",
                                     ".elewbfull_budget_resid.dat", ".basinwbfull.dat"};
        static const char *label[5] = {"elewb3_resid", "elewbfull_resid", "elewb3_budget_resid",
                                       "elewbfull_budget_resid", "basinwbfull (m3)"};
        for (int k = 0; k < 5; k++) {
            w->fname[k] = std::string(o->prefix) + ext[k];
            w->fp[k] = fopen(w->fname[k].c_str(), "wb");
            if (!w->fp[k]) {
                rc = shud_fail(SHUD_WB_ERR_IO, "shud_wb_create: cannot open %s", w->fname[k].c_str());
                return fail(rc);
            }
            wb_header(w, k, label[k], k < 4 ? NE : 9, o);
        }
    }
    *out = w;
    return SHUD_OK;
}

extern "C" int shud_wb_on_et_update(shud_wb_t w) {
    if (!w) return shud_fail(SHUD_ERR_ARG, "null argument");
    shud_rhs *h = w->h;
    HIP_TRY(hipSetDevice(h->device));
    // the carried qEleE_IC the next RHS call reads: the packed record's second word, or the SoA ping-pong slot
    const double *src = h->packed ? reinterpret_cast<const double *>(h->dp.cs[h->cur]) + 1 : h->dm.e_ic[h->cur_e];
    hipLaunchKernelGGL(k_wb_ic, dim3((w->NE + 255) / 256), dim3(256), 0, h->stream, w->NE, src, h->packed ? 2 : 1,
                       w->d_ic);
    HIP_TRY(hipGetLastError());
    return SHUD_OK;
}

static int wb_sample_launch(shud_wb *w, double dt, const double *d_dy, bool has_prev) {
    shud_rhs *h = w->h;
    const DevDiag &g = h->dd;
    SampleArgs a{};
    a.n = w->NE; a.dy = d_dy; a.sy = w->d_sy; a.area = w->d_area; a.flags = w->d_flags;
    a.prcp = h->dm.prcp; a.netp = h->dm.net_prep; a.ic = w->d_ic;
    a.es = g.q_es; a.eu = g.q_eu; a.eg = g.q_eg; a.tu = g.q_tu; a.tg = g.q_tg;
    a.stot = g.qele_surf_tot; a.btot = g.qele_sub_tot; a.qs = g.qele_surf; a.qb = g.qele_sub;
    a.eqbc = h->dm.eqbc;
    for (int k = 0; k < 4; k++) { a.acc[k] = w->d_acc[k]; a.prev[k] = w->d_prev[k]; }
    a.dt = dt; a.trapz = w->trapz ? 1 : 0; a.has_prev = has_prev ? 1 : 0;
    a.part = w->d_epart; a.nblk = w->nblk_e;
    hipLaunchKernelGGL(k_wb_sample, dim3(w->nblk_e), dim3(kRedThreads), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    int rc = wb_launch_river(w);
    if (rc) return rc;
    FinArgs f{w->d_epart, w->d_rpart, EQ_N, w->nblk_e, RQ_N, w->nblk_r, 0, w->open ? 1 : 0, w->trapz ? 1 : 0,
              has_prev ? 1 : 0, dt, w->d_s, nullptr};
    hipLaunchKernelGGL(k_wb_finalize, dim3(1), dim3(kFinThreads), 0, h->stream, f);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int shud_wb_sample(shud_wb_t w, double t, const double *d_dy) {
    if (!w || !d_dy) return shud_fail(SHUD_ERR_ARG, "null argument");
    shud_rhs *h = w->h;
    w->sampled = true;
    const double dt = t - w->last_t;
    if (!(dt > 0.0)) {               // :418-423
        w->last_t = t;
        return SHUD_OK;
    }
    if (!h->have_diag || (w->NR > 0 && !h->d_sum[3]))
        return shud_fail(SHUD_ERR_ARG, "shud_wb_sample: call shud_rhs_summary and shud_rhs_refresh_diagnostics first");
    HIP_TRY(hipSetDevice(h->device));
    int rc = wb_sample_launch(w, dt, d_dy, w->has_prev_rate);
    if (rc) return rc;
    w->has_prev_rate = true;
    w->last_t = t;
    return SHUD_OK;
}

extern "C" int shud_wb_maybe_write(shud_wb_t w, double t) {
    if (!w) return shud_fail(SHUD_ERR_ARG, "null argument");
    const long long t_floor = (long long)floor(t);
    if (t_floor < w->interval || (t_floor % w->interval) != 0 || t_floor == w->last_written_floor) return 0;
    shud_rhs *h = w->h;
    HIP_TRY(hipSetDevice(h->device));
    int rc = wb_launch_storage(w, 1);
    if (rc) return rc;
    // the interval is closed on the device from here on (accumulators zeroed, snapshots rolled): a failed copy below
    // must not let a retry at the same t form a second row
    w->last_written_floor = t_floor;
    w->rows++;
    const double tq = (double)(t_floor - (long long)w->interval);
    if (w->fp[0]) {
        for (int k = 0; k < 4; k++) {
            HIP_TRY(hipMemcpyAsync(w->h_row, w->d_res[k], (size_t)w->NE * sizeof(double), hipMemcpyDeviceToHost,
                                   h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
            wb_record(w, k, tq, w->NE, w->h_row);
        }
        HIP_TRY(hipMemcpyAsync(w->h_row, w->d_s + S_ROW, 9 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        wb_record(w, 4, tq, 9, w->h_row);
    }
    if (w->fp[5]) {                  // :597-618, the basin row's t_quantized
        HIP_TRY(hipMemcpyAsync(w->h_row, w->d_qs + Q_ROW, 9 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        wb_record(w, 5, tq, 9, w->h_row);
    }
    if (w->werr) return shud_fail(w->werr, "shud_wb: %s", w->werr_msg.c_str());
    return 1;
}

extern "C" int shud_wb_read(shud_wb_t w, ShudWbOut *o) {
    if (!w || !o) return shud_fail(SHUD_ERR_ARG, "null argument");
    shud_rhs *h = w->h;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t nb = (size_t)w->NE * sizeof(double);
    double *dst[8] = {o->acc3, o->accfull, o->acc3_budget, o->accfull_budget,
                      o->resid3, o->residfull, o->resid3_budget, o->residfull_budget};
    for (int k = 0; k < 8; k++)
        if (dst[k]) HIP_TRY(hipMemcpy(dst[k], k < 4 ? w->d_acc[k] : w->d_res[k - 4], nb, hipMemcpyDeviceToHost));
    double s[S_COUNT];
    HIP_TRY(hipMemcpy(s, w->d_s, sizeof(s), hipMemcpyDeviceToHost));
    for (int k = 0; k < SHUD_WB_NBASIN; k++) { o->basin_acc[k] = s[S_ACC + k]; o->basin_rate[k] = s[S_RATE + k]; }
    for (int k = 0; k < 9; k++) o->basin_row[k] = s[S_ROW + k];
    o->storage[0] = s[S_STOR]; o->storage[1] = s[S_STOR + 1];
    o->last_t = w->last_t;
    o->rows = w->rows;
    o->n_outlets = w->n_outlets;
    return SHUD_OK;
}

// Measurement helper, not part of the supported interface (tools/wb_sample_time.py): `reps` sample passes (element
// pass, reach pass, finalize) with dt = 1 between HIP events on the handle's stream; *ms_sample = milliseconds per
// sample.  It integrates like shud_wb_sample: the accumulators, the sample time and the previous rates move, so
// use it on a diagnostic made for timing.
extern "C" int shud_wb_time_samples(shud_wb_t w, const double *d_dy, int reps, double *ms_sample) {
    if (!w || !d_dy || !ms_sample || reps < 1) return shud_fail(SHUD_ERR_ARG, "bad argument");
    shud_rhs *h = w->h;
    if (!h->have_diag || (w->NR > 0 && !h->d_sum[3]))
        return shud_fail(SHUD_ERR_ARG, "shud_wb_time_samples: summary / diagnostics arrays missing");
    HIP_TRY(hipSetDevice(h->device));
    const int rc = shud::time_passes(h->stream, reps, [&]() -> int {
        const int r = wb_sample_launch(w, 1.0, d_dy, w->has_prev_rate);
        if (!r) w->has_prev_rate = true;
        return r;
    }, ms_sample);
    w->last_t += 1.0 * (reps + 1);
    w->sampled = true;
    return rc;
}

// ---- SHUD_WB_DIAG_QUAD ----
extern "C" int shud_wb_quad_enable(shud_wb_t w) {
    if (!w) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (w->quad) return shud_fail(SHUD_ERR_ARG, "shud_wb_quad_enable: the monitor is already enabled");
    if (w->sampled || w->rows > 0)
        return shud_fail(SHUD_ERR_ARG, "shud_wb_quad_enable: call it before the first shud_wb_sample");
    HIP_TRY(hipSetDevice(w->h->device));
    int rc = w->dalloc(&w->d_qs, (size_t)Q_COUNT);
    if (rc) return rc;
    if (w->have_prefix) {
        w->fname[5] = w->prefix + ".basinwbfull_quad.dat";
        w->fp[5] = fopen(w->fname[5].c_str(), "wb");
        if (!w->fp[5]) return shud_fail(SHUD_WB_ERR_IO, "shud_wb_quad_enable: cannot open %s", w->fname[5].c_str());
        wb_header(w, 5, "basinwbfull_quad (m3)", 9, &w->hdr);
    }
    w->quad = true;
    return SHUD_OK;
}

static int wb_quad_launch(shud_wb *w, double dt, bool has_prev) {
    shud_rhs *h = w->h;
    const DevDiag &g = h->dd;
    QuadArgs a{w->NE, w->d_area, w->d_flags, h->dm.prcp, w->d_ic, g.q_es, g.q_eu, g.q_eg, g.q_tu, g.q_tg,
               g.qele_surf, g.qele_sub, h->dm.eqbc, w->d_epart, w->nblk_e};
    hipLaunchKernelGGL(k_wb_quad, dim3(w->nblk_e), dim3(kRedThreads), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    if (w->NR > 0) {
        QuadRivArgs r{w->NR, w->d_rflags, w->d_rbc, g.qriv_down, h->dm.rqbc, w->d_rpart, w->nblk_r};
        hipLaunchKernelGGL(k_wb_quad_river, dim3(w->nblk_r), dim3(kRedThreads), 0, h->stream, r);
        HIP_TRY(hipGetLastError());
    }
    FinArgs f{w->d_epart, w->d_rpart, EQ_N, w->nblk_e, 2, w->nblk_r, 3, w->open ? 1 : 0, 1, has_prev ? 1 : 0, dt,
              w->d_s, w->d_qs};
    hipLaunchKernelGGL(k_wb_finalize, dim3(1), dim3(kFinThreads), 0, h->stream, f);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the handle holds flux arrays some f() left: an evaluation to replay exists and the refresh has run at least once
// (its ET sums exist).  A refresh older than the last evaluation cannot be told from a current one.
static bool wb_have_fluxes(const shud_rhs *h) { return h->have_diag && h->have_last && h->d_trans != nullptr; }

extern "C" int shud_wb_quad_step(shud_wb_t w, double t) {
    if (!w) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (!w->quad) return shud_fail(SHUD_ERR_ARG, "shud_wb_quad_step: call shud_wb_quad_enable first");
    shud_rhs *h = w->h;
    const double dt = t - w->quad_last_t;
    if (!(dt > 0.0)) {               // :690-694: the previous rates and has_prev stay
        w->quad_last_t = t;
        return SHUD_OK;
    }
    if (!wb_have_fluxes(h))
        return shud_fail(SHUD_ERR_ARG, "shud_wb_quad_step: call shud_rhs_eval and shud_rhs_refresh_diagnostics first");
    HIP_TRY(hipSetDevice(h->device));
    int rc = wb_quad_launch(w, dt, w->quad_has_prev);
    if (rc) return rc;
    w->quad_has_prev = true;
    w->quad_last_t = t;
    return SHUD_OK;
}

extern "C" int shud_wb_read_quad(shud_wb_t w, double acc[7], double rate[7], double row[9], double *last_t) {
    if (!w) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (!w->quad) return shud_fail(SHUD_ERR_ARG, "shud_wb_read_quad: the monitor is not enabled");
    shud_rhs *h = w->h;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    double q[Q_COUNT];
    HIP_TRY(hipMemcpy(q, w->d_qs, sizeof(q), hipMemcpyDeviceToHost));
    for (int k = 0; k < SHUD_WB_NBASIN; k++) {
        if (acc) acc[k] = q[Q_ACC + k];
        if (rate) rate[k] = q[Q_RATE + k];
    }
    if (row)
        for (int k = 0; k < 9; k++) row[k] = q[Q_ROW + k];
    if (last_t) *last_t = w->quad_last_t;
    return SHUD_OK;
}

// Measurement helper (tools/wb_sample_time.py): `reps` monitor passes with dt = 1 between HIP events; the quad
// accumulators, previous rates and quad_last_t move.
extern "C" int shud_wb_time_quad(shud_wb_t w, int reps, double *ms_pass) {
    if (!w || !ms_pass || reps < 1) return shud_fail(SHUD_ERR_ARG, "bad argument");
    if (!w->quad) return shud_fail(SHUD_ERR_ARG, "shud_wb_time_quad: call shud_wb_quad_enable first");
    shud_rhs *h = w->h;
    if (!wb_have_fluxes(h)) return shud_fail(SHUD_ERR_ARG, "shud_wb_time_quad: diagnostics arrays missing");
    HIP_TRY(hipSetDevice(h->device));
    const int rc = shud::time_passes(h->stream, reps, [&]() -> int {
        const int r = wb_quad_launch(w, 1.0, w->quad_has_prev);
        if (!r) w->quad_has_prev = true;
        return r;
    }, ms_pass);
    w->quad_last_t += 1.0 * (reps + 1);
    return rc;
}

extern "C" int shud_wb_destroy(shud_wb_t w) {
    if (!w) return SHUD_OK;
    (void)hipSetDevice(w->h->device);
    (void)hipStreamSynchronize(w->h->stream);
    for (int k = 0; k < 6; k++) {
        if (!w->fp[k]) continue;
        if (fflush(w->fp[k]) != 0 || ferror(w->fp[k])) wb_werr(w, "flush error on " + w->fname[k]);
        if (fclose(w->fp[k]) != 0) wb_werr(w, "close error on " + w->fname[k]);
        w->fp[k] = nullptr;
    }
    const int rc = w->werr ? shud_fail(w->werr, "shud_wb: %s", w->werr_msg.c_str()) : SHUD_OK;
    wb_free(w);
    return rc;
}
