// shud_kat_ode.hip — known-answer harness for the integrator's vector kernels (test infrastructure; not part of
// the C-ABI).  One dispatcher runs one shud::ode launcher (shud_ode_dev.h) of libshud_rhs.so — the shipped code
// object, this unit compiles no kernel — on host-given vectors, then the finalize the controller (shud_ode.cpp)
// issues after it, and returns every vector, the device slots ds[0..S_COUNT) and the host-mapped twin
// hds[0..S_COUNT + 2).  tests/test_gpu_ode_kernels.py compares with tests/ode_kernels_py.py bit for bit.
#include <hip/hip_runtime.h>

#include <cstring>

#include "shud_ode_dev.h"

using namespace shud::ode;

enum KatOdeOp {
    KO_EWT = 0,       // v: zn0, ewt                       d: rtol, atol
    KO_PREDICT,       // v: zn, y?, ycor                   i: q
    KO_PREDICT_PEND,  // v: zn, y?, acor                   i: q, j0, resc, copy_to, ycor_is_acor   c0: l  c1: r
    KO_RESTORE,       // v: zn                             i: q
    KO_RESCALE,       // v: zn                             i: q                                    c0: eta^j
    KO_VSUM,          // v: x, y, z
    KO_VSUM_ZERO,     // v: x, ycor, z
    KO_COPY,          // v: x, z
    KO_SCALE_TO,      // v: x, z? (absent: in place)       d: c
    KO_ZERO,          // v: z
    KO_AXPY_MULTI,    // v: zn                             i: src, jlo, jhi                        c0: coef
    KO_RESIDUAL,      // v: zn1, ycor?, ftemp, ewt, delta  d: rl1, ngamma
    KO_KRYLOV_V0,     // v: delta, ewt, V0                 d: c
    KO_DQ_WORK,       // v: V, ewt, y, work                (ds[S_SIG])
    KO_ATIMES,        // v: w, fy, V, ewt, V0              d: ngamma                               (ds[S_SIG])
    KO_MGS,           // v: w, Vprev?, Vnext?              i: hslot, slot0                         (ds[hslot])
    KO_NORMALIZE,     // v: w, ewt                         d: c
    KO_NEWTON,        // v: V?, dsrc?, ewt, ycor           i: krydim, ycor_zero                    c0: yg
    KO_COMPLETE,      // v: zn, acor                       i: jlo, q, copy_to                      c0: l
    KO_COMPLETE_EWT,  // v: zn, acor, ewt_next             i: q, copy_to, jst   d: rtol, atol      c0: l
    KO_ETA_NORMS,     // v: znq?, znqmax?, acor?, ewt      i: pend_q            d: ncquot, lq
    KO_DKY,           // v: zn, out, acor?                 i: nvec, pd.j0, pd.q, js[0..nvec)  d: rscale  c0: c  c1: pd.l
    KO_COUNT
};
enum { KO_MAXV = 5, KO_NI = 12, KO_ND = 4 };

namespace {
struct Bufs {                             // everything one call owns; freed on every path
    double *d[KO_MAXV] = {};
    double *part = nullptr, *ds = nullptr, *hds = nullptr;
    uint32_t *err = nullptr;
    hipStream_t s = nullptr;
    ~Bufs() {
        for (double *p : d)
            if (p) (void)hipFree(p);
        if (part) (void)hipFree(part);
        if (ds) (void)hipFree(ds);
        if (err) (void)hipFree(err);
        if (hds) (void)hipHostFree(hds);
        if (s) (void)hipStreamDestroy(s);
    }
};
Coefs coefs(const double *c) {
    Coefs o{};
    if (c) memcpy(o.c, c, sizeof(o.c));
    return o;
}
}  // namespace

extern "C" int shud_kat_ode_slots(int *s_count, int *max_l, int *q_max) {
    *s_count = S_COUNT;
    *max_l = kMaxL;
    *q_max = kQMax;
    return KO_COUNT;
}
extern "C" int shud_kat_ode_grid_blocks(int64_t n) { return n >= 1 ? grid_blocks(n) : -1; }

// vec[k]: host array of cols[k] * n doubles (cols[k] == 0: absent, the launcher gets a null pointer), copied to
// the device before and back after.  ip[KO_NI], dp[KO_ND]; c0, c1: kMaxL + 1 doubles or null (zeros).
// ds[S_COUNT] and hds[S_COUNT + 2] are in-out (pre-fill them to see which slots a finalize wrote).  use_err:
// finalize reads a device word holding err_word; otherwise Red::err is null.
// returns 0, -1 on bad arguments (nothing launched), -3 on a HIP error.
extern "C" int shud_kat_ode_run(int op, int64_t n, const int *ip, const double *dp, const double *c0,
                                const double *c1, double *const *vec, const int *cols, double *ds, double *hds,
                                uint64_t seq, int use_err, uint32_t err_word) {
    if (op < 0 || op >= KO_COUNT || n < 1 || !ip || !dp || !vec || !cols || !ds || !hds) return -1;
    for (int k = 0; k < KO_MAXV; ++k)
        if (cols[k] < 0 || cols[k] > kMaxL + 1 || (cols[k] > 0 && !vec[k])) return -1;
    // ---- per-op validation: required vectors, column counts covering every index the kernel touches ----
    auto need = [&](int k, int c) { return cols[k] >= c; };
    auto only1 = [&](int k) { return cols[k] == 0 || cols[k] == 1; };
    auto qok = [&](int q) { return q >= 1 && q <= kQMax; };
    bool ok = false;
    int slot0 = 0, nacc = 0;
    unsigned minmask = 0u;
    switch (op) {
    case KO_EWT: ok = need(0, 1) && need(1, 1); slot0 = S_EWTMIN; nacc = 2; minmask = 1u; break;
    case KO_PREDICT: ok = qok(ip[0]) && need(0, ip[0] + 1) && only1(1) && need(2, 1); break;
    case KO_PREDICT_PEND:
        ok = qok(ip[0]) && need(0, ip[0] + 1) && only1(1) && need(2, 1) && (ip[1] == 0 || ip[1] == 1) &&
             (ip[2] == 0 || ip[2] == 1) && ip[3] >= -1 && ip[3] < cols[0];
        break;
    case KO_RESTORE: ok = qok(ip[0]) && need(0, ip[0] + 1); break;
    case KO_RESCALE: ok = qok(ip[0]) && need(0, ip[0] + 1); break;
    case KO_VSUM: ok = need(0, 1) && need(1, 1) && need(2, 1); break;
    case KO_VSUM_ZERO: ok = need(0, 1) && need(1, 1) && need(2, 1); break;
    case KO_COPY: ok = need(0, 1) && need(1, 1); break;
    case KO_SCALE_TO: ok = need(0, 1) && only1(1); break;
    case KO_ZERO: ok = need(0, 1); break;
    case KO_AXPY_MULTI:
        ok = ip[0] >= 0 && ip[0] < cols[0] && ip[1] >= 1 && ip[2] <= kQMax + 1 && ip[2] < cols[0] &&
             (ip[0] < ip[1] || ip[0] > ip[2]);
        break;
    case KO_RESIDUAL:
        ok = need(0, 1) && only1(1) && need(2, 1) && need(3, 1) && need(4, 1); slot0 = S_RES; nacc = 1; break;
    case KO_KRYLOV_V0: ok = need(0, 1) && need(1, 1) && need(2, 1); slot0 = S_SIG; nacc = 1; break;
    case KO_DQ_WORK: ok = need(0, 1) && need(1, 1) && need(2, 1) && need(3, 1); break;
    case KO_ATIMES:
        ok = need(0, 1) && need(1, 1) && need(2, 1) && need(3, 1) && need(4, 1); slot0 = S_W; nacc = 2; break;
    case KO_MGS:
        ok = need(0, 1) && only1(1) && only1(2) && ip[0] >= 0 && ip[0] < S_COUNT && ip[1] >= 0 && ip[1] < S_COUNT;
        slot0 = ip[1]; nacc = 1;
        break;
    case KO_NORMALIZE: ok = need(0, 1) && need(1, 1); slot0 = S_SIG; nacc = 1; break;
    case KO_NEWTON:
        ok = ip[0] >= 0 && ip[0] <= kMaxL && need(0, ip[0]) && only1(1) && need(2, 1) && need(3, 1) &&
             (ip[1] == 0 || ip[1] == 1);
        slot0 = S_DEL; nacc = 2;
        break;
    case KO_COMPLETE:
        ok = ip[0] >= 0 && ip[1] >= 0 && ip[1] <= kQMax && need(0, ip[1] + 1) && need(1, 1) && ip[2] >= -1 &&
             ip[2] < cols[0];
        break;
    case KO_COMPLETE_EWT:
        ok = ip[0] >= 0 && ip[0] <= kQMax && need(0, ip[0] + 1) && need(1, 1) && need(2, 1) && ip[1] >= -1 &&
             ip[1] < cols[0] && (ip[2] == 0 || ip[2] == 1);
        slot0 = S_EWTMIN; nacc = 2; minmask = 1u;
        break;
    case KO_ETA_NORMS:
        ok = only1(0) && only1(1) && only1(2) && need(3, 1) && (ip[0] == 0 || ip[0] == 1) &&
             (need(2, 1) || !(cols[1] || ip[0]));
        slot0 = S_ETAQM1; nacc = 2;
        break;
    case KO_DKY:
        ok = ip[0] >= 1 && ip[0] <= kQMax + 1 && need(0, 1) && need(1, 1) && only1(2);
        for (int k = 0; ok && k < ip[0]; ++k) ok = ip[3 + k] >= 0 && ip[3 + k] < cols[0];
        break;
    }
    if (!ok) return -1;

    Bufs b;
    const size_t vb = sizeof(double) * (size_t)n;
#define KO_TRY(x) do { if ((x) != hipSuccess) return -3; } while (0)
    KO_TRY(hipStreamCreate(&b.s));
    for (int k = 0; k < KO_MAXV; ++k)
        if (cols[k] > 0) {
            KO_TRY(hipMalloc(&b.d[k], vb * cols[k]));
            KO_TRY(hipMemcpy(b.d[k], vec[k], vb * cols[k], hipMemcpyHostToDevice));
        }
    // the Red of shud_ode.cpp's ode_alloc
    Red r{};
    r.nblk = grid_blocks(n);
    KO_TRY(hipMalloc(&b.part, (size_t)kMaxAcc * r.nblk * sizeof(double)));
    KO_TRY(hipMalloc(&b.ds, S_COUNT * sizeof(double)));
    KO_TRY(hipMemcpy(b.ds, ds, S_COUNT * sizeof(double), hipMemcpyHostToDevice));
    KO_TRY(hipHostMalloc(&b.hds, (S_COUNT + 2) * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
    memcpy(b.hds, hds, (S_COUNT + 2) * sizeof(double));
    r.part = b.part;
    r.ds = b.ds;
    KO_TRY(hipHostGetDevicePointer((void **)&r.hds, b.hds, 0));
    if (use_err) {
        KO_TRY(hipMalloc(&b.err, sizeof(uint32_t)));
        KO_TRY(hipMemcpy(b.err, &err_word, sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    r.err = b.err;
    r.slot0 = slot0;
    r.seq = seq;

    double *const *d = b.d;
    hipStream_t s = b.s;
    const Coefs k0 = coefs(c0), k1 = coefs(c1);
    switch (op) {
    case KO_EWT: ewt_set(n, d[0], d[1], dp[0], dp[1], r, s); break;
    case KO_PREDICT: predict(n, d[0], ip[0], d[1], d[2], s); break;
    case KO_PREDICT_PEND: {
        Pend pd{};
        pd.acor = d[2];
        pd.l = k0;
        pd.r = k1;
        pd.q = ip[0];
        pd.j0 = ip[1];
        pd.resc = ip[2];
        pd.copy_to = ip[3];
        predict_pend(n, d[0], ip[0], d[1], ip[4] ? d[2] : nullptr, pd, s);
        break;
    }
    case KO_RESTORE: restore(n, d[0], ip[0], s); break;
    case KO_RESCALE: rescale(n, d[0], ip[0], k0, s); break;
    case KO_VSUM: vsum(n, d[0], d[1], d[2], s); break;
    case KO_VSUM_ZERO: vsum_zero(n, d[0], d[1], d[2], s); break;
    case KO_COPY: copy(n, d[0], d[1], s); break;
    case KO_SCALE_TO: scale_to(n, dp[0], d[0], d[1] ? d[1] : d[0], s); break;
    case KO_ZERO: zero(n, d[0], s); break;
    case KO_AXPY_MULTI: axpy_multi(n, d[0], ip[0], k0, ip[1], ip[2], s); break;
    case KO_RESIDUAL: residual(n, d[0], d[1], d[2], dp[0], dp[1], d[3], d[4], r, s); break;
    case KO_KRYLOV_V0: krylov_v0(n, d[0], d[1], dp[0], d[2], r, s); break;
    case KO_DQ_WORK: dq_work(n, d[0], d[1], d[2], d[3], b.ds, s); break;
    case KO_ATIMES: atimes(n, d[0], d[1], d[2], d[3], d[4], dp[0], b.ds, r, s); break;
    case KO_MGS: mgs(n, d[0], d[1], b.ds, ip[0], d[2], r, s); break;
    case KO_NORMALIZE: normalize(n, d[0], dp[0], d[1], r, s); break;
    case KO_NEWTON: newton_update(n, d[0], n, ip[0], k0, d[1], d[2], d[3], ip[1] != 0, r, s); break;
    case KO_COMPLETE: complete_step(n, d[0], d[1], k0, ip[0], ip[1], ip[2], s); break;
    case KO_COMPLETE_EWT: complete_step_ewt(n, d[0], d[1], k0, ip[0], ip[1], ip[2], dp[0], dp[1], d[2], r, s); break;
    case KO_ETA_NORMS: eta_norms(n, d[0], d[1], d[2], dp[0], d[3], ip[0], dp[1], r, s); break;
    case KO_DKY: {
        Pend pd{};
        pd.acor = d[2];
        pd.l = k1;
        pd.j0 = ip[1];
        pd.q = ip[2];
        pd.copy_to = -1;
        dky(n, d[0], n, ip + 3, k0, ip[0], dp[0], d[1], pd, s);
        break;
    }
    }
    KO_TRY(hipGetLastError());
    if (nacc > 0) {
        finalize(r, nacc, minmask, s);
        KO_TRY(hipGetLastError());
    }
    KO_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < KO_MAXV; ++k)
        if (cols[k] > 0) KO_TRY(hipMemcpy(vec[k], b.d[k], vb * cols[k], hipMemcpyDeviceToHost));
    KO_TRY(hipMemcpy(ds, b.ds, S_COUNT * sizeof(double), hipMemcpyDeviceToHost));
    memcpy(hds, b.hds, (S_COUNT + 2) * sizeof(double));
#undef KO_TRY
    return 0;
}
