// shud_rhs.cpp — host runtime behind include/shud_rhs.h (C-ABI).
//
// Replaces the reference RHS callback f() (src/Model/f.cpp:2-32) and the Model_Data arrays it works
// on (src/ModelData/Model_Data.hpp:111-208).  The handle owns device SoA copies of the static mesh and
// parameters (uploaded once, shud_rhs_create), of the per-ET-step inputs (shud_rhs_set_step_inputs),
// and of the carried RHS state (qEleE_IC, u_satn — ping-pong buffers so a diagnostic replay sees the
// exact inputs of the last call).  y / ydot are borrowed per call.
//
// Multi-GPU: one process per GPU, each handle holds its partition (owned + ghost
// entities); ghost states arrive by one grouped RCCL send/recv exchange (= ncclAllToAllv restricted
// to the peers that share a boundary) per eval, before the element kernel.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "shud_handle.h"
#include "shud_order.h"
#include "shud_tables.h"

using namespace shud;

namespace {
thread_local std::string g_last_error;
}  // namespace

// Event scopes.  Every event here orders work between queues of one device (the comm stream's pack / exchange and
// the main stream's kernels) or times kernels: a device-scope release is enough for both, and the default
// system-scope release writes the L2's dirty lines back to HBM at every record (profiles/r03/ev_scope/).  RCCL's
// own kernels on s_comm complete before ev_comm, which then publishes their writes to this device's other queues.
static constexpr unsigned kEvSync = hipEventDisableSystemFence;
static constexpr unsigned kEvTime = hipEventReleaseToDevice;

int shud_fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

int shud_reset_err(shud_rhs *h) {
    DevErr z{};
    z.flags = 0;
    for (int k = 0; k < 8; k++) z.first_index[k] = INT_MAX;
    z.n_warn = 0;
    z.warn = h->d_warn;
    z.map = h->ordered ? h->d_perm : nullptr;
    HIP_TRY(hipMemsetAsync(h->d_warn, 0, kWarnSlots * kWarnStride * sizeof(unsigned long long), h->stream));
    HIP_TRY(hipMemcpyAsync(h->d_err, &z, sizeof(DevErr), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int shud_rhs_abi_version(void) { return SHUD_RHS_ABI_VERSION; }
extern "C" const char *shud_rhs_last_error_string(void) { return g_last_error.c_str(); }

// ---------------------------------------------------------------------------------------------
// create
// ---------------------------------------------------------------------------------------------
// Build the host tables (shud_tables.cpp), copy their scalars into the handle, upload, allocate the work buffers.
// The tables go when this returns; seg_perm alone stays in the handle (diagnostics in reference segment order).
static int build(shud_rhs *h, const ShudMeshSoA *m, const ShudParamsSoA *p, const ShudRhsOptions *opt,
                 const ShudPartition *part) {
    HostTables H;
    int rc = build_tables(m, p, opt, part, &H);
    if (rc) return rc;
    MeshTables &T = H.mesh;
    const PackedTables &K = H.pk;
    const int NE = m->num_ele, NR = m->num_riv, NS = m->num_seg;
    h->NE = NE; h->NR = NR; h->NS = NS;
    h->mode = T.mode; h->open = T.open;
    h->check_errors = opt ? opt->check_errors != 0 : true; h->device = opt ? opt->device : 0;
    h->n_own = T.n_own; h->n_segghost = T.n_segghost; h->n_own_riv = T.n_own_riv; h->n_int = T.n_int;
    h->lakeon = T.lakeon; h->NL = T.NL;
    std::copy(T.max_col, T.max_col + 4, h->max_col);
    h->seg_perm.swap(T.seg_perm);
    h->packed = H.packed; h->dp = K.dp; h->n_classes = K.dp.ncls; h->n_shared = K.n_shared;

    // ---- device ----
    HIP_TRY(hipSetDevice(h->device));
    if (opt && opt->stream) {
        h->stream = (hipStream_t)opt->stream;
    } else {
        HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        h->own_stream = true;
    }
    // the first failure sticks: later uploads are skipped and rc is returned after the last one
    auto up = [&](auto **dst, const auto *src, size_t n) { if (!rc) rc = h->upload(dst, src, n); };
    auto upv = [&](auto **dst, const auto &v) { up(dst, v.data(), v.size()); };
    auto zero = [&](auto **dst, size_t n) { if (!rc) rc = h->zeros(dst, n); };
    auto fill = [&](auto **dst, const double *src, size_t n, double v) { if (!rc) rc = h->upload_fill(dst, src, n, v); };
    const size_t E = (size_t)NE, E3 = 3 * E;
    DevMesh &d = h->dm;
    d.num_ele = NE;
    up(&d.nabr, m->nabr, E3); upv(&d.eflags, T.eflags);
    up(&d.area, m->area, E); up(&d.z_surf, m->z_surf, E); up(&d.z_bottom, m->z_bottom, E);
    fill(&d.depression, m->depression, E, 0.0002);
    up(&d.edge, m->edge, E3); up(&d.dist2nabor, m->dist2nabor, E3); up(&d.avg_rough, m->avg_rough, E3);
    if (h->open) { up(&d.dist2edge, m->dist2edge, E3); up(&d.rough, m->rough, E); }
    else { zero(&d.dist2edge, 1); zero(&d.rough, 1); }
    up(&d.aq, p->aquifer_depth, E); up(&d.macD, p->macD, E); up(&d.macKsatH, p->macKsatH, E);
    up(&d.vAreaF, p->geo_vAreaF, E); up(&d.KsatH, p->KsatH, E); up(&d.KsatV, p->KsatV, E);
    up(&d.infKsatV, p->infKsatV, E); up(&d.hAreaF, p->hAreaF, E); up(&d.macKsatV, p->macKsatV, E);
    up(&d.ThetaS, p->ThetaS, E); up(&d.ThetaR, p->ThetaR, E); up(&d.Beta, p->Beta, E); up(&d.infD, p->infD, E);
    up(&d.Sy, p->Sy, E); up(&d.RzD, p->RzD, E); up(&d.VegFrac, p->VegFrac, E); up(&d.ImpAF, p->ImpAF, E);
    zero(&d.prcp, E); zero(&d.net_prep, E); zero(&d.pot_evap, E); zero(&d.pot_tran, E); zero(&d.etp, E);
    zero(&d.lai, E); zero(&d.ugw_stale, E);
    fill(&d.fu_surf, nullptr, E, 1.0); fill(&d.fu_sub, nullptr, E, 1.0);
    for (int k = 0; k < 2; k++) { zero(&d.e_ic[k], E); zero(&d.u_satn[k], E); }
    for (int k = 0; k < 4; k++) {
        h->tab_len[k] = h->max_col[k] + 1;
        zero(&h->d_tab[k], h->tab_len[k]);
    }
    d.eybc = h->d_tab[0]; d.eqbc = h->d_tab[1]; d.rybc = h->d_tab[2]; d.rqbc = h->d_tab[3];
    upv(&d.seg_off, T.seg_off); upv(&d.seg_riv, T.seg_riv); upv(&d.seg_len, T.seg_len); upv(&d.seg_cwr, T.seg_cwr);
    zero(&d.qseg_surf, NS); zero(&d.qseg_sub, NS);
    upv(&d.riv_down, T.riv_down); upv(&d.riv_bc, T.riv_bc);
    up(&d.riv_len, m->riv_length, NR); up(&d.riv_slope, m->riv_bed_slope, NR); up(&d.riv_d2down, m->riv_dist2down, NR);
    up(&d.riv_avg_rough, m->riv_avg_rough, NR); up(&d.riv_depth, m->riv_depth, NR); up(&d.riv_bw, m->riv_bottom_width, NR);
    up(&d.riv_bankslope, m->riv_bankslope, NR); up(&d.riv_ksath, m->riv_ksath, NR); up(&d.riv_bedthick, m->riv_bedthick, NR);
    upv(&d.up_off, T.up_off); upv(&d.up_idx, T.up_idx);
    up(&d.rseg_off, T.reach_off.data(), (size_t)T.n_own_riv + 1); upv(&d.rseg_pos, T.rseg_pos);
    if (h->packed) {
        DevPacked &P = h->dp;
        upv(&P.ctab, K.ctab); upv(&P.zz, K.zz); upv(&P.meta, K.meta); upv(&P.ged, K.ged); up(&P.area, m->area, E);
        upv(&P.seg_first, K.seg_first);
        if (P.nh) upv(&P.hv, K.hv);
        upv(&P.sg_lc, K.sg_lc); upv(&P.sg_r, T.seg_riv); upv(&P.rrec, K.rrec);
        zero(&P.qseg2, NS); zero(&P.s_np, E); zero(&P.s_tl, E); zero(&P.cs[0], E); zero(&P.cs[1], E);
        if (!rc) rc = h->upload_fill(&P.s_fu, (const double2 *)nullptr, E, make_double2(1.0, 1.0));
        upv(&P.rv, K.rv); upv(&P.rv_u, K.rv_u);
        if (P.nqd) zero(&P.qdown, NR);
    }
    if (h->lakeon) {
        DevLake &L = h->lk;
        const LakeTables &S = H.lake;
        L.nl = h->NL;
        L.y_off = 3 * h->n_own + h->n_own_riv;    // [sf|us|gw|riv|lake] over owned entities
        upv(&L.lake_of, S.lake_of); upv(&L.ele_off, S.ele_off); upv(&L.ele_idx, S.ele_idx);
        upv(&L.bank_off, S.bank_off); upv(&L.bank_pos, S.bank_pos); upv(&L.rin_off, S.rin_off); upv(&L.rin_idx, S.rin_idx);
        const size_t nb = m->lake_bathy_off[h->NL];
        up(&L.bathy_off, m->lake_bathy_off, (size_t)h->NL + 1); up(&L.bathy_y, m->lake_bathy_y, nb); up(&L.bathy_a, m->lake_bathy_a, nb);
        zero(&L.bank_qs, E3); zero(&L.bank_qg, E3);
    }
    if (rc) return rc;

    // ---- work buffers ----
    if ((rc = h->dalloc(&h->d_err, 1)) || (rc = h->dalloc(&h->d_warn, (size_t)kWarnSlots * kWarnStride))) return rc;
    d.err = h->d_err;
    HIP_TRY(hipHostMalloc((void **)&h->h_err, sizeof(DevErr), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void **)&h->h_warn, kWarnSlots * kWarnStride * sizeof(unsigned long long),
                          hipHostMallocDefault));
    if ((rc = shud_reset_err(h))) return rc;
    const size_t ny = 3 * (size_t)h->n_own + h->n_own_riv + h->NL;
    if ((rc = h->dalloc(&h->d_y, ny)) || (rc = h->dalloc(&h->d_ydot, ny))) return rc;
    return h->dalloc(&h->d_scratch_dy, ny);
}

static int setup_partition(shud_rhs *h, const ShudPartition *part) {
    h->partitioned = true;
    h->rank = part->rank;
    h->nranks = part->nranks;
    const int P = part->nranks;
    if (P < 1 || part->rank < 0 || part->rank >= P) return shud_fail(SHUD_ERR_ARG, "bad rank/nranks");
    h->esend_off.assign(part->ele_send_off, part->ele_send_off + P + 1);
    h->erecv_off.assign(part->ele_recv_off, part->ele_recv_off + P + 1);
    h->rsend_off.assign(part->riv_send_off, part->riv_send_off + P + 1);
    h->rrecv_off.assign(part->riv_recv_off, part->riv_recv_off + P + 1);
    h->n_esend = h->esend_off[P];
    h->n_rsend = h->rsend_off[P];
    h->n_eghost = h->erecv_off[P];
    h->n_rghost = h->rrecv_off[P];
    if (h->n_own + h->n_eghost != h->NE) return shud_fail(SHUD_ERR_ARG, "ghost element count mismatch");
    if (h->n_own_riv + h->n_rghost != h->NR) return shud_fail(SHUD_ERR_ARG, "ghost reach count mismatch");
    for (int k = 0; k < h->n_esend; k++)
        if (part->ele_send_idx[k] < 0 || part->ele_send_idx[k] >= h->n_own) return shud_fail(SHUD_ERR_ARG, "bad ele_send_idx");
    for (int k = 0; k < h->n_rsend; k++)
        if (part->riv_send_idx[k] < 0 || part->riv_send_idx[k] >= h->n_own_riv) return shud_fail(SHUD_ERR_ARG, "bad riv_send_idx");
    int rc;
    if ((rc = h->upload(&h->d_esend_idx, part->ele_send_idx, h->n_esend))) return rc;
    if ((rc = h->upload(&h->d_rsend_idx, part->riv_send_idx, h->n_rsend))) return rc;
    if ((rc = h->dalloc(&h->d_esend, 3 * (size_t)h->n_esend))) return rc;
    if ((rc = h->dalloc(&h->d_rsend, (size_t)h->n_rsend))) return rc;
    if ((rc = h->dalloc(&h->d_gele, 3 * (size_t)h->n_eghost))) return rc;
    if ((rc = h->dalloc(&h->d_griv, (size_t)h->n_rghost))) return rc;
    if (part->nccl_unique_id) {
        ncclUniqueId id;
        memcpy(&id, part->nccl_unique_id, sizeof(id));
        h->use_nccl = true;
        NCCL_TRY(ncclCommInitRank(&h->comm, P, id, part->rank));
    }
    // the pack kernel and the exchange run on a side stream beside the interior element kernel (RCCL and
    // external transport alike, so the one-GPU rank timings measure the same pipeline)
    HIP_TRY(hipStreamCreateWithFlags(&h->s_comm, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_pack, hipEventDisableTiming | kEvSync));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_comm, hipEventDisableTiming | kEvSync));
    if ((rc = h->upload(&h->d_halo_flag, (const unsigned long long *)nullptr, 1))) return rc;
    h->fold = env_knob("SHUD_RHS_FOLD", 1, 0, 1) != 0;
    // the trailing join of the comm stream after a folded eval costs ~4 us per eval at 8 ranks (one more packet for
    // the command processor between evals; profiles/r04/rankjoin): off by default.  Without it, after a poll timeout
    // (SHUD_EF_HALO_WAIT, fatal) the late pack / exchange may still run beside later main-stream work — results that
    // the fatal flag already invalidates; the error read (shud_read_err) drains the comm stream before reporting
    h->fold_join = env_knob("SHUD_RHS_FOLD_JOIN", 0, 0, 1) != 0;
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) == hipSuccess && khz > 0)
        h->wall_khz = khz;
    const double ms = env_knob("SHUD_HALO_TIMEOUT_MS", 5000, 1, 3600000);
    h->halo_timeout = (unsigned long long)(ms * h->wall_khz);
    return 0;
}

static void destroy_handle(shud_rhs *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->s_comm) (void)hipStreamSynchronize(h->s_comm);
    if (h->comm) ncclCommDestroy(h->comm);
    shud_et_free(h);
    if (h->ev_pack) (void)hipEventDestroy(h->ev_pack);
    if (h->ev_comm) (void)hipEventDestroy(h->ev_comm);
    for (auto e : h->tm_ev) (void)hipEventDestroy(e);
    if (h->s_comm) (void)hipStreamDestroy(h->s_comm);
    for (void *p : h->allocs) (void)hipFree(p);
    if (h->h_err) (void)hipHostFree(h->h_err);
    if (h->h_warn) (void)hipHostFree(h->h_warn);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

extern "C" int shud_rhs_create(const ShudMeshSoA *mesh, const ShudParamsSoA *par, const ShudRhsOptions *opt,
                               shud_rhs_t *out) {
    if (!mesh || !par || !out) return shud_fail(SHUD_ERR_ARG, "null argument");
    shud_rhs *h = new shud_rhs();
    int rc = build(h, mesh, par, opt, nullptr);
    if (rc) { destroy_handle(h); return rc; }
    *out = h;
    return SHUD_OK;
}

// ---------------------------------------------------------------------------------------------
// ordered handles (include/shud_order.h)
// ---------------------------------------------------------------------------------------------
extern "C" int shud_rhs_create_ordered(const ShudMeshSoA *mesh, const ShudParamsSoA *par, const ShudRhsOptions *opt,
                                       int kind, const int32_t *user_perm, shud_rhs_t *out) {
    if (!mesh || !par || !out) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (kind == SHUD_ORDER_IDENTITY) return shud_rhs_create(mesh, par, opt, out);
    const int NE = mesh->num_ele;
    if (NE < 0) return shud_fail(SHUD_ERR_ARG, "negative num_ele");
    std::vector<int> perm((size_t)NE);
    int rc = shud_order_plan(mesh, kind, user_perm, perm.data());
    if (rc) return rc;
    shud_ordered_t store = nullptr;
    ShudMeshSoA pm;
    ShudParamsSoA pp;
    if ((rc = shud_order_apply(mesh, par, perm.data(), &store, &pm, &pp))) return rc;    // refuses lake models
    shud_rhs *h = new shud_rhs();
    rc = build(h, &pm, &pp, opt, nullptr);
    shud_order_free(store);
    if (!rc) {
        h->order_kind = kind;
        h->inv.resize((size_t)NE);
        for (int k = 0; k < NE; k++) h->inv[perm[k]] = k;
        h->perm.swap(perm);
        bool ident = true;               // an identity plan: nothing to carry, the handle behaves as a plain one
        for (int k = 0; k < NE && ident; k++) ident = h->perm[k] == k;
        h->ordered = !ident;
    }
    if (!rc && h->ordered) {
        if (!(rc = h->dalloc(&h->d_perm, (size_t)NE)) && !(rc = h->dalloc(&h->d_inv, (size_t)NE)) &&
            !(rc = h->dalloc(&h->d_stage, 3 * (size_t)NE + h->NR + h->NL))) {
            hipError_t e = hipMemcpy(h->d_perm, h->perm.data(), (size_t)NE * sizeof(int), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(h->d_inv, h->inv.data(), (size_t)NE * sizeof(int), hipMemcpyHostToDevice);
            if (e != hipSuccess) rc = shud_fail(SHUD_ERR_HIP, "order upload failed: %s", hipGetErrorString(e));
        }
        if (!rc) rc = shud_reset_err(h);             // the error word now carries the index map (DevErr::map)
    }
    if (rc) { destroy_handle(h); return rc; }
    *out = h;
    return SHUD_OK;
}

extern "C" int shud_rhs_order(shud_rhs_t h, int *kind, int32_t *perm_host, int32_t *inv_host) {
    if (!h) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (kind) *kind = h->order_kind;
    const bool have = !h->perm.empty();
    for (int k = 0; k < h->NE; k++) {
        if (perm_host) perm_host[k] = have ? h->perm[k] : k;
        if (inv_host) inv_host[k] = have ? h->inv[k] : k;
    }
    return SHUD_OK;
}

extern "C" int shud_rhs_permute(shud_rhs_t h, int dir, int what, const double *d_src, double *d_dst) {
    if (!h || !d_src || !d_dst || d_src == d_dst) return shud_fail(SHUD_ERR_ARG, "shud_rhs_permute: bad pointers");
    if ((dir != SHUD_PERM_TO_INTERNAL && dir != SHUD_PERM_TO_CALLER) || what < SHUD_PERM_STATE || what > SHUD_PERM_ELE3)
        return shud_fail(SHUD_ERR_ARG, "shud_rhs_permute: bad dir / what");
    HIP_TRY(hipSetDevice(h->device));
    const int planes = what == SHUD_PERM_ELE ? 1 : 3;
    const int ne = what == SHUD_PERM_STATE ? h->n_own : h->NE;
    const int ntail = what == SHUD_PERM_STATE ? h->n_own_riv + h->NL : 0;
    if (!h->ordered) {
        const size_t n = (size_t)planes * ne + ntail;
        if (n) HIP_TRY(hipMemcpyAsync(d_dst, d_src, n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        return SHUD_OK;
    }
    launch_perm_kernel(dir == SHUD_PERM_TO_INTERNAL ? h->d_perm : h->d_inv, ne, planes, d_src, d_dst, ntail, h->stream);
    HIP_TRY(hipGetLastError());
    return SHUD_OK;
}

extern "C" int shud_rhs_nccl_unique_id(char out[128]) {
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    memcpy(out, &id, sizeof(id));
    return SHUD_OK;
}

extern "C" int shud_rhs_create_partitioned(const ShudMeshSoA *mesh, const ShudParamsSoA *par,
                                           const ShudRhsOptions *opt, const ShudPartition *part,
                                           shud_rhs_t *out) {
    if (!mesh || !par || !part || !out) return shud_fail(SHUD_ERR_ARG, "null argument");
    shud_rhs *h = new shud_rhs();
    int rc = build(h, mesh, par, opt, part);
    if (!rc) rc = setup_partition(h, part);
    if (rc) { destroy_handle(h); return rc; }
    *out = h;
    return SHUD_OK;
}

extern "C" int shud_rhs_destroy(shud_rhs_t h) {
    destroy_handle(h);
    return SHUD_OK;
}

// ---------------------------------------------------------------------------------------------
// step inputs
// ---------------------------------------------------------------------------------------------
extern "C" int shud_rhs_set_step_inputs(shud_rhs_t h, const ShudStepInputs *in) {
    if (!h || !in) return shud_fail(SHUD_ERR_ARG, "null argument");
    // ordered handle: the caller's [NE] arrays gathered into the internal numbering on the host, then as below
    ShudStepInputs g;
    std::vector<std::vector<double>> gbuf;
    if (h->ordered) {
        g = *in;
        const double **f[] = {&g.net_prep, &g.pot_evap, &g.pot_tran, &g.etp, &g.lai, &g.fu_surf, &g.fu_sub,
                              &g.e_ic, &g.u_satn, &g.ugw_stale, &g.prcp};
        for (auto pp : f) {
            if (!*pp) continue;
            gbuf.emplace_back((size_t)h->NE);
            int rc = shud_order_gather_host(h->perm.data(), h->NE, sizeof(double), 1, *pp, gbuf.back().data());
            if (rc) return rc;
            *pp = gbuf.back().data();
        }
        in = &g;
    }
    HIP_TRY(hipSetDevice(h->device));
    const size_t nb = (size_t)h->NE * sizeof(double);
    // packed layout: carried-state overrides go through SoA staging slot 0, then into the packed record
    const double *eic_dst = h->packed ? h->dm.e_ic[0] : h->dm.e_ic[h->cur_e];
    const double *satn_dst = h->packed ? h->dm.u_satn[0] : h->dm.u_satn[h->cur];
    struct { const double *src; const double *dst; } arr[] = {
        {in->net_prep, h->dm.net_prep}, {in->pot_evap, h->dm.pot_evap}, {in->pot_tran, h->dm.pot_tran},
        {in->etp, h->dm.etp}, {in->lai, h->dm.lai}, {in->fu_surf, h->dm.fu_surf}, {in->fu_sub, h->dm.fu_sub},
        {in->ugw_stale, h->dm.ugw_stale}, {in->e_ic, eic_dst}, {in->u_satn, satn_dst}, {in->prcp, h->dm.prcp}};
    for (auto &a : arr)
        if (a.src) HIP_TRY(hipMemcpyAsync((void *)a.dst, a.src, nb, hipMemcpyHostToDevice, h->stream));
    if (h->packed) {
        auto all_ones = [&](const double *v) {
            for (int i = 0; i < h->NE; i++)
                if (!(v[i] == 1.0)) return false;
            return true;
        };
        if (in->fu_surf) h->fu_unit[0] = all_ones(in->fu_surf);
        if (in->fu_sub) h->fu_unit[1] = all_ones(in->fu_sub);
        unsigned what = 0;
        if (in->net_prep || in->pot_evap) what |= 1;
        if (in->pot_tran || in->lai || in->etp) what |= 2;
        if (in->fu_surf || in->fu_sub) what |= 4;
        if (in->u_satn) what |= 8;
        if (in->e_ic) what |= 16;
        launch_pack_step_kernel(h->dm, h->dp, h->NE, h->cur, what, h->stream);
        HIP_TRY(hipGetLastError());
    }
    const double *tabs[4] = {in->ele_ybc, in->ele_qbc, in->riv_ybc, in->riv_qbc};
    const int ns[4] = {in->n_ele_ybc, in->n_ele_qbc, in->n_riv_ybc, in->n_riv_qbc};
    for (int k = 0; k < 4; k++) {
        if (!tabs[k]) continue;
        if (ns[k] < h->max_col[k])
            return shud_fail(SHUD_ERR_ARG, "BC table %d has %d columns, mesh references column %d", k, ns[k], h->max_col[k]);
        HIP_TRY(hipMemcpyAsync(h->d_tab[k], tabs[k], (size_t)h->tab_len[k] * sizeof(double), hipMemcpyHostToDevice,
                               h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->have_last = false;
    return SHUD_OK;
}

// ---------------------------------------------------------------------------------------------
// eval
// ---------------------------------------------------------------------------------------------
// on the comm stream, once y is ready on the main stream (ev_pack): pack the owned states peers need, then the
// grouped RCCL send/recv; ev_comm marks the ghost buffers filled.  The main stream meanwhile runs the interior
// elements, so the pack (~4 us at 8 ranks) and the exchange leave the critical path.  s_comm is in order and
// waits for everything enqueued on the main stream before this eval, so neither the send buffers nor the
// ghost buffers are rewritten while the previous eval still reads them.
static int exchange(shud_rhs *h, const double *y) {
    if (!h->partitioned) return 0;
    HIP_TRY(hipEventRecord(h->ev_pack, h->stream));
    HIP_TRY(hipStreamWaitEvent(h->s_comm, h->ev_pack, 0));
    launch_pack_kernel(y, h->n_own, h->n_own_riv, h->d_esend_idx, h->n_esend, h->d_rsend_idx, h->n_rsend,
                       h->d_esend, h->d_rsend, h->s_comm);
    if (h->use_nccl) {
    NCCL_TRY(ncclGroupStart());
    for (int p = 0; p < h->nranks; p++) {
        if (p == h->rank) continue;
        size_t se = h->esend_off[p + 1] - h->esend_off[p], re = h->erecv_off[p + 1] - h->erecv_off[p];
        size_t sr = h->rsend_off[p + 1] - h->rsend_off[p], rr = h->rrecv_off[p + 1] - h->rrecv_off[p];
        if (se) NCCL_TRY(ncclSend(h->d_esend + 3 * (size_t)h->esend_off[p], 3 * se, ncclDouble, p, h->comm, h->s_comm));
        if (re) NCCL_TRY(ncclRecv(h->d_gele + 3 * (size_t)h->erecv_off[p], 3 * re, ncclDouble, p, h->comm, h->s_comm));
        if (sr) NCCL_TRY(ncclSend(h->d_rsend + h->rsend_off[p], sr, ncclDouble, p, h->comm, h->s_comm));
        if (rr) NCCL_TRY(ncclRecv(h->d_griv + h->rrecv_off[p], rr, ncclDouble, p, h->comm, h->s_comm));
    }
    NCCL_TRY(ncclGroupEnd());
    }                                // external transport (tests): the caller placed the ghost buffers
    if (h->dbg_armed) {              // test hook: the halo arrives late (spin), written by a kernel, or never
        if (h->dbg_spin) launch_spin(h->dbg_spin, h->s_comm);
        if (h->dbg_gele) launch_copy_f64(h->d_gele, h->dbg_gele, 3 * (size_t)h->n_eghost, h->s_comm);
        if (h->dbg_griv) launch_copy_f64(h->d_griv, h->dbg_griv, (size_t)h->n_rghost, h->s_comm);
    }
    ++h->halo_epoch;
    if (h->fold && !(h->dbg_armed && !h->dbg_publish)) launch_halo_flag(h->d_halo_flag, h->halo_epoch, h->s_comm);
    HIP_TRY(hipEventRecord(h->ev_comm, h->s_comm));
    h->n_exch++;
    return 0;
}

static void launch_ele(shud_rhs *h, const double *y, double *dy, int cur, int cur_e, bool diag, int i0 = 0,
                       int i1 = -1) {
    YView Y{y, h->d_gele, h->d_griv, h->n_own, h->n_own_riv};
    if (i1 < 0) i1 = h->n_own + h->n_segghost;
    // the last element launch of an eval (after the halo in every partitioned path) carries the QrivDown pre-pass
    const bool last = i1 == h->n_own + h->n_segghost;
    if (h->packed) {
        const bool qd = launch_element_kernel_packed(h->dm, h->dp, Y, dy, i0, i1, cur, h->mode, h->open, diag,
                                                     h->fu_unit[0] && h->fu_unit[1], h->dd, h->stream,
                                                     h->lakeon ? &h->lk : nullptr, h->partitioned && i1 <= h->n_int,
                                                     last);
        if (last) h->qd_now = qd;
    } else {
        launch_element_kernel(h->dm, Y, dy, h->n_own + h->n_segghost, cur, cur_e, h->mode, h->open, diag, h->dd,
                              h->stream);
        h->qd_now = false;
    }
}
static void launch_riv(shud_rhs *h, const double *y, double *dy, bool diag) {
    YView Y{y, h->d_gele, h->d_griv, h->n_own, h->n_own_riv};
    if (h->packed)
        launch_river_kernel_packed(h->dm, h->dp, Y, dy, h->mode, diag, h->dd, h->stream, h->qd_now);
    else
        launch_river_kernel(h->dm, Y, dy, h->mode, diag, h->dd, h->stream);
    if (h->lakeon) launch_lake_kernel(h->dm, h->dp, h->lk, Y, dy, diag, h->dd, h->stream);
}
static void launch_all(shud_rhs *h, const double *y, double *dy, int cur, int cur_e, bool diag) {
    launch_ele(h, y, dy, cur, cur_e, diag);
    launch_riv(h, y, dy, diag);
}
// carried-state ping-pong after an eval: the packed record carries {u_satn, e_ic} together
static void flip(shud_rhs *h) {
    h->cur ^= 1;
    if (h->packed) h->cur_e = h->cur;
    else if (h->mode == SHUD_MODE_SERIAL) h->cur_e ^= 1;
}

int shud_read_err(shud_rhs *h) {
    HIP_TRY(hipMemcpyAsync(h->h_err, h->d_err, sizeof(DevErr), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->h_err->n_warn = 0;
    if (h->h_err->flags & SHUD_EF_AET_WARN) {          // the only counted report
        HIP_TRY(hipMemcpyAsync(h->h_warn, h->d_warn, kWarnSlots * kWarnStride * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        for (int k = 0; k < kWarnSlots; k++) h->h_err->n_warn += h->h_warn[k * kWarnStride];
    }
    // a halo poll timed out: the pack / exchange it gave up on may still be running — drain the comm stream before
    // the failure reaches the caller, so nothing of that eval is still in flight when the caller reacts
    if ((h->h_err->flags & SHUD_EF_HALO_WAIT) && h->s_comm) HIP_TRY(hipStreamSynchronize(h->s_comm));
    return 0;
}
static int read_err(shud_rhs *h) { return shud_read_err(h); }

static const uint32_t kFatal = SHUD_EF_NAN_QELE | SHUD_EF_EFFKH | SHUD_EF_ET_NEG | SHUD_EF_ET_NAN | SHUD_EF_HALO_WAIT;

// partitioned handles: the interior elements [0, n_int) run while the halo exchange is in flight (RCCL on
// s_comm); boundary + ghost elements and the reaches wait for it.  Unpartitioned: one launch each.
// stream_halo: the halo is already ordered on the main stream (eval_compute, external transport) — the folded
// launch's boundary workgroups then skip the flag
static int launch_split(shud_rhs *h, const double *y, double *dy, hipEvent_t e_mid = nullptr,
                        bool stream_halo = false) {
    // an RCCL communicator connects its peers lazily on the first send/recv (can take far longer than any eval):
    // that first exchange is waited for on the stream (split path), never polled by workgroups
    const bool first_rccl = h->use_nccl && h->n_exch <= 1 && !stream_halo;
    if (h->fold && h->packed && !h->lakeon && !first_rccl) {
        YView Y{y, h->d_gele, h->d_griv, h->n_own, h->n_own_riv};
        const HaloWait hw{h->d_halo_flag, stream_halo ? 0ull : h->halo_epoch, h->halo_timeout};
        if (launch_element_kernel_packed_fold(h->dm, h->dp, Y, dy, h->n_int, h->n_own + h->n_segghost, h->cur,
                                              h->mode, h->open, h->fu_unit[0] && h->fu_unit[1], h->dd, hw,
                                              h->stream, true)) {
            h->qd_now = h->dp.qdown != nullptr && h->dp.nqd > 0;
            if (e_mid) HIP_TRY(hipEventRecord(e_mid, h->stream));
            launch_riv(h, y, dy, false);             // after the boundary workgroups, which saw the halo
            // optional join of the comm stream (normally complete long before: the boundary workgroups saw its flag),
            // so that after a poll timeout no later main-stream work runs beside the late pack / exchange
            if (h->fold_join && !stream_halo) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_comm, 0));
            HIP_TRY(hipGetLastError());
            return 0;
        }
    }
    if (h->partitioned && h->packed && h->n_int > 0) {
        launch_ele(h, y, dy, h->cur, h->cur_e, false, 0, h->n_int);
        HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_comm, 0));
        launch_ele(h, y, dy, h->cur, h->cur_e, false, h->n_int, h->n_own + h->n_segghost);
        if (e_mid) HIP_TRY(hipEventRecord(e_mid, h->stream));
        launch_riv(h, y, dy, false);
    } else {
        if (h->partitioned) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_comm, 0));
        launch_ele(h, y, dy, h->cur, h->cur_e, false);
        if (e_mid) HIP_TRY(hipEventRecord(e_mid, h->stream));
        launch_riv(h, y, dy, false);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

static int eval_device(shud_rhs *h, double t, const double *y, double *dy) {
    (void)t;
    hipEvent_t *E = nullptr;
    if (h->tm_n < h->tm_cap && (h->tm_seen++ % h->tm_stride) == 0) E = &h->tm_ev[3 * (size_t)h->tm_n++];
    if (E) HIP_TRY(hipEventRecord(E[0], h->stream));
    int rc = exchange(h, y);
    if (rc) return rc;
    h->last_cur = h->cur;
    h->last_cur_e = h->cur_e;
    if ((rc = launch_split(h, y, dy, E ? E[1] : nullptr))) return rc;
    if (E) HIP_TRY(hipEventRecord(E[2], h->stream));
    flip(h);
    h->last_y = y;
    h->have_last = true;
    h->ncalls++;
    return 0;
}

extern "C" int shud_rhs_eval(shud_rhs_t h, double t, const double *y, double *ydot, int where) {
    if (!h || !y || !ydot) return shud_fail(SHUD_ERR_ARG, "null argument");
    const size_t ny = 3 * (size_t)h->n_own + h->n_own_riv + h->NL;
    if (where == SHUD_WHERE_DEVICE) return eval_device(h, t, y, ydot);
    if (where != SHUD_WHERE_HOST) return shud_fail(SHUD_ERR_ARG, "bad where");
    HIP_TRY(hipSetDevice(h->device));
    // ordered handle: y lands in the caller-numbered stage, one permute launch carries it into d_y; ydot goes back
    // through the same stage before its D2H copy
    const int ntail = h->n_own_riv + h->NL;
    HIP_TRY(hipMemcpyAsync(h->ordered ? h->d_stage : h->d_y, y, ny * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (h->ordered) {
        launch_perm_kernel(h->d_perm, h->NE, 3, h->d_stage, h->d_y, ntail, h->stream);
        HIP_TRY(hipGetLastError());
    }
    int rc = eval_device(h, t, h->d_y, h->d_ydot);
    if (rc) return rc;
    if (h->ordered) {
        launch_perm_kernel(h->d_inv, h->NE, 3, h->d_ydot, h->d_stage, ntail, h->stream);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(ydot, h->ordered ? h->d_stage : h->d_ydot, ny * sizeof(double), hipMemcpyDeviceToHost,
                           h->stream));
    if (h->check_errors) {
        if ((rc = read_err(h))) return rc;
        if (h->h_err->flags & kFatal) return shud_fail(SHUD_ERR_PHYSICS, "physics error flags 0x%x", h->h_err->flags);
    } else {
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return SHUD_OK;
}

extern "C" long long shud_rhs_num_calls(shud_rhs_t h) { return h ? h->ncalls : -1; }

extern "C" int shud_rhs_layout_streamed(shud_rhs_t h, int *n_streamed) {
    if (!h || !n_streamed) return shud_fail(SHUD_ERR_ARG, "null argument");
    *n_streamed = h->packed ? h->dp.nh : 0;
    return SHUD_OK;
}

extern "C" int shud_rhs_layout_shared(shud_rhs_t h, int *n_shared) {
    if (!h || !n_shared) return shud_fail(SHUD_ERR_ARG, "null argument");
    *n_shared = h->packed ? h->n_shared : 0;
    return SHUD_OK;
}

extern "C" int shud_rhs_layout(shud_rhs_t h, int *packed, int *n_classes) {
    if (!h) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (packed) *packed = h->packed ? 1 : 0;
    if (n_classes) *n_classes = h->n_classes;
    return SHUD_OK;
}

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
extern "C" int shud_rhs_get_error(shud_rhs_t h, ShudErr *e) {
    if (!h || !e) return shud_fail(SHUD_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    int rc = read_err(h);
    if (rc) return rc;
    const DevErr &d = *h->h_err;         // an ordered handle's kernels recorded the caller's indices (DevErr::map)
    memset(e, 0, sizeof(*e));
    e->flags = d.flags;
    for (int k = 0; k < 8; k++) e->first_index[k] = (d.first_index[k] == INT_MAX) ? -1 : d.first_index[k];
    e->n_aet_warn = (int64_t)d.n_warn;
    // ET-step prelude (shud_et_step): tReadForcing's CheckNonZero(ra) then CheckNANi(qPotTran), per element
    if (d.flags & (SHUD_EF_ET_RA | SHUD_EF_ET_PT_NAN)) {
        const int ra = (d.flags & SHUD_EF_ET_RA) ? d.first_index[5] : INT_MAX;
        const int pt = (d.flags & SHUD_EF_ET_PT_NAN) ? d.first_index[6] : INT_MAX;
        e->exit_code = 10;
        if (ra <= pt)
            snprintf(e->message, sizeof(e->message),
                     "ERROR: Value for Aerodynamic Resistance of Element %d is not allowed. Please check again.", ra + 1);
        else
            snprintf(e->message, sizeof(e->message), "ERROR: NAN error for qPotTran[i] %d", pt + 1);
        return SHUD_OK;
    }
    // the reference stops at the first myexit() in loop order: loop A (f_etFlux then effKH, per element,
    // MD_f.cpp:11-26), then the applyDY NaN check (MD_f.cpp:73-74)
    int et = INT_MAX;
    if (d.flags & SHUD_EF_ET_NEG) et = std::min(et, d.first_index[2]);
    if (d.flags & SHUD_EF_ET_NAN) et = std::min(et, d.first_index[3]);
    int kh = (d.flags & SHUD_EF_EFFKH) ? d.first_index[1] : INT_MAX;
    if (et != INT_MAX || kh != INT_MAX) {
        if (et <= kh) {
            e->exit_code = 10;
            bool neg = (d.flags & SHUD_EF_ET_NEG) && d.first_index[2] == et;
            snprintf(e->message, sizeof(e->message), neg ? "ERROR: Negative ET flux of Element %d is not allowed."
                                                         : "ERROR: NAN error for ET flux %d", et + 1);
        } else {
            e->exit_code = 13;
            snprintf(e->message, sizeof(e->message), "Wrong effKH for ground water (element %d)", kh + 1);
        }
    } else if (d.flags & SHUD_EF_NAN_QELE) {
        e->exit_code = 10;
        snprintf(e->message, sizeof(e->message), "ERROR: NAN error for QeleSurf/QeleSub %d", d.first_index[0] + 1);
    }
    return SHUD_OK;
}

extern "C" int shud_rhs_clear_error(shud_rhs_t h) {
    if (!h) return shud_fail(SHUD_ERR_ARG, "null argument");
    return shud_reset_err(h);
}

extern "C" int shud_rhs_cvrhs(double t, const double *y, double *ydot, void *user_data) {
    shud_rhs *h = (shud_rhs *)user_data;
    int rc = shud_rhs_eval(h, t, y, ydot, SHUD_WHERE_HOST);
    if (rc == SHUD_OK) return 0;
    if (rc == SHUD_ERR_PHYSICS && env_knob("SHUD_RHS_STRICT_EXIT", 0, 0, 1)) {
        ShudErr e;
        shud_rhs_get_error(h, &e);
        printf("\n%s\n", e.message);
        fprintf(stderr, "\nEXIT with error code %d\n", e.exit_code);
        exit(e.exit_code);
    }
    return -1;
}

// ---------------------------------------------------------------------------------------------
// diagnostics (replay of the last call with DIAG kernels)
// ---------------------------------------------------------------------------------------------
int shud_ensure_diag(shud_rhs *h) {
    if (h->have_diag) return 0;
    const size_t NE = h->NE, NR = h->NR;
    double **e1[] = {&h->dd.qele_surf_tot, &h->dd.qele_sub_tot, &h->dd.q_infil, &h->dd.q_exfil, &h->dd.q_recharge,
                     &h->dd.q_es, &h->dd.q_eu, &h->dd.q_eg, &h->dd.q_tu, &h->dd.q_tg, &h->dd.q_eta,
                     &h->dd.e_ic, &h->dd.u_satn, &h->dd.i_beta, &h->dd.eff_kh, &h->dd.qe2r_surf, &h->dd.qe2r_sub};
    int rc;
    for (auto pp : e1)
        if ((rc = h->upload(pp, (const double *)nullptr, NE))) return rc;
    if ((rc = h->upload(&h->dd.qele_surf, (const double *)nullptr, 3 * NE))) return rc;
    if ((rc = h->upload(&h->dd.qele_sub, (const double *)nullptr, 3 * NE))) return rc;
    double **r1[] = {&h->dd.qriv_down, &h->dd.qriv_up, &h->dd.qriv_surf, &h->dd.qriv_sub};
    for (auto pp : r1)
        if ((rc = h->upload(pp, (const double *)nullptr, NR))) return rc;
    double **l1[] = {&h->dd.q_lake_surf, &h->dd.q_lake_sub, &h->dd.q_lake_rivin, &h->dd.q_lake_evap,
                     &h->dd.q_lake_prcp, &h->dd.lake_toparea};
    for (auto pp : l1)
        if ((rc = h->upload(pp, (const double *)nullptr, std::max(h->NL, 1)))) return rc;
    h->have_diag = true;
    return 0;
}

// replay of the last evaluation with diagnostic stores: same y, same carried-state inputs (it rewrites the
// same carried outputs), ydot into scratch; stream-ordered, the diagnostics stay in HBM (DevDiag)
int shud_diag_replay(shud_rhs *h) {
    if (!h->have_last) return shud_fail(SHUD_ERR_ARG, "no evaluation to report diagnostics for");
    HIP_TRY(hipSetDevice(h->device));
    int rc = shud_ensure_diag(h);
    if (rc) return rc;
    launch_all(h, h->last_y, h->d_scratch_dy, h->last_cur, h->last_cur_e, true);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int shud_rhs_sync_diagnostics(shud_rhs_t h, ShudFluxOut *o) {
    if (!h || !o) return shud_fail(SHUD_ERR_ARG, "null argument");
    int rc = shud_diag_replay(h);
    if (rc) return rc;
    const size_t NE = h->NE, NR = h->NR, NS = h->NS;
    // planes: 1 = an [NE] array, 3 = a [3*NE] edge-major array (an ordered handle carries these to the caller's
    // numbering through the stage; the stream is in order, so the stage is free again once the copy before it has
    // run); 0 = per reach or per lake, copied as it is
    auto get = [&](double *dst, const double *src, size_t n, int planes) -> int {
        if (!dst || !n) return 0;
        if (h->ordered && planes) {
            launch_perm_kernel(h->d_inv, h->NE, planes, src, h->d_stage, 0, h->stream);
            HIP_TRY(hipGetLastError());
            src = h->d_stage;
        }
        HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        return 0;
    };
    const DevDiag &g = h->dd;
    const size_t NL = h->NL;
    struct { double *dst; const double *src; size_t n; int planes; } arrs[] = {
        {o->qele_surf, g.qele_surf, 3 * NE, 3}, {o->qele_sub, g.qele_sub, 3 * NE, 3},
        {o->qele_surf_tot, g.qele_surf_tot, NE, 1}, {o->qele_sub_tot, g.qele_sub_tot, NE, 1},
        {o->q_infil, g.q_infil, NE, 1}, {o->q_exfil, g.q_exfil, NE, 1}, {o->q_recharge, g.q_recharge, NE, 1},
        {o->q_es, g.q_es, NE, 1}, {o->q_eu, g.q_eu, NE, 1}, {o->q_eg, g.q_eg, NE, 1}, {o->q_tu, g.q_tu, NE, 1},
        {o->q_tg, g.q_tg, NE, 1}, {o->q_eta, g.q_eta, NE, 1}, {o->e_ic, g.e_ic, NE, 1}, {o->u_satn, g.u_satn, NE, 1},
        {o->i_beta, g.i_beta, NE, 1}, {o->eff_kh, g.eff_kh, NE, 1}, {o->qe2r_surf, g.qe2r_surf, NE, 1},
        {o->qe2r_sub, g.qe2r_sub, NE, 1},
        {o->qriv_down, g.qriv_down, NR, 0}, {o->qriv_up, g.qriv_up, NR, 0}, {o->qriv_surf, g.qriv_surf, NR, 0},
        {o->qriv_sub, g.qriv_sub, NR, 0},
        {o->q_lake_surf, g.q_lake_surf, NL, 0}, {o->q_lake_sub, g.q_lake_sub, NL, 0},
        {o->q_lake_rivin, g.q_lake_rivin, NL, 0}, {o->q_lake_evap, g.q_lake_evap, NL, 0},
        {o->q_lake_prcp, g.q_lake_prcp, NL, 0}, {o->lake_toparea, g.lake_toparea, NL, 0}};
    for (const auto &a : arrs)
        if ((rc = get(a.dst, a.src, a.n, a.planes))) return rc;
    std::vector<double> tmp;
    if (o->qseg_surf || o->qseg_sub) tmp.resize(std::max<size_t>(NS, 1));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const std::vector<int> &perm = h->seg_perm;
    if (h->packed && NS && (o->qseg_surf || o->qseg_sub)) {
        std::vector<double2> q2(NS);
        HIP_TRY(hipMemcpy(q2.data(), h->dp.qseg2, NS * sizeof(double2), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < NS; k++) {
            if (o->qseg_surf) o->qseg_surf[perm[k]] = q2[k].x;
            if (o->qseg_sub) o->qseg_sub[perm[k]] = q2[k].y;
        }
        return SHUD_OK;
    }
    if (o->qseg_surf) {
        HIP_TRY(hipMemcpy(tmp.data(), h->dm.qseg_surf, NS * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < NS; k++) o->qseg_surf[perm[k]] = tmp[k];
    }
    if (o->qseg_sub) {
        HIP_TRY(hipMemcpy(tmp.data(), h->dm.qseg_sub, NS * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < NS; k++) o->qseg_sub[perm[k]] = tmp[k];
    }
    return SHUD_OK;
}

// ---------------------------------------------------------------------------------------------
// measurement helpers
// ---------------------------------------------------------------------------------------------
extern "C" int shud_rhs_device_alloc(shud_rhs_t h, size_t bytes, void **dptr) {
    if (!h || !dptr) return shud_fail(SHUD_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMalloc(dptr, bytes ? bytes : 8));
    return SHUD_OK;
}
extern "C" int shud_rhs_device_free(shud_rhs_t h, void *dptr) {
    (void)h;
    HIP_TRY(hipFree(dptr));
    return SHUD_OK;
}
extern "C" int shud_rhs_memcpy(shud_rhs_t h, void *dst, const void *src, size_t bytes, int kind) {
    if (!h) return shud_fail(SHUD_ERR_ARG, "null argument");
    hipMemcpyKind k = kind == 1 ? hipMemcpyHostToDevice : kind == 2 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, k, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SHUD_OK;
}
extern "C" int shud_rhs_synchronize(shud_rhs_t h) {
    if (!h) return shud_fail(SHUD_ERR_ARG, "null argument");
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SHUD_OK;
}
extern "C" void *shud_rhs_stream(shud_rhs_t h) { return h ? (void *)h->stream : nullptr; }

// halo buffers of a partitioned handle (external-transport tests move them between handles)
extern "C" int shud_rhs_halo_buffers(shud_rhs_t h, double **esend, double **rsend, double **gele, double **griv) {
    if (!h || !h->partitioned) return shud_fail(SHUD_ERR_ARG, "not a partitioned handle");
    *esend = h->d_esend; *rsend = h->d_rsend; *gele = h->d_gele; *griv = h->d_griv;
    return SHUD_OK;
}
// test hook: a late, kernel-written or missing halo on the comm stream of every following device eval
extern "C" int shud_rhs_debug_halo(shud_rhs_t h, double spin_us, const double *d_ele_src, const double *d_riv_src,
                                   int publish, double timeout_ms) {
    if (!h || !h->partitioned) return shud_fail(SHUD_ERR_ARG, "not a partitioned handle");
    if (spin_us < 0 || spin_us > 1e7) return shud_fail(SHUD_ERR_ARG, "spin_us out of range");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipStreamSynchronize(h->s_comm));
    h->dbg_spin = (unsigned long long)(spin_us * 1e-3 * h->wall_khz);
    h->dbg_gele = d_ele_src;
    h->dbg_griv = d_riv_src;
    h->dbg_publish = publish != 0;
    h->dbg_armed = h->dbg_spin || d_ele_src || d_riv_src || !h->dbg_publish;
    const double ms = timeout_ms > 0 ? timeout_ms : env_knob("SHUD_HALO_TIMEOUT_MS", 5000, 1, 3600000);
    h->halo_timeout = (unsigned long long)(ms * h->wall_khz);
    return SHUD_OK;
}
// split eval for external transport: pack, (caller exchanges), compute
extern "C" int shud_rhs_eval_pack(shud_rhs_t h, const double *d_y) {
    if (!h || !h->partitioned) return shud_fail(SHUD_ERR_ARG, "not a partitioned handle");
    launch_pack_kernel(d_y, h->n_own, h->n_own_riv, h->d_esend_idx, h->n_esend, h->d_rsend_idx, h->n_rsend,
                       h->d_esend, h->d_rsend, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev_comm, h->stream));      // what eval_compute's boundary launch waits for
    return SHUD_OK;
}
extern "C" int shud_rhs_eval_compute(shud_rhs_t h, double t, const double *d_y, double *d_ydot) {
    (void)t;
    if (!h) return shud_fail(SHUD_ERR_ARG, "null argument");
    h->last_cur = h->cur;
    h->last_cur_e = h->cur_e;
    int rc = launch_split(h, d_y, d_ydot, nullptr, true);
    if (rc) return rc;
    flip(h);
    h->last_y = d_y;
    h->have_last = true;
    h->ncalls++;
    return SHUD_OK;
}

extern "C" int shud_rhs_timing(shud_rhs_t h, int max_evals, int stride) {
    if (!h || max_evals < 0 || stride < 1) return shud_fail(SHUD_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t need = 3 * (size_t)max_evals;
    while (h->tm_ev.size() < need) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, kEvTime));
        h->tm_ev.push_back(e);
    }
    h->tm_cap = max_evals;
    h->tm_n = 0;
    h->tm_seen = 0;
    h->tm_stride = stride;
    return SHUD_OK;
}

extern "C" int shud_rhs_timing_read(shud_rhs_t h, double *ms_ele, double *ms_riv, double *ms_eval, int *n_evals) {
    if (!h) return shud_fail(SHUD_ERR_ARG, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    double a = 0., b = 0., c = 0.;
    for (int r = 0; r < h->tm_n; r++) {
        hipEvent_t *E = &h->tm_ev[3 * (size_t)r];
        float x = 0.f, y = 0.f, z = 0.f;
        HIP_TRY(hipEventElapsedTime(&x, E[0], E[1]));
        HIP_TRY(hipEventElapsedTime(&y, E[1], E[2]));
        HIP_TRY(hipEventElapsedTime(&z, E[0], E[2]));
        a += x; b += y; c += z;
    }
    const int n = h->tm_n;
    if (ms_ele) *ms_ele = n ? a / n : 0.;
    if (ms_riv) *ms_riv = n ? b / n : 0.;
    if (ms_eval) *ms_eval = n ? c / n : 0.;
    if (n_evals) *n_evals = n;
    h->tm_n = 0;
    h->tm_cap = 0;
    return SHUD_OK;
}

extern "C" int shud_rhs_time_kernels(shud_rhs_t h, double t, const double *d_y, double *d_ydot, int reps,
                                     double *ms_eval, double *ms_out, int *nk, char *names_out, int names_len) {
    (void)t;
    if (!h || reps <= 0) return shud_fail(SHUD_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    const int K = h->partitioned ? 3 : 2;
    std::vector<hipEvent_t> ev((size_t)reps * (K + 1));
    for (auto &e : ev) HIP_TRY(hipEventCreateWithFlags(&e, kEvTime));
    for (int r = 0; r < reps; r++) {
        hipEvent_t *E = &ev[(size_t)r * (K + 1)];
        int k = 0;
        HIP_TRY(hipEventRecord(E[k++], h->stream));
        if (h->partitioned) {
            int rc = exchange(h, d_y);        // serialized here (no overlap) so each phase is timed alone
            if (rc) return rc;
            HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_comm, 0));
            HIP_TRY(hipEventRecord(E[k++], h->stream));
        }
        launch_ele(h, d_y, d_ydot, h->cur, h->cur_e, false);
        HIP_TRY(hipEventRecord(E[k++], h->stream));
        launch_riv(h, d_y, d_ydot, false);
        HIP_TRY(hipEventRecord(E[k++], h->stream));
        h->last_cur = h->cur; h->last_cur_e = h->cur_e;
        flip(h);
        h->last_y = d_y; h->have_last = true; h->ncalls++;
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::vector<double> acc(K, 0.0);
    double tot = 0.0;
    for (int r = 0; r < reps; r++) {
        hipEvent_t *E = &ev[(size_t)r * (K + 1)];
        for (int k = 0; k < K; k++) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, E[k], E[k + 1]));
            acc[k] += ms;
        }
        float all = 0.f;
        HIP_TRY(hipEventElapsedTime(&all, E[0], E[K]));
        tot += all;
    }
    for (auto &e : ev) (void)hipEventDestroy(e);
    const char *nm = h->partitioned ? "halo_exchange,shud_ele_kernel,shud_riv_kernel" : "shud_ele_kernel,shud_riv_kernel";
    int n = std::min(*nk, K);
    for (int k = 0; k < n; k++) ms_out[k] = acc[k] / reps;
    *nk = K;
    if (ms_eval) *ms_eval = tot / reps;
    if (names_out && names_len > 0) snprintf(names_out, names_len, "%s", nm);
    return SHUD_OK;
}
