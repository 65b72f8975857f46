// shud_ckpt.cpp — host side of the exact checkpoint / resume (include/shud_ckpt.h): which buffers and scalars of
// each object a checkpoint holds, the snapshot's pack pass and background drain, and the restore.
//
// A snapshot lists the live device buffers of the objects (the RHS handle's here; the integrator's, the ET prelude's
// and the output set's through csrc/shud_ckpt_parts.h), lays them out in one staging slab, and enqueues the pack
// kernel (shud_ckpt.hip): one pass over HBM that copies them and forms their checksums.  The host scalars go into
// byte archives.  The call returns; a writer thread then moves the slab through two pinned banks on a copy stream
// into <path>.tmp (copy of chunk k + 1 in flight while chunk k is written), flushes and renames it.
// A restore reads and verifies the file, checks every header field and section size against the objects and the
// statics fingerprint against the handle's static tables, and only then uploads, verifies the upload with the
// kernel's checksum-only mode and sets the scalars: a refused restore leaves the objects as they were.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <cerrno>
#include <climits>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "shud_ckpt_dev.h"
#include "shud_ckpt_parts.h"
#include "shud_diag_host.h"
#include "shud_handle.h"

using namespace shud::ckpt;

namespace {

constexpr size_t kBankWords = (8u << 20) / 8;          // two pinned banks of 8 MiB, whatever the slab's size
constexpr int kMaxDev = SHUD_CKPT_MAX_SECTIONS;

struct Layout {                                        // where each device buffer sits in the slab
    std::vector<uint64_t> off;
    uint64_t words = 0;
};
Layout lay_out(const std::vector<CkptDev> &dev, uint64_t guard) {
    Layout L;
    uint64_t at = guard;
    for (const auto &d : dev) {
        at = place(at, d.p);
        L.off.push_back(at);
        at += d.bytes / 8 + guard;
    }
    L.words = at;
    return L;
}

// the pack kernel over dev, kMaxSeg buffers per launch; off == nullptr or dst == nullptr: checksums only.
// d_sums[2 k], d_sums[2 k + 1] receive buffer k's sums (zeroed here, stream-ordered).
int pack_launch(const std::vector<CkptDev> &dev, const std::vector<uint64_t> *off, uint64_t *dst,
                unsigned long long *d_sums, hipStream_t s) {
    if (dev.empty()) return SHUD_OK;
    HIP_TRY(hipMemsetAsync(d_sums, 0, 2 * dev.size() * sizeof(unsigned long long), s));
    for (size_t k0 = 0; k0 < dev.size(); k0 += kMaxSeg) {
        SegTable t{};
        uint32_t nblk = 0;
        const size_t n = std::min<size_t>(kMaxSeg, dev.size() - k0);
        for (size_t k = 0; k < n; k++) {
            const CkptDev &d = dev[k0 + k];
            if ((uintptr_t)d.p & 7u) return shud_fail(SHUD_ERR_ARG, "shud_ckpt: buffer %s is not 8-byte aligned", d.name);
            t.s[k] = Seg{(const uint64_t *)d.p, off ? (*off)[k0 + k] : 0, d.bytes / 8, nblk, 0};
            nblk += seg_blocks(d.p, d.bytes / 8);
        }
        t.nseg = (int)n;
        t.nblk = nblk;
        launch_pack(t, off ? dst : nullptr, d_sums + 2 * k0, s);
        HIP_TRY(hipGetLastError());
    }
    return SHUD_OK;
}

// ---- the RHS handle ----
const uint32_t kErrSet = SHUD_EF_NAN_QELE | SHUD_EF_EFFKH | SHUD_EF_ET_NEG | SHUD_EF_ET_NAN | SHUD_EF_HALO_WAIT |
                         SHUD_EF_ET_RA | SHUD_EF_ET_PT_NAN;

int rhs_check(shud_rhs *h, ShudCkptInfo *hdr, bool restore) {
    if (h->partitioned)
        return shud_fail(SHUD_ERR_UNSUPPORTED, "shud_ckpt: partitioned handles cannot be checkpointed");
    HIP_TRY(hipSetDevice(h->device));
    int rc = shud_read_err(h);                          // synchronizes the handle's stream
    if (rc) return rc;
    if (h->h_err->flags & kErrSet)
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt: the handle's error word is set (flags 0x%x)", h->h_err->flags);
    uint64_t pc[2] = {0, 0};
    if (!h->perm.empty()) {
        std::vector<uint64_t> w((h->perm.size() + 1) / 2, 0);
        memcpy(w.data(), h->perm.data(), h->perm.size() * sizeof(int));
        shud_ckpt_checksum(w.data(), w.size(), &pc[0], &pc[1]);
    }
    const int32_t layout = !h->packed ? SHUD_CKPT_LAYOUT_SOA : h->dp.nh ? SHUD_CKPT_LAYOUT_HYBRID : SHUD_CKPT_LAYOUT_PACKED;
    const int64_t ny = 3 * (int64_t)h->n_own + h->n_own_riv + h->NL;
    if (!restore) {
        hdr->ne = h->NE; hdr->nr = h->NR; hdr->ns = h->NS; hdr->nl = h->NL; hdr->ny = ny;
        hdr->mode = h->mode; hdr->layout = layout; hdr->n_classes = h->n_classes; hdr->n_streamed = h->packed ? h->dp.nh : 0;
        hdr->n_shared = h->n_shared; hdr->order_kind = h->order_kind; hdr->perm_c0 = pc[0]; hdr->perm_c1 = pc[1];
        return SHUD_OK;
    }
    auto bad = [](const char *f, long long file, long long obj) {
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: field %s differs (file %lld, handle %lld)", f, file, obj);
    };
    if (hdr->ne != h->NE) return bad("NE", hdr->ne, h->NE);
    if (hdr->nr != h->NR) return bad("NR", hdr->nr, h->NR);
    if (hdr->ns != h->NS) return bad("NS", hdr->ns, h->NS);
    if (hdr->nl != h->NL) return bad("NL", hdr->nl, h->NL);
    if (hdr->ny != ny) return bad("NY", hdr->ny, ny);
    if (hdr->mode != h->mode) return bad("mode", hdr->mode, h->mode);
    if (hdr->layout != layout) return bad("layout", hdr->layout, layout);
    if (hdr->order_kind != h->order_kind) return bad("order_kind", hdr->order_kind, h->order_kind);
    if (hdr->perm_c0 != pc[0] || hdr->perm_c1 != pc[1]) return bad("perm checksum", (long long)hdr->perm_c0, (long long)pc[0]);
    return SHUD_OK;
}
// the layout counts follow from the static tables: compared after the statics fingerprint, which says more
int rhs_check_counts(shud_rhs *h, const ShudCkptInfo *hdr) {
    auto bad = [](const char *f, long long file, long long obj) {
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: field %s differs (file %lld, handle %lld)", f, file, obj);
    };
    if (hdr->n_classes != h->n_classes) return bad("n_classes", hdr->n_classes, h->n_classes);
    if (hdr->n_streamed != (h->packed ? h->dp.nh : 0)) return bad("n_streamed", hdr->n_streamed, h->dp.nh);
    if (hdr->n_shared != h->n_shared) return bad("n_shared", hdr->n_shared, h->n_shared);
    return SHUD_OK;
}

// the buffers an evaluation, an ET step or an export reads before writing.  file != nullptr (restore): the replay
// vector lands in the handle's own d_y, and a summary array the file holds and the handle lacks is listed without a
// pointer (rhs_alloc_sums allocates it once every check has passed).
int rhs_dev(shud_rhs *h, CkptPart &p, const CkptFile *file) {
    const size_t E = (size_t)h->NE, D = sizeof(double), NS = (size_t)h->NS;
    const DevMesh &d = h->dm;
    const struct { const char *name; const double *ptr; } soa[] = {
        {"rhs.net_prep", d.net_prep}, {"rhs.pot_evap", d.pot_evap}, {"rhs.pot_tran", d.pot_tran}, {"rhs.etp", d.etp},
        {"rhs.lai", d.lai}, {"rhs.fu_surf", d.fu_surf}, {"rhs.fu_sub", d.fu_sub}, {"rhs.prcp", d.prcp},
        {"rhs.e_ic0", d.e_ic[0]}, {"rhs.e_ic1", d.e_ic[1]}, {"rhs.u_satn0", d.u_satn[0]}, {"rhs.u_satn1", d.u_satn[1]},
        {"rhs.ugw_stale", d.ugw_stale}};
    for (const auto &a : soa) p.add(a.name, a.ptr, E * D);
    p.add("rhs.qseg_surf", d.qseg_surf, NS * D);
    p.add("rhs.qseg_sub", d.qseg_sub, NS * D);
    if (h->packed) {
        const DevPacked &P = h->dp;
        p.add("rhs.cs0", P.cs[0], E * 2 * D);
        p.add("rhs.cs1", P.cs[1], E * 2 * D);
        p.add("rhs.s_np", P.s_np, E * 2 * D);
        p.add("rhs.s_tl", P.s_tl, E * 2 * D);
        p.add("rhs.s_fu", P.s_fu, E * 2 * D);
        p.add("rhs.seg_first", P.seg_first, E * sizeof(int));       // bit 31 follows the step inputs
        p.add("rhs.qseg2", P.qseg2, NS * 2 * D);
        if (P.nqd && P.qdown) p.add("rhs.qdown", P.qdown, (size_t)h->NR * D);
    }
    if (h->lakeon) {
        p.add("rhs.bank_qs", h->lk.bank_qs, 3 * E * D);
        p.add("rhs.bank_qg", h->lk.bank_qg, 3 * E * D);
    }
    for (int k = 0; k < 4; k++) {
        char name[SHUD_CKPT_NAME_LEN];
        snprintf(name, sizeof(name), "rhs.tab%d", k);
        p.add(name, h->d_tab[k], (size_t)h->tab_len[k] * D);
    }
    const size_t len[5] = {(size_t)h->n_own, (size_t)h->n_own, (size_t)h->n_own, (size_t)h->n_own_riv, (size_t)h->NL};
    for (int k = 0; k < 5; k++) {
        char name[SHUD_CKPT_NAME_LEN];
        snprintf(name, sizeof(name), "rhs.sum%d", k);
        if (file && file->find(name) && !h->d_sum[k]) {     // allocated once every check has passed (rhs_alloc_sums)
            CkptDev e{};
            strncpy(e.name, name, SHUD_CKPT_NAME_LEN - 1);
            e.bytes = len[k] * D;
            p.dev.push_back(e);
            continue;
        }
        p.add(name, h->d_sum[k], len[k] * D);
    }
    const size_t ny = 3 * (size_t)h->n_own + h->n_own_riv + h->NL;
    if (file ? file->find("rhs.last_y") != nullptr : (h->have_last && h->last_y))
        p.add("rhs.last_y", file ? h->d_y : h->last_y, ny * D);
    return SHUD_OK;
}

// restore, after the checks: the summary arrays the file holds and the handle has not allocated yet
int rhs_alloc_sums(shud_rhs *h, CkptPart &p) {
    const size_t len[5] = {(size_t)h->n_own, (size_t)h->n_own, (size_t)h->n_own, (size_t)h->n_own_riv, (size_t)h->NL};
    for (auto &d : p.dev) {
        if (d.p || strncmp(d.name, "rhs.sum", 7) != 0) continue;
        const int k = d.name[7] - '0';
        if (k < 0 || k > 4) return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: section %s", d.name);
        if (!h->d_sum[k]) {
            const int rc = h->zeros(&h->d_sum[k], len[k]);
            if (rc) return rc;
        }
        d.p = h->d_sum[k];
    }
    return SHUD_OK;
}

int rhs_host(shud_rhs *h, CkptAr &a, bool check_only) {
    int open = h->open ? 1 : 0;
    bool eq = a.same(open);
    for (int k = 0; k < 4; k++) eq &= a.same(h->tab_len[k]);
    if (!eq) return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: field boundary mode / BC table lengths differs");
    if (check_only) return SHUD_OK;
    a.pod(h->cur); a.pod(h->cur_e); a.pod(h->ncalls); a.pod(h->fu_unit); a.pod(h->qd_now);
    a.pod(h->have_last); a.pod(h->last_cur); a.pod(h->last_cur_e);
    if (a.load) h->last_y = h->have_last ? h->d_y : nullptr;        // rhs.last_y was uploaded there
    return a.ok ? SHUD_OK : shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: section rhs.host is too short");
}

// the static device tables: what another mesh, another calibration or another layout changes
void rhs_statics(shud_rhs *h, CkptPart &p) {
    const size_t E = (size_t)h->NE, D = sizeof(double), NS = (size_t)h->NS, R = (size_t)h->NR, I = sizeof(int);
    const DevMesh &d = h->dm;
    p.add("nabr", d.nabr, 3 * E * I); p.add("eflags", d.eflags, E * I);
    const double *e1[] = {d.area, d.z_surf, d.z_bottom, d.depression, d.aq, d.macD, d.macKsatH, d.vAreaF, d.KsatH, d.KsatV,
                          d.infKsatV, d.hAreaF, d.macKsatV, d.ThetaS, d.ThetaR, d.Beta, d.infD, d.Sy, d.RzD, d.VegFrac,
                          d.ImpAF};
    for (const double *q : e1) p.add("ele", q, E * D);
    const double *e3[] = {d.edge, d.dist2nabor, d.avg_rough};
    for (const double *q : e3) p.add("ele3", q, 3 * E * D);
    if (h->open) { p.add("dist2edge", d.dist2edge, 3 * E * D); p.add("rough", d.rough, E * D); }
    p.add("seg_len", d.seg_len, NS * D); p.add("seg_cwr", d.seg_cwr, NS * D); p.add("seg_riv", d.seg_riv, NS * I);
    const double *r1[] = {d.riv_len, d.riv_slope, d.riv_d2down, d.riv_avg_rough, d.riv_depth, d.riv_bw, d.riv_bankslope,
                          d.riv_ksath, d.riv_bedthick};
    for (const double *q : r1) p.add("riv", q, R * D);
    p.add("riv_down", d.riv_down, R * I); p.add("riv_bc", d.riv_bc, R * I);
    if (h->packed) {
        const DevPacked &P = h->dp;
        p.add("ctab", P.ctab, (size_t)P.ncls * CF_STRIDE * D);
        p.add("zz", P.zz, E * 2 * D); p.add("meta", P.meta, E * 4 * I); p.add("ged", P.ged, 3 * E * 2 * D);
        if (P.nh) p.add("hv", P.hv, E * (size_t)P.hs * D);
        p.add("sg_lc", P.sg_lc, NS * 2 * D); p.add("rrec", P.rrec, 2 * R * 2 * D);
        p.add("rv", P.rv, 4 * R * 2 * D); p.add("rv_u", P.rv_u, R * 4 * I);
    }
}

// fingerprint of the statics: the checksum of the per-table sums, in table order.  d_sums: room for 2 * kMaxDev
int statics_fingerprint(shud_rhs *h, unsigned long long *d_sums, hipStream_t s, uint64_t fp[2]) {
    CkptPart st;
    rhs_statics(h, st);
    int rc = pack_launch(st.dev, nullptr, nullptr, d_sums, s);
    if (rc) return rc;
    std::vector<uint64_t> sums(2 * st.dev.size());
    HIP_TRY(hipMemcpyAsync(sums.data(), d_sums, sums.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    shud_ckpt_checksum(sums.data(), sums.size(), &fp[0], &fp[1]);
    return SHUD_OK;
}

// every listed object's device buffers (each object's stream is idle afterwards)
int collect_dev(const ShudCkptParts *p, CkptPart &part, const CkptFile *file) {
    int rc;
    if (p->rhs && (rc = rhs_dev(p->rhs, part, file))) return rc;
    if (p->rhs && p->rhs->et && (rc = shud_et_ckpt_dev(p->rhs, part))) return rc;
    if (p->ode && (rc = shud_ode_ckpt_dev(p->ode, part))) return rc;
    if (p->out && (rc = shud_out_ckpt_dev(p->out, part))) return rc;
    if ((int)part.dev.size() > kMaxDev - 8) return shud_fail(SHUD_ERR_UNSUPPORTED, "shud_ckpt: too many device buffers");
    return SHUD_OK;
}

int check_parts(const ShudCkptParts *p, ShudCkptInfo *hdr, bool restore) {
    if (!p || !p->ode) return shud_fail(SHUD_ERR_ARG, "shud_ckpt: an integrator is required");
    if (p->wb)
        return shud_fail(SHUD_ERR_UNSUPPORTED, "shud_ckpt: a run with a water-balance object cannot be checkpointed "
                                               "(shud_wb keeps accumulators of its own, which a checkpoint does not hold)");
    const int have[5] = {p->rhs ? 1 : 0, (p->rhs && p->rhs->et) ? 1 : 0, 1, p->out ? 1 : 0, p->mon ? 1 : 0};
    int rc;
    if (p->out && (rc = shud_out_ckpt_check(p->out))) return rc;
    if (p->rhs && (rc = rhs_check(p->rhs, hdr, restore))) return rc;
    if ((rc = shud_ode_ckpt_check(p->ode, hdr, restore))) return rc;
    if (!restore) {
        hdr->have_rhs = have[0]; hdr->have_et = have[1]; hdr->have_ode = have[2]; hdr->have_out = have[3];
        hdr->have_mon = have[4];
        return SHUD_OK;
    }
    const int32_t file[5] = {hdr->have_rhs, hdr->have_et, hdr->have_ode, hdr->have_out, hdr->have_mon};
    const char *nm[5] = {"have_rhs", "have_et", "have_ode", "have_out", "have_mon"};
    for (int k = 0; k < 5; k++)
        if (file[k] != have[k])
            return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: field %s differs (file %d, objects %d)", nm[k], file[k], have[k]);
    return SHUD_OK;
}

struct HostSec {
    std::string name;
    std::vector<uint64_t> words;
};
HostSec host_sec(const char *name, const std::vector<uint8_t> &b) {
    HostSec s;
    s.name = name;
    s.words.assign((b.size() + 7) / 8, 0);
    if (!b.empty()) memcpy(s.words.data(), b.data(), b.size());
    return s;
}

struct Job {
    std::string path;
    ShudCkptInfo hdr{};
    std::vector<ShudCkptSection> table;      // host sections first, then one per device buffer
    std::vector<uint64_t> host;              // the host sections' words
    size_t n_host = 0, n_dev = 0;
    uint64_t slab_words = 0;
};

}  // namespace

struct shud_ckpt {
    int device = 0;
    hipStream_t stream = nullptr, s_copy = nullptr;
    uint64_t *d_slab = nullptr;
    uint64_t slab_cap = 0;
    unsigned long long *d_sums = nullptr;
    uint64_t *h_sums = nullptr, *h_bank[2] = {nullptr, nullptr};
    hipEvent_t ev_pack = nullptr, ev_bank[2] = {nullptr, nullptr};
    std::thread writer;
    std::mutex mu;
    std::condition_variable cv;
    bool busy = false, stop = false;
    Job job;
    int werr = 0;
    std::string werr_msg;
};

static void ckpt_fail(shud_ckpt *c, int code, const std::string &msg) {
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->werr) { c->werr = code; c->werr_msg = msg; }
}

// one job: the sums, then header + table + host sections, then the slab in bank-sized chunks
static void ckpt_write(shud_ckpt *c, Job &j) {
    hipError_t he = hipStreamWaitEvent(c->s_copy, c->ev_pack, 0);
    if (he == hipSuccess && j.n_dev)
        he = hipMemcpyAsync(c->h_sums, c->d_sums, 2 * j.n_dev * 8, hipMemcpyDeviceToHost, c->s_copy);
    if (he == hipSuccess) he = hipStreamSynchronize(c->s_copy);
    if (he != hipSuccess) return ckpt_fail(c, SHUD_ERR_HIP, std::string("checkpoint pack failed: ") + hipGetErrorString(he));
    for (size_t k = 0; k < j.n_dev; k++) {
        j.table[j.n_host + k].c0 = c->h_sums[2 * k];
        j.table[j.n_host + k].c1 = c->h_sums[2 * k + 1];
    }
    shud_ckpt_fmt_seal(&j.hdr, j.table.data());
    const std::string tmp = j.path + ".tmp";
    FILE *fp = fopen(tmp.c_str(), "wb");
    if (!fp) return ckpt_fail(c, SHUD_ERR_ARG, "cannot open " + tmp + ": " + strerror(errno));
    bool ok = fwrite(&j.hdr, sizeof(j.hdr), 1, fp) == 1 &&
              fwrite(j.table.data(), sizeof(ShudCkptSection), j.table.size(), fp) == j.table.size() &&
              (j.host.empty() || fwrite(j.host.data(), 8, j.host.size(), fp) == j.host.size());
    const uint64_t nchunk = (j.slab_words + kBankWords - 1) / kBankWords;
    auto issue = [&](uint64_t k) {
        const uint64_t w0 = k * kBankWords, nw = std::min<uint64_t>(kBankWords, j.slab_words - w0);
        hipError_t e = hipMemcpyAsync(c->h_bank[k & 1], c->d_slab + w0, nw * 8, hipMemcpyDeviceToHost, c->s_copy);
        if (e == hipSuccess) e = hipEventRecord(c->ev_bank[k & 1], c->s_copy);
        return e;
    };
    if (ok && nchunk) he = issue(0);
    for (uint64_t k = 0; ok && he == hipSuccess && k < nchunk; k++) {
        he = hipEventSynchronize(c->ev_bank[k & 1]);
        if (he == hipSuccess && k + 1 < nchunk) he = issue(k + 1);   // bank (k + 1) & 1 was written out at k - 1
        if (he != hipSuccess) break;
        const uint64_t nw = std::min<uint64_t>(kBankWords, j.slab_words - k * kBankWords);
        ok = fwrite(c->h_bank[k & 1], 8, nw, fp) == nw;
    }
    (void)hipStreamSynchronize(c->s_copy);
    if (ok) ok = fflush(fp) == 0 && fsync(fileno(fp)) == 0;
    if (fclose(fp) != 0) ok = false;
    if (he != hipSuccess || !ok || rename(tmp.c_str(), j.path.c_str()) != 0) {
        remove(tmp.c_str());
        return ckpt_fail(c, he != hipSuccess ? SHUD_ERR_HIP : SHUD_ERR_ARG,
                         he != hipSuccess ? std::string("checkpoint copy failed: ") + hipGetErrorString(he)
                                          : "cannot write " + j.path + ": " + strerror(errno));
    }
}

static void ckpt_writer(shud_ckpt *c) {
    (void)hipSetDevice(c->device);
    for (;;) {
        {
            std::unique_lock<std::mutex> lk(c->mu);
            c->cv.wait(lk, [&] { return c->stop || c->busy; });
            if (!c->busy) return;
        }
        ckpt_write(c, c->job);
        {
            std::lock_guard<std::mutex> lk(c->mu);
            c->busy = false;
        }
        c->cv.notify_all();
    }
}

static int ckpt_drain(shud_ckpt *c) {
    std::unique_lock<std::mutex> lk(c->mu);
    c->cv.wait(lk, [&] { return !c->busy; });
    return c->werr;
}
static int ckpt_report(shud_ckpt *c) {
    return c->werr ? shud_fail(c->werr, "shud_ckpt: %s", c->werr_msg.c_str()) : SHUD_OK;
}

extern "C" int shud_ckpt_create(int device, void *stream, shud_ckpt_t *out) {
    if (!out) return shud_fail(SHUD_ERR_ARG, "null argument");
    *out = nullptr;
    HIP_TRY(hipSetDevice(device));
    shud_ckpt *c = new shud_ckpt;
    c->device = device;
    c->stream = (hipStream_t)stream;
    *out = c;                                // a failure below leaves a handle shud_ckpt_destroy can free
    c->writer = std::thread(ckpt_writer, c);
    HIP_TRY(hipStreamCreateWithFlags(&c->s_copy, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_pack, hipEventDisableTiming));
    for (int b = 0; b < 2; b++) {
        HIP_TRY(hipEventCreateWithFlags(&c->ev_bank[b], hipEventDisableTiming));
        HIP_TRY(hipHostMalloc((void **)&c->h_bank[b], kBankWords * 8, hipHostMallocDefault));
    }
    HIP_TRY(hipMalloc((void **)&c->d_sums, 2 * kMaxDev * sizeof(unsigned long long)));
    HIP_TRY(hipHostMalloc((void **)&c->h_sums, 2 * kMaxDev * 8, hipHostMallocDefault));
    return SHUD_OK;
}

static int ckpt_slab(shud_ckpt *c, uint64_t words) {
    if (words <= c->slab_cap) return SHUD_OK;
    if (c->d_slab) HIP_TRY(hipFree(c->d_slab));
    c->d_slab = nullptr;
    c->slab_cap = 0;
    HIP_TRY(hipMalloc((void **)&c->d_slab, words * 8));
    HIP_TRY(hipMemsetAsync(c->d_slab, 0, words * 8, c->stream));      // the phase-padding words between buffers
    c->slab_cap = words;
    return SHUD_OK;
}

extern "C" int shud_ckpt_snapshot(shud_ckpt_t c, const ShudCkptParts *p, double t, int64_t step, const char *path) {
    if (!c || !path) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (ckpt_drain(c)) return ckpt_report(c);               // a second snapshot waits for the first one's drain
    HIP_TRY(hipSetDevice(c->device));
    Job &j = c->job;
    j = Job{};
    j.path = path;
    ShudCkptInfo &hdr = j.hdr;
    memcpy(hdr.magic, SHUD_CKPT_MAGIC, 8);
    hdr.version = SHUD_CKPT_VERSION;
    hdr.abi_version = (uint32_t)shud_rhs_abi_version();
    hdr.t = t;
    hdr.step = step;
    int rc = check_parts(p, &hdr, false);
    if (rc) return rc;
    CkptPart part;
    if ((rc = collect_dev(p, part, nullptr))) return rc;
    if (p->rhs) {
        // every snapshot: one checksum-only pass (a cache keyed on the handle's address could outlive the handle)
        uint64_t fp[2];
        if ((rc = statics_fingerprint(p->rhs, c->d_sums, c->stream, fp))) return rc;
        hdr.statics_c0 = fp[0];
        hdr.statics_c1 = fp[1];
    }
    const Layout L = lay_out(part.dev, 0);
    if ((rc = ckpt_slab(c, L.words))) return rc;
    // the one batched pass, then the 4-byte tails of buffers that are no whole number of words
    if ((rc = pack_launch(part.dev, &L.off, c->d_slab, c->d_sums, c->stream))) return rc;
    HIP_TRY(hipEventRecord(c->ev_pack, c->stream));
    // an object on another stream than the pack's must not overwrite a buffer the pass still reads
    {
        hipStream_t os[3] = {p->rhs ? p->rhs->stream : c->stream, (hipStream_t)shud_ode_ckpt_stream(p->ode),
                             p->out ? (hipStream_t)shud_out_ckpt_stream(p->out) : c->stream};
        for (hipStream_t s : os)
            if (s != c->stream) HIP_TRY(hipStreamWaitEvent(s, c->ev_pack, 0));
    }
    CkptAr tails;
    for (const auto &d : part.dev)
        if (d.bytes % 8) {
            uint64_t w = 0;
            HIP_TRY(hipMemcpy(&w, (const char *)d.p + d.bytes / 8 * 8, d.bytes % 8, hipMemcpyDeviceToHost));
            tails.pod(w);
        }
    // the host scalars
    std::vector<HostSec> hs;
    if (p->rhs) {
        CkptAr a;
        if ((rc = rhs_host(p->rhs, a, false))) return rc;
        hs.push_back(host_sec("rhs.host", a.buf));
        if (p->rhs->et) {
            CkptAr e, q;
            if ((rc = shud_et_ckpt_host(p->rhs, e, false)) || (rc = shud_et_ckpt_queues(p->rhs, q))) return rc;
            hs.push_back(host_sec("et.host", e.buf));
            hs.push_back(host_sec("et.queues.host", q.buf));
        }
    }
    {
        CkptAr a;
        if ((rc = shud_ode_ckpt_host(p->ode, a))) return rc;
        hs.push_back(host_sec("ode.host", a.buf));
    }
    if (p->out) {
        CkptAr a;
        if ((rc = shud_out_ckpt_host(p->out, a, false))) return rc;
        hs.push_back(host_sec("out.host", a.buf));
    }
    if (p->mon) {
        CkptAr a;
        if ((rc = shud_mon_ckpt_host(p->mon, a, false))) return rc;
        hs.push_back(host_sec("mon.host", a.buf));
    }
    hs.push_back(host_sec("dev.tails", tails.buf));
    uint64_t at = 0;
    for (const auto &s : hs) {
        ShudCkptSection e{};
        strncpy(e.name, s.name.c_str(), SHUD_CKPT_NAME_LEN - 1);
        e.offset = at;
        e.words = s.words.size();
        shud_ckpt_checksum(s.words.data(), s.words.size(), &e.c0, &e.c1);
        j.table.push_back(e);
        j.host.insert(j.host.end(), s.words.begin(), s.words.end());
        at += s.words.size();
    }
    j.n_host = hs.size();
    j.n_dev = part.dev.size();
    for (size_t k = 0; k < part.dev.size(); k++) {
        ShudCkptSection e{};
        memcpy(e.name, part.dev[k].name, SHUD_CKPT_NAME_LEN);
        e.offset = at + L.off[k];
        e.words = part.dev[k].bytes / 8;
        j.table.push_back(e);                               // c0 / c1: the kernel's sums, filled in by the writer
    }
    j.slab_words = L.words;
    hdr.n_sections = (uint32_t)j.table.size();
    hdr.header_bytes = (uint32_t)(sizeof(ShudCkptInfo) + j.table.size() * sizeof(ShudCkptSection));
    hdr.payload_words = at + L.words;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        c->busy = true;
    }
    c->cv.notify_all();
    return SHUD_OK;
}

extern "C" int shud_ckpt_flush(shud_ckpt_t c) {
    if (!c) return shud_fail(SHUD_ERR_ARG, "null argument");
    ckpt_drain(c);
    return ckpt_report(c);
}

extern "C" int shud_ckpt_destroy(shud_ckpt_t c) {
    if (!c) return SHUD_OK;
    (void)hipSetDevice(c->device);
    ckpt_drain(c);
    const int rc = ckpt_report(c);
    {
        std::lock_guard<std::mutex> lk(c->mu);
        c->stop = true;
    }
    c->cv.notify_all();
    if (c->writer.joinable()) c->writer.join();
    if (c->s_copy) (void)hipStreamSynchronize(c->s_copy);
    if (c->d_slab) (void)hipFree(c->d_slab);
    if (c->d_sums) (void)hipFree(c->d_sums);
    if (c->h_sums) (void)hipHostFree(c->h_sums);
    for (int b = 0; b < 2; b++) {
        if (c->h_bank[b]) (void)hipHostFree(c->h_bank[b]);
        if (c->ev_bank[b]) (void)hipEventDestroy(c->ev_bank[b]);
    }
    if (c->ev_pack) (void)hipEventDestroy(c->ev_pack);
    if (c->s_copy) (void)hipStreamDestroy(c->s_copy);
    delete c;
    return rc;
}

extern "C" int shud_ckpt_restore(const char *path, const ShudCkptParts *p, double *t, int64_t *step) {
    if (!path || !p) return shud_fail(SHUD_ERR_ARG, "null argument");
    CkptFile f;
    int rc = shud_ckpt_fmt_read(path, true, &f);            // every section's checksum
    if (rc) return rc;
    if (f.hdr.abi_version != (uint32_t)shud_rhs_abi_version())
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: field abi_version differs (file %u, library %d)",
                         f.hdr.abi_version, shud_rhs_abi_version());
    if ((rc = check_parts(p, &f.hdr, true))) return rc;
    CkptPart part;
    if ((rc = collect_dev(p, part, &f))) return rc;
    // every buffer has its section, of its size, and the file holds no buffer the objects lack
    size_t n_dev_file = 0;
    for (const auto &s : f.table) {
        const std::string nm(s.name, strnlen(s.name, SHUD_CKPT_NAME_LEN));
        if (!(nm.size() > 5 && nm.compare(nm.size() - 5, 5, ".host") == 0) && nm != "dev.tails") n_dev_file++;
    }
    std::vector<const ShudCkptSection *> sec;
    for (const auto &d : part.dev) {
        const ShudCkptSection *s = f.find(d.name);
        if (!s) return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: the file has no section %s", d.name);
        if (s->words != d.bytes / 8)
            return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: section %s has %llu words, the object's buffer %zu", d.name,
                             (unsigned long long)s->words, d.bytes / 8);
        sec.push_back(s);
    }
    if (n_dev_file != part.dev.size())
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: the file holds %zu device sections, the objects have %zu buffers",
                         n_dev_file, part.dev.size());
    unsigned long long *d_sums = nullptr;
    HIP_TRY(hipMalloc((void **)&d_sums, 2 * kMaxDev * sizeof(unsigned long long)));
    struct Free { void *p; ~Free() { (void)hipFree(p); } } fr{d_sums};
    if (p->rhs) {
        uint64_t fp[2];
        if ((rc = statics_fingerprint(p->rhs, d_sums, nullptr, fp))) return rc;
        if (fp[0] != f.hdr.statics_c0 || fp[1] != f.hdr.statics_c1)
            return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: field statics fingerprint differs (the handle was built "
                                           "from another mesh, calibration or layout)");
        if ((rc = rhs_check_counts(p->rhs, &f.hdr))) return rc;
    }
    // the host sections parse and their settings match (nothing is assigned yet)
    auto archive = [&](const char *name, CkptAr &a) -> int {
        const ShudCkptSection *s = f.find(name);
        if (!s) return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: the file has no section %s", name);
        a.load = true;
        a.buf.resize(s->words * 8);
        if (s->words) memcpy(a.buf.data(), f.payload.data() + s->offset, s->words * 8);
        return SHUD_OK;
    };
    for (int pass = 0; pass < 2; pass++) {
        const bool chk = pass == 0;
        if (!chk) {
            // upload, then the kernel's checksum-only mode over what landed
            CkptAr tails;
            if ((rc = archive("dev.tails", tails))) return rc;
            if (p->rhs && (rc = rhs_alloc_sums(p->rhs, part))) return rc;
            for (size_t k = 0; k < part.dev.size(); k++) {
                const CkptDev &d = part.dev[k];
                if (sec[k]->words)
                    HIP_TRY(hipMemcpyAsync(d.p, f.payload.data() + sec[k]->offset, sec[k]->words * 8, hipMemcpyHostToDevice,
                                           nullptr));
                if (d.bytes % 8) {
                    uint64_t w = 0;
                    tails.pod(w);
                    HIP_TRY(hipMemcpyAsync((char *)d.p + d.bytes / 8 * 8, &w, d.bytes % 8, hipMemcpyHostToDevice, nullptr));
                    HIP_TRY(hipStreamSynchronize(nullptr));
                }
            }
            HIP_TRY(hipDeviceSynchronize());
            if ((rc = pack_launch(part.dev, nullptr, nullptr, d_sums, nullptr))) return rc;
            std::vector<uint64_t> sums(2 * part.dev.size());
            HIP_TRY(hipMemcpy(sums.data(), d_sums, sums.size() * 8, hipMemcpyDeviceToHost));
            HIP_TRY(hipDeviceSynchronize());
            for (size_t k = 0; k < part.dev.size(); k++)
                if (sums[2 * k] != sec[k]->c0 || sums[2 * k + 1] != sec[k]->c1)
                    return shud_fail(SHUD_ERR_HIP, "shud_ckpt_restore: section %s: the uploaded buffer's checksum differs",
                                     part.dev[k].name);
        }
        if (p->rhs) {
            CkptAr a;
            if ((rc = archive("rhs.host", a)) || (rc = rhs_host(p->rhs, a, chk))) return rc;
            if (p->rhs->et) {
                CkptAr e, q;
                if ((rc = archive("et.host", e)) || (rc = shud_et_ckpt_host(p->rhs, e, chk))) return rc;
                if ((rc = archive("et.queues.host", q)) || (!chk && (rc = shud_et_ckpt_queues(p->rhs, q)))) return rc;
            }
        }
        if (p->out) {
            CkptAr a;
            if ((rc = archive("out.host", a)) || (rc = shud_out_ckpt_host(p->out, a, chk))) return rc;
        }
        if (p->mon) {
            CkptAr a;
            if ((rc = archive("mon.host", a)) || (rc = shud_mon_ckpt_host(p->mon, a, chk))) return rc;
        }
        CkptAr a;
        if ((rc = archive("ode.host", a))) return rc;
        if (!chk && (rc = shud_ode_ckpt_host(p->ode, a))) return rc;
    }
    if (t) *t = f.hdr.t;
    if (step) *step = f.hdr.step;
    return SHUD_OK;
}

// ---------------------------------------------------------------------------------------------
// test / measurement entries
// ---------------------------------------------------------------------------------------------
extern "C" int shud_ckpt_pack_test(int32_t nseg, const uint64_t *src, const int64_t *words, const int32_t *misalign,
                                   int32_t guard, uint64_t fill, int32_t verify, uint64_t *slab, int64_t slab_cap,
                                   int64_t *slab_words, int64_t *dst_off, uint64_t *c0, uint64_t *c1) {
    if (nseg < 1 || nseg > kMaxSeg || !src || !words || !misalign || guard < 0 || !slab || !slab_words || !dst_off ||
        !c0 || !c1)
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt_pack_test: bad argument");
    // sources: each 16-byte aligned plus its misalignment, one spare pair between them
    std::vector<uint64_t> at((size_t)nseg);
    uint64_t n_src = 0;
    for (int k = 0; k < nseg; k++) {
        if (words[k] < 0 || (misalign[k] != 0 && misalign[k] != 1)) return shud_fail(SHUD_ERR_ARG, "shud_ckpt_pack_test: segment %d", k);
        n_src = (n_src + 1) / 2 * 2 + (uint64_t)misalign[k];
        at[k] = n_src;
        n_src += (uint64_t)words[k] + 2;
    }
    uint64_t *d_src = nullptr, *d_slab = nullptr;
    unsigned long long *d_sums = nullptr;
    struct Free {
        uint64_t **a, **b;
        unsigned long long **c;
        ~Free() { (void)hipFree(*a); (void)hipFree(*b); (void)hipFree(*c); }
    } fr{&d_src, &d_slab, &d_sums};
    HIP_TRY(hipMalloc((void **)&d_src, n_src * 8));
    std::vector<uint64_t> h_src(n_src, 0);
    std::vector<CkptDev> dev((size_t)nseg);
    uint64_t in = 0;
    for (int k = 0; k < nseg; k++) {
        if (words[k]) memcpy(h_src.data() + at[k], src + in, (size_t)words[k] * 8);
        in += (uint64_t)words[k];
        dev[k] = CkptDev{};
        snprintf(dev[k].name, sizeof(dev[k].name), "seg%d", k);
        dev[k].p = d_src + at[k];
        dev[k].bytes = (size_t)words[k] * 8;
    }
    HIP_TRY(hipMemcpy(d_src, h_src.data(), n_src * 8, hipMemcpyHostToDevice));
    const Layout L = lay_out(dev, (uint64_t)guard);
    *slab_words = (int64_t)L.words;
    for (int k = 0; k < nseg; k++) dst_off[k] = (int64_t)L.off[k];
    if ((int64_t)L.words > slab_cap) return shud_fail(SHUD_ERR_ARG, "shud_ckpt_pack_test: the slab needs %llu words", (unsigned long long)L.words);
    std::vector<uint64_t> h_slab(std::max<uint64_t>(L.words, 1), fill);
    HIP_TRY(hipMalloc((void **)&d_slab, h_slab.size() * 8));
    HIP_TRY(hipMemcpy(d_slab, h_slab.data(), h_slab.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc((void **)&d_sums, 2 * kMaxSeg * sizeof(unsigned long long)));
    HIP_TRY(hipDeviceSynchronize());
    int rc = pack_launch(dev, verify ? nullptr : &L.off, verify ? nullptr : d_slab, d_sums, nullptr);
    if (rc) return rc;
    std::vector<uint64_t> sums(2 * (size_t)nseg);
    HIP_TRY(hipMemcpy(sums.data(), d_sums, sums.size() * 8, hipMemcpyDeviceToHost));
    if (L.words) HIP_TRY(hipMemcpy(slab, d_slab, L.words * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    for (int k = 0; k < nseg; k++) {
        c0[k] = sums[2 * k];
        c1[k] = sums[2 * k + 1];
    }
    return SHUD_OK;
}

extern "C" int shud_ckpt_time_pack(shud_ckpt_t c, const ShudCkptParts *p, int reps, double *ms_pass, int64_t *bytes) {
    if (!c || !p || reps < 1 || !ms_pass) return shud_fail(SHUD_ERR_ARG, "bad argument");
    if (ckpt_drain(c)) return ckpt_report(c);
    HIP_TRY(hipSetDevice(c->device));
    ShudCkptInfo hdr{};
    int rc = check_parts(p, &hdr, false);
    if (rc) return rc;
    CkptPart part;
    if ((rc = collect_dev(p, part, nullptr))) return rc;
    const Layout L = lay_out(part.dev, 0);
    if ((rc = ckpt_slab(c, L.words))) return rc;
    if (bytes) {
        *bytes = 0;
        for (const auto &d : part.dev) *bytes += (int64_t)(d.bytes / 8 * 8);
    }
    return shud::time_passes(c->stream, reps, [&]() -> int {
        return pack_launch(part.dev, &L.off, c->d_slab, c->d_sums, c->stream);
    }, ms_pass);
}
