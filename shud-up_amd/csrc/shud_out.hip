// shud_out.hip — output path on the device (include/shud_out.h).
//
// The reference keeps one host buffer per Print_Ctrl and, at every solver step, adds each selected
// Model_Data value into it (Print_Ctrl::PrintData, src/classes/Model_Control.cpp:926-960); the mean over the
// interval goes to a binary .dat (fun_printBINARY :893-899) and/or ASCII .csv (:900-909) file.  Here the values
// already live in HBM, so the buffers do too: every export adds all registered variables with ONE batched
// kernel (blockIdx.y = control; a control's selected columns are a device index list when flag_IO masks some),
// and only the controls whose interval ends scale their buffer on the device (buffer *= tau / NumUpdate, the
// reference's expression) and come back over PCIe to be written with the reference's byte layout.
//
// Finished intervals leave the compute stream at once: one kernel per control writes the scaled mean into a
// snapshot buffer and zeroes the accumulator; the snapshot goes device->host on a copy stream into one of two
// pinned banks, and writer threads (controls dealt round-robin, so each file keeps one writer and its row order)
// append the rows once that copy's event has fired.  The time loop only waits when both banks are still being
// written (the reference writes synchronously inside ExportResults; the bytes written are the same, in the
// same order).
//
// NetCDF sinks (OUTPUT_MODE NETCDF / BOTH, include/shud_nc.h): a control registered with shud_out_add_nc keeps, beside
// its accumulator, the on-disk record slab of its variable on the device: n_all big-endian float words, fill at every
// unselected position (written once at registration).  At the interval's end one kernel forms k_snap's product, stores
// its float (round-to-nearest-even, bytes swapped) at the selected positions of the slab, the double into the
// snapshot when a .dat / .csv is written too, and zeroes the accumulator.  The slab crosses PCIe at 4 bytes per
// value into pinned banks of its own and the control's writer thread places it with one positioned write; the record
// index is fixed by the exporting thread (control order, as the reference's ensureTimeIndex sees it).
#include <hip/hip_runtime.h>

#include <sys/stat.h>
#include <unistd.h>

#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "shud_ckpt_parts.h"
#include "shud_diag_host.h"
#include "shud_handle.h"
#include "shud_nc.h"
#include "shud_out.h"
#include "shud_reduce.h"
#include "shud_zone.h"

namespace {

struct PrintSlot {                       // one Print_Ctrl on the device (POD, copied to a device table)
    const double *src;
    const int *sel;                      // selected column -> source index; nullptr = identity
    double *buf;
    int nvar;
};

__global__ void __launch_bounds__(256) k_accumulate(const PrintSlot *__restrict__ slots) {
    const PrintSlot s = slots[blockIdx.y];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < s.nvar; i += gridDim.x * blockDim.x)
        s.buf[i] += s.src[s.sel ? s.sel[i] : i];                 // buffer[i] += *(PrintVar[i])
}

// buffer[i] *= tau / NumUpdate (the reference's expression, into the snapshot), then buffer[i] = 0
__global__ void __launch_bounds__(256) k_snap(double *__restrict__ buf, double *__restrict__ snap, int n, double f) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        snap[i] = buf[i] * f;
        buf[i] = 0.0;
    }
}

// ---- zonal controls (shud_out_add_zonal): the source reduced to one value per zone before it is accumulated ----------
// Plan (shud_zone.cpp): the members of every zone are contiguous in `member` (source indices) with their weights beside
// them in the same order, cut into chunks of 1024; a zone's partials are contiguous in `part`.  Two launches per export
// for every zonal control of the set (blockIdx.y = control), in shud_reduce.h's order and without atomics.
struct ZoneSlot {                        // one zonal control on the device (POD, copied to a device table)
    const double *src;
    const int *member;                   // [n_member]
    const double *weight;                // [n_member] in member order; nullptr = unweighted
    const int *chunk_zone, *chunk_first; // [n_chunk]
    const int *zone_off, *zone_chunk;    // [nz + 1] member / chunk offsets of zone z (0-based)
    const int *multi;                    // [n_multi] zones of more than one chunk
    double *part;                        // [n_chunk]
    double *buf;                         // [nz]
    int n_chunk, nz, n_multi;
};

// one block per chunk: lane l holds weight * x of member chunk_first + l (one multiplication; the build has no
// contraction), 0.0 past the zone's end; block_partial stores part[chunk]
__global__ void __launch_bounds__(shud::red::kRedThreads) k_zone_partial(const ZoneSlot *__restrict__ slots) {
    const ZoneSlot s = slots[blockIdx.y];
    const int b = blockIdx.x;
    if (b >= s.n_chunk) return;                                  // the whole block: the grid is the set's widest control
    const int first = s.chunk_first[b];
    const int end = min(first + shud::kZoneChunk, s.zone_off[s.chunk_zone[b] + 1]);
    const int i = first + (int)threadIdx.x;
    double v[1] = {0.0};
    if (i < end) {
        const double x = s.src[s.member[i]];
        v[0] = s.weight ? s.weight[i] * x : x;
    }
    shud::red::block_partial<1>(v, 0u, s.part, s.n_chunk);
}

// buf_z += S_z.  Blocks 0 .. n_multi-1: ordered_total over the partials of one zone of several chunks.  The blocks after
// them take 1024 zones each, a thread per zone of at most one chunk: ordered_total over one partial p is 0.0 + p (acc[0]
// of lane 0 starts from the identity, so a -0.0 partial gives +0.0; every later addend is +0.0), and over none +0.0.
__global__ void __launch_bounds__(shud::red::kFinThreads) k_zone_final(const ZoneSlot *__restrict__ slots) {
    __shared__ double sm[shud::red::kFinThreads / 64];
    const ZoneSlot s = slots[blockIdx.y];
    const int b = blockIdx.x;
    if (b < s.n_multi) {
        const int z = s.multi[b];
        const int c0 = s.zone_chunk[z];
        const double t = shud::red::ordered_total(s.part + c0, s.zone_chunk[z + 1] - c0, false, sm);
        if (threadIdx.x == 0) s.buf[z] += t;
        return;
    }
    const int z = (b - s.n_multi) * shud::red::kFinThreads + (int)threadIdx.x;
    if (z >= s.nz) return;
    const int c0 = s.zone_chunk[z], nc = s.zone_chunk[z + 1] - c0;
    if (nc > 1) return;
    const double t = nc ? 0.0 + s.part[c0] : 0.0;
    s.buf[z] += t;
}

// the interval's end of a SHUD_ZONE_WMEAN control: k_snap's product, divided by W_z
__global__ void __launch_bounds__(256) k_snap_wmean(double *__restrict__ buf, double *__restrict__ snap,
                                                    const double *__restrict__ wsum, int n, double f) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        snap[i] = (buf[i] * f) / wsum[i];
        buf[i] = 0.0;
    }
}

// The interval's end of a control with a NetCDF sink.  mean = buf[j] * f is k_snap's product; slab position p holds the
// big-endian bits of (float)mean of its column j (out[idx0] = (float)buffer[j], NetcdfOutputContext.cpp:1000), or the
// fill; snap (BOTH mode; else nullptr) receives the same double; buf is zeroed once.  A lane owns four consecutive slab
// positions and writes them with one 16-byte store (slab, buf, snap and col are allocated in whole quads, so there is
// no tail); the slab and the snapshot are single-use streams on their way to the host: non-temporal stores where a
// lane writes 16 bytes.
__device__ __forceinline__ uint32_t be_float(double m) { return __builtin_bswap32(__float_as_uint((float)m)); }

// every column selected: position p is column p
__global__ void __launch_bounds__(256) k_snap_nc(double *__restrict__ buf, double *__restrict__ snap,
                                                 uint32_t *__restrict__ slab, int nquad, double f) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nquad) return;
    typedef double v2d __attribute__((ext_vector_type(2)));
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    v2d *b = (v2d *)buf + 2 * (size_t)q;
    const v2d a0 = b[0], a1 = b[1];
    const v2d m0 = a0 * f, m1 = a1 * f;
    b[0] = (v2d){0.0, 0.0};
    b[1] = (v2d){0.0, 0.0};
    if (snap) {
        shud::red::stn((v2d *)snap + 2 * (size_t)q, m0);
        shud::red::stn((v2d *)snap + 2 * (size_t)q + 1, m1);
    }
    shud::red::stn((v4u *)slab + q, (v4u){be_float(m0.x), be_float(m0.y), be_float(m1.x), be_float(m1.y)});
}

// a column selection: col[p] is the selected column at position p, -1 where the slab keeps its fill
__global__ void __launch_bounds__(256) k_snap_nc_sel(double *__restrict__ buf, double *__restrict__ snap,
                                                     uint32_t *__restrict__ slab, const int *__restrict__ col,
                                                     int nquad, double f) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nquad) return;
    typedef int v4i __attribute__((ext_vector_type(4)));
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const v4i j4 = ((const v4i *)col)[q];
    const int j[4] = {j4.x, j4.y, j4.z, j4.w};
    uint32_t w[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        w[u] = __builtin_bswap32(SHUD_NC_FILL_BITS);
        if (j[u] >= 0) {
            const double m = buf[j[u]] * f;
            buf[j[u]] = 0.0;
            if (snap) snap[j[u]] = m;                            // 8-byte pieces: plain stores, merged in L2
            w[u] = be_float(m);
        }
    }
    shud::red::stn((v4u *)slab + q, (v4u){w[0], w[1], w[2], w[3]});
}

// Model_Data::summary (MD_update.cpp:190-216): element storages and river stage from a state vector, BC
// values where the element / reach has a head boundary condition.  summary(N_Vector) leaves yLakeStg alone: the
// reference sets it in LoadIC and then in f_update only (MD_update.cpp:175), so ylake is given (non-null) only
// before the handle's first evaluation, when the vector is the initial condition; afterwards
// shud_rhs_refresh_diagnostics takes the lake entries of the last RHS input.
__global__ void __launch_bounds__(256) k_summary(DevMesh m, const double *__restrict__ y, int ne, int nr, int nl,
                                                 double *ysf, double *yus, double *ygw, double *yriv, double *ylake) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ne) {
        ysf[i] = y[i];
        yus[i] = y[ne + i];
        const int ibc = (int)(int16_t)(m.eflags[i] & 0xffff);
        ygw[i] = ibc > 0 ? m.eybc[ibc] : y[2 * ne + i];
    }
    if (i < nr) {
        const int bc = m.riv_bc[i];
        yriv[i] = bc > 0 ? m.rybc[bc] : y[3 * ne + i];
    }
    if (ylake && i < nl) ylake[i] = y[3 * ne + nr + i];
}

// qEleTrans = Tg + Tu, qEleEvapo = Eu + Eg + Es (MD_ET.cpp:388-389), from the replayed diagnostics; a lake
// element has qEleTrans = 0 and qEleEvapo = qPotEvap (fun_Ele_lakeVertical, MD_ElementFlux.cpp:14-15).
// lake_of: [ne] lake of a lake element, -1 otherwise; null for a model without lakes
__global__ void __launch_bounds__(256) k_et_sums(DevDiag d, int ne, const int *__restrict__ lake_of,
                                                 const double *__restrict__ pot_evap, double *trans, double *evapo) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ne) return;
    const bool lake = lake_of && lake_of[i] >= 0;
    trans[i] = lake ? 0. : d.q_tg[i] + d.q_tu[i];
    evapo[i] = lake ? pot_evap[i] : d.q_eu[i] + d.q_eg[i] + d.q_es[i];
}

}  // namespace

struct PrintCtrl {
    std::string filename;
    long long start_time = 0;
    int interval = 0, numvar = 0, numall = 0, num_update = 0;
    double tau = 1.0;
    std::vector<double> icol;
    int *d_sel = nullptr;
    double *d_buf = nullptr;
    double *d_snap = nullptr;            // the finished interval's mean, on its way to the host
    double *h_buf[2] = {nullptr, nullptr};   // pinned banks for the interval mean
    FILE *fb = nullptr, *fa = nullptr;
    int64_t rows = 0;
    // NetCDF sink (shud_out_add_nc): file kind (-1: none), the control's id in that file, the record slab on the
    // device (whole quads), its pinned banks, and the position -> column list when a selection masks some columns
    int nc_kind = -1, nc_ctrl = -1;
    bool legacy = true;                  // a .dat / .csv is written too: the double snapshot is formed and copied
    uint32_t *d_slab = nullptr, *h_slab[2] = {nullptr, nullptr};
    int *d_col = nullptr;
    // zonal control (shud_out_add_zonal): the operation (-1: a plain control), the plan's integer tables (one
    // allocation), the weights in member order, the chunk partials and W_z (WMEAN)
    int zone_op = -1;
    int *d_zint = nullptr;
    double *d_zweight = nullptr, *d_zpart = nullptr, *d_zwsum = nullptr;
};

struct OutTask {                         // one row of one control: (bank, control, left endpoint of the interval)
    int bank, ctrl;
    double tq;
    int64_t rec;                         // NetCDF record of tq (fixed at export, in control order)
};
constexpr int kWriters = 4;

struct shud_out {
    int device = 0;
    hipStream_t stream = nullptr;        // compute stream (accumulate / snapshot kernels)
    hipStream_t s_copy = nullptr;        // device->host copies of the snapshots
    hipEvent_t ev_snap = nullptr, ev_copied[2] = {nullptr, nullptr};
    bool copy_pending = false;           // a snapshot copy is in flight (the next snapshot waits for it)
    int bank = 0;
    std::vector<PrintCtrl> pc;
    std::vector<PrintSlot> slots;        // host mirror of d_slots: the plain controls, in registration order
    PrintSlot *d_slots = nullptr;
    int n_slots_alloc = 0;
    int max_nvar = 0;
    std::vector<ZoneSlot> zslots;        // host mirror of d_zslots: the zonal controls, in registration order
    ZoneSlot *d_zslots = nullptr;
    int n_zslots_alloc = 0;
    int max_zchunk = 0, max_zfin = 0;    // grid widths of k_zone_partial / k_zone_final
    int64_t n_launch[SHUD_OUT_KERNELS] = {};   // launches enqueued so far, per kernel (shud_out_launches)
    // writer threads: writer w owns the controls k with k % kWriters == w
    std::thread writer[kWriters];
    std::mutex mu;
    std::condition_variable cv;
    std::deque<OutTask> tasks[kWriters];
    int bank_left[2] = {0, 0};           // rows of the bank's event not yet written
    bool stop = false;
    // first writer-side failure (the snapshot copy's event or a file write): reported by shud_out_flush /
    // shud_out_rows / shud_out_destroy; rows whose copy failed are never written (no stale bank reaches a file)
    int werr = 0;
    std::string werr_msg;
    shud_nc_t nc[SHUD_NC_KINDS] = {nullptr, nullptr, nullptr};   // attached NetCDF files
    bool nc_begun = false;
    bool resume = false;                 // shud_out_resume: controls added from now on keep their files
};
static void writer_fail(shud_out *o, int code, const std::string &msg) {
    std::lock_guard<std::mutex> lk(o->mu);
    if (!o->werr) { o->werr = code; o->werr_msg = msg; }
}

static void writer_loop(shud_out *o, int w) {
    (void)hipSetDevice(o->device);
    for (;;) {
        OutTask job;
        {
            std::unique_lock<std::mutex> lk(o->mu);
            o->cv.wait(lk, [&] { return o->stop || !o->tasks[w].empty(); });
            if (o->tasks[w].empty()) return;
            job = o->tasks[w].front();
            o->tasks[w].pop_front();
        }
        const hipError_t he = hipEventSynchronize(o->ev_copied[job.bank]);
        PrintCtrl &p = o->pc[job.ctrl];
        const double *hb = p.h_buf[job.bank];
        if (he != hipSuccess) {
            writer_fail(o, SHUD_ERR_HIP, std::string("output snapshot copy failed (") + hipGetErrorString(he) +
                                             "): row of " + p.filename + " not written");
        } else {
            if (p.fa) {                                              // fun_printASCII
                fprintf(p.fa, "%.1f\t", job.tq);
                for (int i = 0; i < p.numvar; i++) fprintf(p.fa, "%e\t", hb[i]);
                fprintf(p.fa, "\n");
                if (ferror(p.fa)) writer_fail(o, SHUD_ERR_ARG, "write error on " + p.filename + ".csv");
            }
            if (p.fb) {                                              // fun_printBINARY
                const size_t w1 = fwrite(&job.tq, sizeof(double), 1, p.fb);
                const size_t w2 = fwrite(hb, sizeof(double), p.numvar, p.fb);
                if (w1 != 1 || w2 != (size_t)p.numvar) writer_fail(o, SHUD_ERR_ARG, "write error on " + p.filename + ".dat");
            }
            if (p.nc_ctrl >= 0) {                                    // Netcdf*VarSink::onWrite
                shud_nc_t nc = o->nc[p.nc_kind];
                int64_t rec = job.rec;
                if (shud_nc_record(nc, job.tq, &rec) || shud_nc_put_slab(nc, p.nc_ctrl, rec, p.h_slab[job.bank]))
                    writer_fail(o, SHUD_ERR_ARG, shud_nc_last_error());
            }
        }
        {
            std::lock_guard<std::mutex> lk(o->mu);
            o->bank_left[job.bank]--;
        }
        o->cv.notify_all();
    }
}

// wait until every queued row is in the files (flushed to the C library); returns the first writer failure
static int out_drain(shud_out *o) {
    std::unique_lock<std::mutex> lk(o->mu);
    o->cv.wait(lk, [&] { return o->bank_left[0] == 0 && o->bank_left[1] == 0; });
    for (PrintCtrl &p : o->pc) {
        if (p.fb && fflush(p.fb) != 0 && !o->werr) { o->werr = SHUD_ERR_ARG; o->werr_msg = "flush error on " + p.filename + ".dat"; }
        if (p.fa && fflush(p.fa) != 0 && !o->werr) { o->werr = SHUD_ERR_ARG; o->werr_msg = "flush error on " + p.filename + ".csv"; }
    }
    return o->werr;
}
static int out_report(shud_out *o) {
    return o->werr ? shud_fail(o->werr, "shud_out: %s", o->werr_msg.c_str()) : SHUD_OK;
}

static int out_fail_io(const char *what, const std::string &f) {
    return shud_fail(SHUD_ERR_ARG, "%s: cannot open %s", what, f.c_str());
}

extern "C" int shud_out_create(int device, void *stream, shud_out_t *out) {
    if (!out) return shud_fail(SHUD_ERR_ARG, "null argument");
    *out = nullptr;
    HIP_TRY(hipSetDevice(device));
    shud_out *o = new shud_out;
    o->device = device;
    o->stream = (hipStream_t)stream;
    HIP_TRY(hipStreamCreateWithFlags(&o->s_copy, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&o->ev_snap, hipEventDisableTiming));
    for (int b = 0; b < 2; b++) HIP_TRY(hipEventCreateWithFlags(&o->ev_copied[b], hipEventDisableTiming));
    for (int w = 0; w < kWriters; w++) o->writer[w] = std::thread(writer_loop, o, w);
    *out = o;
    return SHUD_OK;
}

// Print_Ctrl::Init / InitIJ (Model_Control.cpp:759-858) + open_file (:683-758)
// col_src (NULL: identity): caller column c reads d_src[col_src[c]]; flag_io and the header's icol stay by caller column
// nc_kind >= 0: a NetCDF sink in the attached file of that kind; legacy = false: no .dat / .csv beside it
// zp: the plan of a zonal control (op zone_op): NumVar = zp->nz columns 1..nz, no column selection
static int out_add(shud_out_t o, const ShudPrintSpec *s, const int32_t *col_src, int nc_kind = -1, bool legacy = true,
                   const shud::ZonePlan *zp = nullptr, int zone_op = -1) {
    if (!o || !s || !s->basename || !s->d_src) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (nc_kind >= 0 && (nc_kind >= SHUD_NC_KINDS || !o->nc[nc_kind]))
        return shud_fail(SHUD_ERR_ARG, "Print_Ctrl %s: no NetCDF file of kind %d attached (shud_out_attach_nc)",
                         s->basename, nc_kind);
    if (col_src)
        for (int i = 0; i < s->n_all; i++)
            if (col_src[i] < 0 || col_src[i] >= s->n_all)
                return shud_fail(SHUD_ERR_ARG, "Print_Ctrl %s: col_src[%d] = %d outside the source", s->basename, i, col_src[i]);
    if (s->interval == 0) return shud_fail(SHUD_ERR_ARG, "Print_Ctrl %s: interval 0 (reference: myexit(ERRCONSIS))",
                                           s->basename);
    if (s->n_all < 0 || s->interval < 0) return shud_fail(SHUD_ERR_ARG, "bad n_all / interval");
    HIP_TRY(hipSetDevice(o->device));
    if (out_drain(o)) return out_report(o);   // the writer indexes pc: no rows in flight while it grows
    PrintCtrl p;
    p.filename = s->basename;
    p.start_time = (long long)s->start_time;
    p.interval = s->interval;
    p.numall = s->n_all;
    p.tau = s->iflux ? 1440. : 1.;
    std::vector<int> sel;
    for (int i = 0; i < s->n_all && !zp; i++) {
        if (s->flag_io && !s->flag_io[i]) continue;
        sel.push_back(col_src ? col_src[i] : i);
        p.icol.push_back((double)(i + 1));                       // icol[k] = (double)(i + 1)
    }
    for (int k = 0; zp && k < zp->nz; k++) p.icol.push_back((double)(k + 1));
    p.numvar = (int)p.icol.size();
    if (p.numvar <= 0) fprintf(stderr, "WARNING: Empty columns in %s.\n;", p.filename.c_str());
    p.legacy = legacy;
    if (nc_kind >= 0) {                                              // Netcdf*VarSink::onInit
        std::vector<int32_t> icol(p.icol.begin(), p.icol.end());
        int32_t ctrl = -1;
        if (shud_nc_add_var(o->nc[nc_kind], s->basename, s->n_all, s->start_time, icol.data(), p.numvar, &ctrl))
            return shud_fail(SHUD_ERR_ARG, "shud_out_add_nc: %s", shud_nc_last_error());
        p.nc_kind = nc_kind;
        p.nc_ctrl = ctrl;
    }
    const size_t nb = ((size_t)std::max(p.numvar, 1) + 3) / 4 * 4;   // whole quads (k_snap_nc)
    HIP_TRY(hipMalloc(&p.d_buf, nb * sizeof(double)));
    HIP_TRY(hipMemsetAsync(p.d_buf, 0, nb * sizeof(double), o->stream));   // buffer[k] = 0.0
    if (legacy) {
        HIP_TRY(hipMalloc(&p.d_snap, nb * sizeof(double)));
        for (int b = 0; b < 2; b++) HIP_TRY(hipHostMalloc(&p.h_buf[b], nb * sizeof(double), hipHostMallocDefault));
    }
    if (nc_kind >= 0) {
        // the slab as it goes to disk: fill everywhere; the selected positions are rewritten at every interval's end
        const size_t nq = ((size_t)std::max(s->n_all, 1) + 3) / 4 * 4;
        std::vector<uint32_t> fill(nq, __builtin_bswap32(SHUD_NC_FILL_BITS));
        HIP_TRY(hipMalloc(&p.d_slab, nq * sizeof(uint32_t)));
        HIP_TRY(hipMemcpy(p.d_slab, fill.data(), nq * sizeof(uint32_t), hipMemcpyHostToDevice));
        for (int b = 0; b < 2; b++) HIP_TRY(hipHostMalloc(&p.h_slab[b], nq * sizeof(uint32_t), hipHostMallocDefault));
        if (p.numvar < s->n_all) {
            std::vector<int> col(nq, -1);
            for (int k = 0; k < p.numvar; k++) col[(size_t)p.icol[k] - 1] = k;
            HIP_TRY(hipMalloc(&p.d_col, nq * sizeof(int)));
            HIP_TRY(hipMemcpy(p.d_col, col.data(), nq * sizeof(int), hipMemcpyHostToDevice));
        }
    }
    ZoneSlot zs{};
    if (zp) {
        // the plan's integer tables in one allocation, in this order
        const std::vector<int> *tab[6] = {&zp->member, &zp->chunk_zone, &zp->chunk_first, &zp->zone_off, &zp->zone_chunk,
                                          &zp->multi};
        std::vector<int> all;
        size_t at[6];
        for (int k = 0; k < 6; k++) {
            at[k] = all.size();
            all.insert(all.end(), tab[k]->begin(), tab[k]->end());
        }
        const size_t nch = zp->chunk_zone.size();
        HIP_TRY(hipMalloc(&p.d_zint, std::max(all.size(), (size_t)1) * sizeof(int)));
        HIP_TRY(hipMemcpy(p.d_zint, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(hipMalloc(&p.d_zpart, std::max(nch, (size_t)1) * sizeof(double)));
        if (!zp->weight.empty()) {
            HIP_TRY(hipMalloc(&p.d_zweight, zp->weight.size() * sizeof(double)));
            HIP_TRY(hipMemcpy(p.d_zweight, zp->weight.data(), zp->weight.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        if (zone_op == SHUD_ZONE_WMEAN) {
            HIP_TRY(hipMalloc(&p.d_zwsum, zp->wsum.size() * sizeof(double)));
            HIP_TRY(hipMemcpy(p.d_zwsum, zp->wsum.data(), zp->wsum.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        p.zone_op = zone_op;
        zs = ZoneSlot{s->d_src, p.d_zint + at[0], p.d_zweight, p.d_zint + at[1], p.d_zint + at[2], p.d_zint + at[3],
                      p.d_zint + at[4], p.d_zint + at[5], p.d_zpart, p.d_buf, (int)nch, zp->nz, (int)zp->multi.size()};
    } else if (col_src || (s->flag_io && p.numvar < s->n_all)) {
        HIP_TRY(hipMalloc(&p.d_sel, nb * sizeof(int)));
        HIP_TRY(hipMemcpy(p.d_sel, sel.data(), sel.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    // open_file: fixed 1024-byte header, StartTime, NumVar, icol (binary); the ASCII twin's preamble
    const char *mode = s->solar_lonlat_mode ? s->solar_lonlat_mode : "";
    auto dat_preamble = [&](FILE *fp) {
        // a failed write here is not reported; every row's write is checked (writer_loop)
        (void)shud::write_dat_preamble(fp, nullptr, s->radiation_input_mode, s->terrain_radiation, mode,
                                       s->solar_lon_deg, s->solar_lat_deg, (double)p.start_time, p.numvar,
                                       p.icol.data());
    };
    auto csv_preamble = [&](FILE *fp) {
        fprintf(fp, "# Timestamp semantics: left endpoint (t-Interval)\n");
        fprintf(fp, "%d\t %d\t %ld\n", 0, p.numvar, (long)p.start_time);
        fprintf(fp, "# Radiation input mode: %s\n", s->radiation_input_mode == 1 ? "SWNET" : "SWDOWN");
        fprintf(fp, "# Terrain radiation (TSR): %s\n", s->terrain_radiation ? "ON" : "OFF");
        fprintf(fp, "# Solar lon/lat mode: %s\n", mode);
        fprintf(fp, "# Solar lon/lat (deg): lon=%.6f, lat=%.6f\n", s->solar_lon_deg, s->solar_lat_deg);
        fprintf(fp, "%s", "Time_min");
        for (int i = 0; i < p.numvar; i++) fprintf(fp, " \tX%d", i + 1);
        fprintf(fp, "\n");
    };
    // shud_out_resume: the file of an earlier run is kept — opened without truncation, its preamble compared with
    // the one written above, positioned at its end (shud_ckpt_restore cuts it back to the checkpoint's length)
    auto reopen = [&](const std::string &f, auto &preamble, FILE **out) -> int {
        char *want = nullptr;
        size_t nwant = 0;
        FILE *ms = open_memstream(&want, &nwant);
        if (!ms) return out_fail_io("shud_out_add", f);
        preamble(ms);
        fclose(ms);
        FILE *fp = fopen(f.c_str(), "r+b");
        std::vector<char> have(nwant);
        const bool same = fp && fread(have.data(), 1, nwant, fp) == nwant && memcmp(have.data(), want, nwant) == 0;
        free(want);
        if (!fp) return out_fail_io("shud_out_add (resume)", f);
        if (!same || fseek(fp, 0, SEEK_END) != 0) {
            fclose(fp);
            return shud_fail(SHUD_ERR_ARG, "shud_out_add (resume): the header of %s is not the one this control writes",
                             f.c_str());
        }
        *out = fp;
        return SHUD_OK;
    };
    if (legacy && s->binary) {
        const std::string fb = p.filename + ".dat";
        if (o->resume) {
            const int rc = reopen(fb, dat_preamble, &p.fb);
            if (rc) return rc;
        } else {
            p.fb = fopen(fb.c_str(), "wb");
            if (!p.fb) return out_fail_io("shud_out_add", fb);
            dat_preamble(p.fb);
        }
    }
    if (legacy && s->ascii) {
        const std::string fa = p.filename + ".csv";
        if (o->resume) {
            const int rc = reopen(fa, csv_preamble, &p.fa);
            if (rc) return rc;
        } else {
            p.fa = fopen(fa.c_str(), "w");
            if (!p.fa) return out_fail_io("shud_out_add", fa);
            csv_preamble(p.fa);
        }
    }
    o->pc.push_back(p);
    if (zp) {
        o->max_zchunk = std::max(o->max_zchunk, zs.n_chunk);
        o->max_zfin = std::max(o->max_zfin, zs.n_multi + (zs.nz + shud::red::kFinThreads - 1) / shud::red::kFinThreads);
        o->zslots.push_back(zs);
        if ((int)o->zslots.size() > o->n_zslots_alloc) {
            if (o->d_zslots) HIP_TRY(hipFree(o->d_zslots));
            o->n_zslots_alloc = std::max(16, 2 * (int)o->zslots.size());
            HIP_TRY(hipMalloc(&o->d_zslots, o->n_zslots_alloc * sizeof(ZoneSlot)));
        }
        HIP_TRY(hipMemcpyAsync(o->d_zslots, o->zslots.data(), o->zslots.size() * sizeof(ZoneSlot), hipMemcpyHostToDevice,
                               o->stream));
        HIP_TRY(hipStreamSynchronize(o->stream));
        return SHUD_OK;
    }
    o->max_nvar = std::max(o->max_nvar, p.numvar);
    o->slots.push_back(PrintSlot{s->d_src, p.d_sel, p.d_buf, p.numvar});
    // the device slot table (tiny): re-uploaded whole on every add
    if ((int)o->slots.size() > o->n_slots_alloc) {
        if (o->d_slots) HIP_TRY(hipFree(o->d_slots));
        o->n_slots_alloc = std::max(16, 2 * (int)o->slots.size());
        HIP_TRY(hipMalloc(&o->d_slots, o->n_slots_alloc * sizeof(PrintSlot)));
    }
    HIP_TRY(hipMemcpyAsync(o->d_slots, o->slots.data(), o->slots.size() * sizeof(PrintSlot), hipMemcpyHostToDevice,
                           o->stream));
    HIP_TRY(hipStreamSynchronize(o->stream));
    return SHUD_OK;
}

extern "C" int shud_out_add(shud_out_t o, const ShudPrintSpec *s) { return out_add(o, s, nullptr); }
extern "C" int shud_out_add_mapped(shud_out_t o, const ShudPrintSpec *s, const int32_t *col_src) {
    if (!col_src) return shud_fail(SHUD_ERR_ARG, "shud_out_add_mapped: null col_src");
    return out_add(o, s, col_src);
}

extern "C" int shud_out_add_zonal(shud_out_t o, const ShudPrintSpec *s, const int32_t *col_src, const ShudZoneSpec *z) {
    if (!o || !s || !s->basename || !s->d_src || !z) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (s->flag_io)
        return shud_fail(SHUD_ERR_ARG, "Print_Ctrl %s: flag_io is not for a zonal control (zone 0 leaves a column out)",
                         s->basename);
    shud::ZonePlan plan;
    const int rc = shud::zone_plan(s->basename, s->n_all, col_src, z, &plan);
    if (rc) return rc;
    return out_add(o, s, nullptr, -1, true, &plan, z->op);
}

// the per-export pass of the zonal controls: every chunk's partial, then every zone's total into its accumulator
static void launch_zonal(shud_out *o) {
    o->n_launch[SHUD_OUT_K_ZONE_PARTIAL]++;
    o->n_launch[SHUD_OUT_K_ZONE_FINAL]++;
    hipLaunchKernelGGL(k_zone_partial, dim3((unsigned)std::max(o->max_zchunk, 1), (unsigned)o->zslots.size()),
                       dim3(shud::red::kRedThreads), 0, o->stream, o->d_zslots);
    hipLaunchKernelGGL(k_zone_final, dim3((unsigned)std::max(o->max_zfin, 1), (unsigned)o->zslots.size()),
                       dim3(shud::red::kFinThreads), 0, o->stream, o->d_zslots);
}
static void launch_accumulate(shud_out *o) {
    o->n_launch[SHUD_OUT_K_ACCUMULATE]++;
    const int gx = std::min((o->max_nvar + 255) / 256, 2048);
    hipLaunchKernelGGL(k_accumulate, dim3(gx, (unsigned)o->slots.size()), dim3(256), 0, o->stream, o->d_slots);
}

extern "C" int shud_out_time_pass(shud_out_t o, int which, int reps, double *ms_pass) {
    if (!o || !ms_pass || reps < 1 || which < 0 || which > 1) return shud_fail(SHUD_ERR_ARG, "bad argument");
    if (which == 0 ? o->zslots.empty() : (o->slots.empty() || o->max_nvar <= 0))
        return shud_fail(SHUD_ERR_ARG, "shud_out_time_pass: the set has no %s control", which == 0 ? "zonal" : "plain");
    HIP_TRY(hipSetDevice(o->device));
    if (out_drain(o)) return out_report(o);
    return shud::time_passes(o->stream, reps, [&]() -> int {
        if (which == 0) launch_zonal(o); else launch_accumulate(o);
        HIP_TRY(hipGetLastError());
        return SHUD_OK;
    }, ms_pass);
}

// NetCDF sinks: NetcdfOutputContext's three files (NetcdfOutputContext.cpp:1155-1175) and setSink (MD_initialize.cpp:
// 348-356)
extern "C" int shud_out_attach_nc(shud_out_t o, const ShudNcSpec *spec) {
    if (!o || !spec) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (spec->kind < 0 || spec->kind >= SHUD_NC_KINDS) return shud_fail(SHUD_ERR_ARG, "shud_out_attach_nc: unknown kind %d", spec->kind);
    if (o->nc[spec->kind]) return shud_fail(SHUD_ERR_ARG, "shud_out_attach_nc: a file of kind %d is already attached", spec->kind);
    // the output directory must be usable now, not at the first record: OUT_DIR that is a regular file, ...
    if (spec->out_dir && spec->out_dir[0]) {
        struct stat st;
        if (stat(spec->out_dir, &st) == 0 && !S_ISDIR(st.st_mode))
            return shud_fail(SHUD_ERR_ARG, "shud_out_attach_nc: OUT_DIR %s exists and is not a directory", spec->out_dir);
    }
    if (shud_nc_create(spec, &o->nc[spec->kind])) return shud_fail(SHUD_ERR_ARG, "shud_out_attach_nc: %s", shud_nc_last_error());
    return SHUD_OK;
}

extern "C" int shud_out_add_nc(shud_out_t o, const ShudPrintSpec *s, const int32_t *col_src, int32_t kind, int32_t legacy) {
    if (kind < 0) return shud_fail(SHUD_ERR_ARG, "shud_out_add_nc: kind %d", kind);
    if (o && o->nc_begun) return shud_fail(SHUD_ERR_ARG, "shud_out_add_nc: the NetCDF headers are final (a control "
                                           "with a NetCDF sink is registered before the first export)");
    return out_add(o, s, col_src, kind, legacy != 0);
}

// the headers and fixed variables of every attached file that has a control (no later than the first export)
extern "C" int shud_out_nc_begin(shud_out_t o) {
    if (!o) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (o->nc_begun) return SHUD_OK;
    for (int k = 0; k < SHUD_NC_KINDS; k++)
        if (o->nc[k] && shud_nc_num_ctrl(o->nc[k]) > 0 && shud_nc_begin(o->nc[k]))
            return shud_fail(SHUD_ERR_ARG, "shud_out_nc_begin: %s", shud_nc_last_error());
    o->nc_begun = true;
    return SHUD_OK;
}

static void launch_snap_nc(shud_out *o, PrintCtrl &p, double f) {
    const int nquad = (p.numall + 3) / 4;
    o->n_launch[p.d_col ? SHUD_OUT_K_SNAP_NC_SEL : SHUD_OUT_K_SNAP_NC]++;
    if (p.d_col)
        hipLaunchKernelGGL(k_snap_nc_sel, dim3((nquad + 255) / 256), dim3(256), 0, o->stream, p.d_buf, p.d_snap,
                           p.d_slab, p.d_col, nquad, f);
    else
        hipLaunchKernelGGL(k_snap_nc, dim3((nquad + 255) / 256), dim3(256), 0, o->stream, p.d_buf, p.d_snap, p.d_slab,
                           nquad, f);
}

// measurement only: the interval-end kernel of control k, `reps` times back to back (it zeroes the accumulator)
extern "C" int shud_out_time_nc(shud_out_t o, int k, int reps, double *ms_pass) {
    if (!o || !ms_pass || reps < 1 || k < 0 || k >= (int)o->pc.size()) return shud_fail(SHUD_ERR_ARG, "bad argument");
    PrintCtrl &p = o->pc[k];
    if (p.nc_ctrl < 0 || p.numvar <= 0) return shud_fail(SHUD_ERR_ARG, "shud_out_time_nc: control %d has no NetCDF sink", k);
    HIP_TRY(hipSetDevice(o->device));
    if (out_drain(o)) return out_report(o);
    return shud::time_passes(o->stream, reps, [&]() -> int {
        launch_snap_nc(o, p, 1.0);
        HIP_TRY(hipGetLastError());
        return SHUD_OK;
    }, ms_pass);
}

// Control_Data::ExportResults (Model_Control.cpp:123-127) -> Print_Ctrl::PrintData (:926-960) for every control
extern "C" int shud_out_export(shud_out_t o, double t) {
    if (!o) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (o->pc.empty()) return SHUD_OK;
    HIP_TRY(hipSetDevice(o->device));
    if (!o->nc_begun) {
        const int rc = shud_out_nc_begin(o);
        if (rc) return rc;
    }
    if (o->max_nvar > 0) {                                       // the plain controls only
        launch_accumulate(o);
        HIP_TRY(hipGetLastError());
    }
    if (!o->zslots.empty()) {
        launch_zonal(o);
        HIP_TRY(hipGetLastError());
    }
    // OUTPUT_TRIGGER_EPSILON = 0.001 min (:939)
    const long long t_floor = (long long)floor(t + 0.001);
    std::vector<OutTask> rows;
    const int bank = o->bank;
    for (size_t k = 0; k < o->pc.size(); k++) {
        PrintCtrl &p = o->pc[k];
        p.num_update++;
        if (t_floor % p.interval != 0) continue;
        rows.push_back(OutTask{bank, (int)k, (double)(t_floor - (long long)p.interval), -1});   // left endpoint
    }
    if (rows.empty()) return SHUD_OK;
    // a free host bank (the writers may still be writing the one used two events ago)
    {
        std::unique_lock<std::mutex> lk(o->mu);
        o->cv.wait(lk, [&] { return o->bank_left[bank] == 0; });
    }
    // the snapshots are free once the previous copy has finished
    if (o->copy_pending) HIP_TRY(hipStreamWaitEvent(o->stream, o->ev_copied[bank ^ 1], 0));
    for (const auto &r : rows) {
        PrintCtrl &p = o->pc[r.ctrl];
        const double f = p.tau / p.num_update;
        if (p.numvar <= 0) continue;
        if (p.zone_op == SHUD_ZONE_WMEAN) {
            o->n_launch[SHUD_OUT_K_SNAP_WMEAN]++;
            hipLaunchKernelGGL(k_snap_wmean, dim3((p.numvar + 255) / 256), dim3(256), 0, o->stream, p.d_buf, p.d_snap,
                               p.d_zwsum, p.numvar, f);
        } else if (p.nc_ctrl < 0) {
            o->n_launch[SHUD_OUT_K_SNAP]++;
            hipLaunchKernelGGL(k_snap, dim3((p.numvar + 255) / 256), dim3(256), 0, o->stream, p.d_buf, p.d_snap,
                               p.numvar, f);
        } else {
            launch_snap_nc(o, p, f);
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(o->ev_snap, o->stream));
    HIP_TRY(hipStreamWaitEvent(o->s_copy, o->ev_snap, 0));
    for (const auto &r : rows) {
        PrintCtrl &p = o->pc[r.ctrl];
        if (p.numvar > 0 && p.legacy)
            HIP_TRY(hipMemcpyAsync(p.h_buf[bank], p.d_snap, p.numvar * sizeof(double), hipMemcpyDeviceToHost,
                                   o->s_copy));
        if (p.nc_ctrl >= 0 && p.numall > 0)
            HIP_TRY(hipMemcpyAsync(p.h_slab[bank], p.d_slab, (size_t)p.numall * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                   o->s_copy));
    }
    HIP_TRY(hipEventRecord(o->ev_copied[bank], o->s_copy));
    // every launch and copy is enqueued: only now are the rows committed (a failure above returns with the
    // intervals still open and nothing queued for the writers)
    for (auto &r : rows) {
        PrintCtrl &p = o->pc[r.ctrl];
        p.num_update = 0;
        p.rows++;
        // the record's index, in control order (ensureTimeIndex); a failure here surfaces from the writer's own call
        if (p.nc_ctrl >= 0) (void)shud_nc_reserve(o->nc[p.nc_kind], r.tq, &r.rec);
    }
    o->bank ^= 1;
    o->copy_pending = true;
    {
        std::lock_guard<std::mutex> lk(o->mu);
        o->bank_left[bank] = (int)rows.size();
        for (const auto &r : rows) o->tasks[r.ctrl % kWriters].push_back(r);
    }
    o->cv.notify_all();
    return SHUD_OK;
}

extern "C" int shud_out_launches(shud_out_t o, int64_t counts[SHUD_OUT_KERNELS]) {
    if (!o || !counts) return shud_fail(SHUD_ERR_ARG, "null argument");
    for (int k = 0; k < SHUD_OUT_KERNELS; k++) counts[k] = o->n_launch[k];
    return SHUD_OK;
}
extern "C" const char *shud_out_kernel_name(int which) {
    static const char *name[SHUD_OUT_KERNELS] = {"k_accumulate", "k_snap", "k_snap_nc", "k_snap_nc_sel", "k_zone_partial",
                                                 "k_zone_final", "k_snap_wmean"};
    return which >= 0 && which < SHUD_OUT_KERNELS ? name[which] : nullptr;
}

extern "C" int shud_out_flush(shud_out_t o) {
    if (!o) return shud_fail(SHUD_ERR_ARG, "null argument");
    out_drain(o);
    return out_report(o);
}

extern "C" int shud_out_resume(shud_out_t o, int on) {
    if (!o) return shud_fail(SHUD_ERR_ARG, "null argument");
    o->resume = on != 0;
    return SHUD_OK;
}

// ---- checkpoint access (shud_ckpt.cpp) ----
int shud_out_ckpt_check(shud_out *o) {
    for (int k = 0; k < SHUD_NC_KINDS; k++)
        if (o->nc[k])
            return shud_fail(SHUD_ERR_UNSUPPORTED, "shud_ckpt: an output set with a NetCDF sink cannot be checkpointed "
                                                   "(a record file has no reopen path)");
    return SHUD_OK;
}
void *shud_out_ckpt_stream(shud_out *o) { return (void *)o->stream; }
// each control's accumulator, once every queued row is in its file
int shud_out_ckpt_dev(shud_out *o, CkptPart &p) {
    HIP_TRY(hipSetDevice(o->device));
    if (out_drain(o)) return out_report(o);
    HIP_TRY(hipStreamSynchronize(o->stream));            // the last export's accumulate pass
    for (size_t k = 0; k < o->pc.size(); k++) {
        char name[SHUD_CKPT_NAME_LEN];
        snprintf(name, sizeof(name), "out.buf%zu", k);
        p.add(name, o->pc[k].d_buf, ((size_t)std::max(o->pc[k].numvar, 1) + 3) / 4 * 4 * sizeof(double));
    }
    return SHUD_OK;
}
// interval bookkeeping, rows and the byte length of each file; loading cuts every file back to that length
int shud_out_ckpt_host(shud_out *o, CkptAr &a, bool check_only) {
    int n = (int)o->pc.size();
    if (!a.same(n)) return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: field number of output controls differs");
    std::vector<long long> len(2 * (size_t)n, -1);
    for (int k = 0; k < n; k++) {
        PrintCtrl &p = o->pc[k];
        int has_b = p.fb ? 1 : 0, has_a = p.fa ? 1 : 0;
        if (!a.same(p.numvar) || !a.same(p.interval) || !a.same(p.start_time) || !a.same(has_b) || !a.same(has_a))
            return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: output control %d (%s) differs", k, p.filename.c_str());
        int nu = p.num_update;
        int64_t rows = p.rows;
        FILE *fp[2] = {p.fb, p.fa};
        a.pod(nu);
        a.pod(rows);
        for (int j = 0; j < 2; j++) {
            long long l = -1;
            if (!a.load && fp[j]) l = ftello(fp[j]);
            a.pod(l);
            len[2 * k + j] = l;
            if (a.load && fp[j]) {                   // the file must still hold everything up to the checkpoint
                if (fseeko(fp[j], 0, SEEK_END) != 0 || ftello(fp[j]) < l)
                    return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: %s%s is shorter than at the checkpoint",
                                     p.filename.c_str(), j ? ".csv" : ".dat");
            }
        }
        if (a.load && !check_only) {
            p.num_update = nu;
            p.rows = rows;
        }
    }
    // zonal controls: a trailer after the per-control fields, written only by a set that has one (so the section of a
    // set without them is what it always was): a tag, then every control's operation (-1: plain)
    static const char kZoneTag[8] = {'Z', 'O', 'N', 'A', 'L', 'O', 'P', '1'};
    bool zonal = false;
    for (int k = 0; k < n; k++) zonal = zonal || o->pc[k].zone_op >= 0;
    if (zonal) {
        char tag[8];
        memcpy(tag, kZoneTag, 8);
        a.raw(tag, 8);
        if (a.load && (!a.ok || memcmp(tag, kZoneTag, 8) != 0))
            return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: field zone_op is missing: the checkpoint's output set has "
                                           "no zonal control, this one has");
        for (int k = 0; k < n; k++)
            if (!a.same(o->pc[k].zone_op))
                return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: field zone_op of output control %d (%s) differs", k,
                                 o->pc[k].filename.c_str());
    } else if (a.load && a.ok && a.pos + 8 <= a.buf.size() && memcmp(a.buf.data() + a.pos, kZoneTag, 8) == 0) {
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: field zone_op differs: the checkpoint's output set has zonal "
                                       "controls, this one has none");
    }
    if (!a.ok) return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: section out.host is too short");
    if (a.load && !check_only)
        for (int k = 0; k < n; k++) {
            FILE *fp[2] = {o->pc[k].fb, o->pc[k].fa};
            for (int j = 0; j < 2; j++)
                if (fp[j] && (fflush(fp[j]) != 0 || ftruncate(fileno(fp[j]), len[2 * k + j]) != 0 ||
                              fseeko(fp[j], len[2 * k + j], SEEK_SET) != 0))
                    return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: cannot cut %s back", o->pc[k].filename.c_str());
        }
    return SHUD_OK;
}

extern "C" int64_t shud_out_rows(shud_out_t o, int k) {
    if (!o || k < 0 || k >= (int)o->pc.size()) return -1;
    if (out_drain(o)) return out_report(o);          // a writer failure: its (negative) error code
    return o->pc[k].rows;
}

extern "C" int shud_out_destroy(shud_out_t o) {
    if (!o) return SHUD_OK;
    (void)hipSetDevice(o->device);
    out_drain(o);
    const int rc = out_report(o);
    {
        std::lock_guard<std::mutex> lk(o->mu);
        o->stop = true;
    }
    o->cv.notify_all();
    for (int w = 0; w < kWriters; w++)
        if (o->writer[w].joinable()) o->writer[w].join();
    (void)hipStreamSynchronize(o->stream);
    (void)hipStreamSynchronize(o->s_copy);
    for (PrintCtrl &p : o->pc) {
        if (p.fb) fclose(p.fb);
        if (p.fa) fclose(p.fa);
        if (p.d_buf) (void)hipFree(p.d_buf);
        if (p.d_snap) (void)hipFree(p.d_snap);
        if (p.d_sel) (void)hipFree(p.d_sel);
        if (p.d_slab) (void)hipFree(p.d_slab);
        if (p.d_col) (void)hipFree(p.d_col);
        if (p.d_zint) (void)hipFree(p.d_zint);
        if (p.d_zweight) (void)hipFree(p.d_zweight);
        if (p.d_zpart) (void)hipFree(p.d_zpart);
        if (p.d_zwsum) (void)hipFree(p.d_zwsum);
        for (int b = 0; b < 2; b++) {
            if (p.h_buf[b]) (void)hipHostFree(p.h_buf[b]);
            if (p.h_slab[b]) (void)hipHostFree(p.h_slab[b]);
        }
    }
    int nrc = SHUD_OK;
    for (int k = 0; k < SHUD_NC_KINDS; k++)                  // a file with no record is still written, with 0 records
        if (o->nc[k] && shud_nc_close(o->nc[k]) && !nrc) nrc = shud_fail(SHUD_ERR_ARG, "shud_out: %s", shud_nc_last_error());
    if (o->d_slots) (void)hipFree(o->d_slots);
    if (o->d_zslots) (void)hipFree(o->d_zslots);
    if (o->ev_snap) (void)hipEventDestroy(o->ev_snap);
    for (int b = 0; b < 2; b++)
        if (o->ev_copied[b]) (void)hipEventDestroy(o->ev_copied[b]);
    if (o->s_copy) (void)hipStreamDestroy(o->s_copy);
    delete o;
    return rc ? rc : nrc;
}

// ---------------------------------------------------------------------------------------------
// device sources on the RHS handle
// ---------------------------------------------------------------------------------------------
extern "C" int shud_rhs_prepare_outputs(shud_rhs_t h) {
    if (!h) return shud_fail(SHUD_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    const size_t len[5] = {(size_t)h->n_own, (size_t)h->n_own, (size_t)h->n_own, (size_t)h->n_own_riv,
                           (size_t)h->NL};
    int rc;
    for (int k = 0; k < 5; k++)
        if (!h->d_sum[k] && (rc = h->upload(&h->d_sum[k], (const double *)nullptr, len[k]))) return rc;
    if ((rc = shud_ensure_diag(h))) return rc;
    if (!h->d_zero_lake && (rc = h->upload(&h->d_zero_lake, (const double *)nullptr, std::max(h->NL, 1)))) return rc;
    if (!h->d_trans && ((rc = h->upload(&h->d_trans, (const double *)nullptr, h->NE)) ||
                        (rc = h->upload(&h->d_evapo, (const double *)nullptr, h->NE))))
        return rc;
    return SHUD_OK;
}

extern "C" int shud_rhs_summary(shud_rhs_t h, const double *d_y) {
    if (!h || !d_y) return shud_fail(SHUD_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    const int ne = h->n_own, nr = h->n_own_riv, nl = h->NL;
    const size_t len[5] = {(size_t)ne, (size_t)ne, (size_t)ne, (size_t)nr, (size_t)nl};
    for (int k = 0; k < 5; k++)
        if (!h->d_sum[k]) {
            int rc = h->dalloc(&h->d_sum[k], len[k]);
            if (rc) return rc;
        }
    const int n = std::max(ne, std::max(nr, nl));
    if (n > 0)
        hipLaunchKernelGGL(k_summary, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->dm, d_y, ne, nr, nl,
                           h->d_sum[0], h->d_sum[1], h->d_sum[2], h->d_sum[3], h->have_last ? nullptr : h->d_sum[4]);
    HIP_TRY(hipGetLastError());
    return SHUD_OK;
}

extern "C" int shud_rhs_refresh_diagnostics(shud_rhs_t h) {
    if (!h) return shud_fail(SHUD_ERR_ARG, "null argument");
    int rc = shud_diag_replay(h);
    if (rc) return rc;
    const int ne = h->NE;
    if (!h->d_trans && ((rc = h->dalloc(&h->d_trans, ne)) || (rc = h->dalloc(&h->d_evapo, ne)))) return rc;
    if (ne > 0)
        hipLaunchKernelGGL(k_et_sums, dim3((ne + 255) / 256), dim3(256), 0, h->stream, h->dd, ne,
                           h->lakeon ? h->lk.lake_of : nullptr, h->dm.pot_evap, h->d_trans, h->d_evapo);
    HIP_TRY(hipGetLastError());
    // yLakeStg = Y[iLAKE] of the last f() call (f_update, MD_update.cpp:175), like y2LakeArea (lake_toparea above):
    // lakystage.dat and the restart file's lake block hold the last RHS input, not the vector given to summary
    if (h->NL > 0) {
        if (!h->d_sum[4] && (rc = h->dalloc(&h->d_sum[4], (size_t)h->NL))) return rc;
        HIP_TRY(hipMemcpyAsync(h->d_sum[4], h->last_y + 3 * (size_t)h->n_own + (size_t)h->n_own_riv,
                               (size_t)h->NL * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    }
    return SHUD_OK;
}

extern "C" const double *shud_rhs_device_array(shud_rhs_t h, int which, int64_t *n) {
    if (!h) return nullptr;
    const int64_t ne = h->n_own, nr = h->n_own_riv, nl = h->NL;
    const double *p = nullptr;
    int64_t len = 0;
    const DevDiag &d = h->dd;
    switch (which) {
        case SHUD_ARR_Y_ELE_SURF: p = h->d_sum[0]; len = ne; break;
        case SHUD_ARR_Y_ELE_UNSAT: p = h->d_sum[1]; len = ne; break;
        case SHUD_ARR_Y_ELE_GW: p = h->d_sum[2]; len = ne; break;
        case SHUD_ARR_Y_RIV_STG: p = h->d_sum[3]; len = nr; break;
        case SHUD_ARR_Y_LAKE_STG: p = h->d_sum[4]; len = nl; break;
        case SHUD_ARR_QELE_SURF_TOT: p = d.qele_surf_tot; len = ne; break;
        case SHUD_ARR_QELE_SUB_TOT: p = d.qele_sub_tot; len = ne; break;
        case SHUD_ARR_QELE_SURF: p = d.qele_surf; len = 3 * (int64_t)h->NE; break;
        case SHUD_ARR_QELE_SUB: p = d.qele_sub; len = 3 * (int64_t)h->NE; break;
        case SHUD_ARR_QE2R_SURF: p = d.qe2r_surf; len = ne; break;
        case SHUD_ARR_QE2R_SUB: p = d.qe2r_sub; len = ne; break;
        case SHUD_ARR_Q_INFIL: p = d.q_infil; len = ne; break;
        case SHUD_ARR_Q_EXFIL: p = d.q_exfil; len = ne; break;
        case SHUD_ARR_Q_RECHARGE: p = d.q_recharge; len = ne; break;
        case SHUD_ARR_Q_ETA: p = d.q_eta; len = ne; break;
        case SHUD_ARR_Q_E_IC: p = d.e_ic; len = ne; break;
        case SHUD_ARR_Q_TRANS: p = h->d_trans; len = ne; break;
        case SHUD_ARR_Q_EVAPO: p = h->d_evapo; len = ne; break;
        case SHUD_ARR_QRIV_DOWN: p = d.qriv_down; len = nr; break;
        case SHUD_ARR_QRIV_UP: p = d.qriv_up; len = nr; break;
        case SHUD_ARR_QRIV_SURF: p = d.qriv_surf; len = nr; break;
        case SHUD_ARR_QRIV_SUB: p = d.qriv_sub; len = nr; break;
        case SHUD_ARR_Q_PRCP: p = h->dm.prcp; len = ne; break;
        case SHUD_ARR_Q_NET_PRCP: p = h->dm.net_prep; len = ne; break;
        case SHUD_ARR_Q_ETP: p = h->dm.etp; len = ne; break;
        case SHUD_ARR_Y_ELE_IS: p = shud_et_array(h, which); len = ne; break;
        case SHUD_ARR_Y_ELE_SNOW: p = shud_et_array(h, which); len = ne; break;
        case SHUD_ARR_RN_H: p = shud_et_array(h, which); len = ne; break;
        case SHUD_ARR_RN_T: p = shud_et_array(h, which); len = ne; break;
        case SHUD_ARR_RN_FACTOR: p = shud_et_array(h, which); len = ne; break;
        case SHUD_ARR_LAKE_TOPAREA: p = nl ? d.lake_toparea : nullptr; len = nl; break;
        case SHUD_ARR_Q_LAKE_EVAP: p = nl ? d.q_lake_evap : nullptr; len = nl; break;
        case SHUD_ARR_Q_LAKE_PRCP: p = nl ? d.q_lake_prcp : nullptr; len = nl; break;
        case SHUD_ARR_Q_LAKE_RIVIN: p = nl ? d.q_lake_rivin : nullptr; len = nl; break;
        case SHUD_ARR_Q_LAKE_RIVOUT: p = nl ? h->d_zero_lake : nullptr; len = nl; break;
        case SHUD_ARR_Q_LAKE_SURF: p = nl ? d.q_lake_surf : nullptr; len = nl; break;
        case SHUD_ARR_Q_LAKE_SUB: p = nl ? d.q_lake_sub : nullptr; len = nl; break;
        default: break;
    }
    if (n) *n = p ? len : 0;
    return p;
}
