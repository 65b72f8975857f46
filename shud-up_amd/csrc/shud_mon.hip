// shud_mon.hip — run monitors on the device (include/shud_mon.h): <prj>.flood.csv and <prj>.cfg.ic.update.
//
// The reference scans yRivStg on the host after every solver step (FloodAlert::FloodWarning, FloodAlert.cpp:71-87)
// and prints the five element storages and the reach / lake stages every UpdateICStep minutes (Model_Data::PrintInit,
// MD_update.cpp:268-299).  Here those arrays live in HBM, so selection and packing happen there:
//   flood pass   order-preserving stream compaction in three short launches: k_flood_count (wave ballots, one count
//                per 256-reach block), k_flood_scan (one block: exclusive scan of the block counts, total to the
//                count word), k_flood_scatter (ballot rank + block offset -> packed ShudFloodRec).  No workgroup
//                waits on another.  The count word goes to a pinned host word on the copy stream; the writer thread
//                then copies exactly `count` records on its own stream, so with no flood only 4 bytes cross PCIe.
//   IC pass      k_ic_pack reads each of the five element arrays with one coalesced load per array and transposes
//                through LDS into row-major [n_ele][5] records (contiguous stores per wave); reach and lake stages
//                follow in the same staging buffer, which goes device->host on the copy stream into one of two
//                pinned banks (the pattern of shud_out.hip).
// Two writer threads, one per file (flood rows never queue behind the formatting of a snapshot), format through
// shud_mon_fmt.cpp in call order.  shud_mon_flood / shud_mon_ic_update return after enqueue; a call that finds its
// bank still with its writer waits for it (banks alternate, so that is the older one): nothing is dropped or
// reordered.  A failed copy means those rows / that snapshot are not written; the first failure is reported by
// flush, destroy and the row getters.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "shud_ckpt_parts.h"
#include "shud_diag_host.h"
#include "shud_handle.h"
#include "shud_mon.h"
#include "shud_mon_fmt.h"

namespace {

constexpr int kB = 256;                  // threads per block (4 waves of 64)
constexpr int kW = kB / 64;

// reaches above their bank in this block's 256 (strict >: NaN is not above, +inf is)
__global__ void __launch_bounds__(kB) k_flood_count(const double *__restrict__ stage, const double *__restrict__ depth,
                                                    int n, int *__restrict__ blk) {
    __shared__ int wc[kW];
    const int i = blockIdx.x * kB + threadIdx.x;
    const bool f = i < n && stage[i] > depth[i];
    const unsigned long long b = __ballot(f);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kW; w++) s += wc[w];
        blk[blockIdx.x] = s;
    }
}

// one block: blk[0..nb) counts -> exclusive offsets in place, the total to *count
__global__ void __launch_bounds__(kB) k_flood_scan(int *__restrict__ blk, int nb, int *__restrict__ count) {
    __shared__ int ws[kW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < nb; base += kB) {
        const int k = base + threadIdx.x;
        const int v = k < nb ? blk[k] : 0;
        int x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) ws[wave] = x;
        __syncthreads();
        int woff = 0, tot = 0;
        for (int w = 0; w < kW; w++) {
            if (w < wave) woff += ws[w];
            tot += ws[w];
        }
        if (k < nb) blk[k] = carry + woff + x - v;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = carry;
}

// record of reach i at blk[block] + (flooded reaches before i in the block): ascending i
__global__ void __launch_bounds__(kB) k_flood_scatter(const double *__restrict__ stage, const double *__restrict__ qdown,
                                                      const double *__restrict__ depth, int n,
                                                      const int *__restrict__ blk, ShudFloodRec *__restrict__ rec) {
    __shared__ int wc[kW];
    const int i = blockIdx.x * kB + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double s = 0.0;
    bool f = false;
    if (i < n) {
        s = stage[i];
        f = s > depth[i];
    }
    const unsigned long long b = __ballot(f);
    if (lane == 0) wc[wave] = __popcll(b);
    __syncthreads();
    if (!f) return;
    int pos = blk[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) pos += wc[w];
    ShudFloodRec r;
    r.idx = i;
    r.pad = 0;
    r.stage = s;
    r.qdown = qdown[i];
    rec[pos] = r;                        // pos < total <= n
}

struct IcSrc {
    const double *col[5];                // yEleIS, yEleSnow, yEleSurf, yEleUnsat, yEleGW
    const double *riv, *lake;
    int ne, nr, nl;
    const int *inv;                      // shud_mon_set_ic_order: file row c reads source element inv[c]; nullptr = c
};

// pack = [ne][5] row-major | riv[nr] | lake[nl]
__global__ void __launch_bounds__(kB) k_ic_pack(IcSrc s, double *__restrict__ pack) {
    __shared__ double tile[kB * 5];
    const int base = blockIdx.x * kB;
    const int i = base + threadIdx.x;
    if (base < s.ne) {
        const int cnt = min(kB, s.ne - base);
        if (threadIdx.x < cnt) {
            const int e = s.inv ? s.inv[i] : i;
            for (int k = 0; k < 5; k++) tile[threadIdx.x * 5 + k] = s.col[k][e];
        }
        __syncthreads();
        double *out = pack + (size_t)base * 5;
        for (int j = threadIdx.x; j < cnt * 5; j += kB) out[j] = tile[j];
    }
    if (i < s.nr) pack[(size_t)s.ne * 5 + i] = s.riv[i];
    if (i < s.nl) pack[(size_t)s.ne * 5 + s.nr + i] = s.lake[i];
}

struct MonTask {
    int kind;                            // 0 flood rows, 1 IC snapshot
    int bank;
    double t;
};

}  // namespace

struct shud_mon {
    int device = 0;
    hipStream_t stream = nullptr;        // the caller's compute stream
    hipStream_t s_copy = nullptr;        // count words and snapshots, device -> host
    hipStream_t s_wr = nullptr;          // the writer's copies of the packed flood records
    // ---- flood ----
    bool have_flood = false;
    FILE *ff = nullptr;
    std::string fpath;
    int nr = 0, nb = 0;
    std::vector<double> depth;
    std::vector<int32_t> type;
    const double *d_stage = nullptr, *d_qdown = nullptr;
    double *d_depth = nullptr;
    int *d_blk = nullptr;
    ShudFloodRec *d_rec[2] = {nullptr, nullptr}, *h_rec[2] = {nullptr, nullptr};
    int *d_cnt[2] = {nullptr, nullptr}, *h_cnt[2] = {nullptr, nullptr};
    hipEvent_t ev_fk[2] = {nullptr, nullptr}, ev_fc[2] = {nullptr, nullptr};
    int fbank = 0;
    bool f_busy[2] = {false, false};
    int64_t rows = 0;
    int last = 0;
    // ---- IC snapshots ----
    bool have_ic = false;
    std::string ipath;
    int step = 0;
    IcSrc src{};
    int *d_inv = nullptr;                // IcSrc::inv
    size_t npack = 0;
    double *d_pack = nullptr, *h_pack[2] = {nullptr, nullptr};
    hipEvent_t ev_ik = nullptr, ev_ic[2] = {nullptr, nullptr};
    int ibank = 0;
    bool i_busy[2] = {false, false};
    bool i_copy_pending = false;
    int64_t snaps = 0;
    // ---- writer ----
    std::thread writer[2];               // [0] flood rows, [1] snapshots
    std::mutex mu;
    std::condition_variable cv;
    std::deque<MonTask> tasks[2];
    int pending = 0;                     // queued + in progress, both writers
    bool stop = false;
    double wsec = 0.0;
    int werr = 0;
    std::string werr_msg;
    bool resume = false;                 // shud_mon_resume: add_flood keeps the file of an earlier run
};

static void mon_fail(shud_mon *m, int code, const std::string &msg) {
    std::lock_guard<std::mutex> lk(m->mu);
    if (!m->werr) { m->werr = code; m->werr_msg = msg; }
}

static void mon_writer(shud_mon *m, int kind) {
    (void)hipSetDevice(m->device);
    for (;;) {
        MonTask job;
        {
            std::unique_lock<std::mutex> lk(m->mu);
            m->cv.wait(lk, [&] { return m->stop || !m->tasks[kind].empty(); });
            if (m->tasks[kind].empty()) return;
            job = m->tasks[kind].front();
            m->tasks[kind].pop_front();
        }
        int64_t nrow = 0;
        bool wrote = false;
        double sec = 0.0;
        if (job.kind == 0) {
            hipError_t he = hipEventSynchronize(m->ev_fc[job.bank]);
            int n = he == hipSuccess ? *m->h_cnt[job.bank] : 0;
            if (he == hipSuccess && (n < 0 || n > m->nr)) {
                mon_fail(m, SHUD_ERR_HIP, "flood pass: record count out of range: rows of " + m->fpath + " not written");
                n = 0;
            } else if (he == hipSuccess && n > 0) {
                he = hipMemcpyAsync(m->h_rec[job.bank], m->d_rec[job.bank], (size_t)n * sizeof(ShudFloodRec),
                                    hipMemcpyDeviceToHost, m->s_wr);
                if (he == hipSuccess) he = hipStreamSynchronize(m->s_wr);
            }
            if (he != hipSuccess) {
                mon_fail(m, SHUD_ERR_HIP, std::string("flood record copy failed (") + hipGetErrorString(he) +
                                              "): rows of " + m->fpath + " not written");
            } else if (n > 0) {
                const auto w0 = std::chrono::steady_clock::now();
                if (shud_mon_fmt_flood_file(m->ff, job.t, m->h_rec[job.bank], n, m->type.data(), m->depth.data()))
                    mon_fail(m, SHUD_MON_ERR_IO, "write error on " + m->fpath);
                else
                    nrow = n;
                sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
            }
        } else {
            const hipError_t he = hipEventSynchronize(m->ev_ic[job.bank]);
            if (he != hipSuccess) {
                mon_fail(m, SHUD_ERR_HIP, std::string("snapshot copy failed (") + hipGetErrorString(he) + "): " +
                                              m->ipath + " not written");
            } else {
                const auto w0 = std::chrono::steady_clock::now();
                const double *hp = m->h_pack[job.bank];
                const double *const col[5] = {hp, hp + 1, hp + 2, hp + 3, hp + 4};
                const double *riv = hp + (size_t)m->src.ne * 5;
                if (shud_mon_fmt_write_ic(m->ipath.c_str(), job.t, m->src.ne, m->src.nr, m->src.nl, col, 5, riv,
                                          riv + m->src.nr))
                    mon_fail(m, SHUD_MON_ERR_IO, "cannot write " + m->ipath + ": " + strerror(errno));
                else
                    wrote = true;
                sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
            }
        }
        {
            std::lock_guard<std::mutex> lk(m->mu);
            if (job.kind == 0) {
                m->f_busy[job.bank] = false;
                m->rows += nrow;
                m->last = nrow > 0;
            } else {
                m->i_busy[job.bank] = false;
                if (wrote) m->snaps++;
            }
            m->wsec += sec;
            m->pending--;
        }
        m->cv.notify_all();
    }
}

// wait until the writer is idle; returns its first failure
static int mon_drain(shud_mon *m) {
    std::unique_lock<std::mutex> lk(m->mu);
    m->cv.wait(lk, [&] { return m->pending == 0; });
    if (m->ff && fflush(m->ff) != 0 && !m->werr) { m->werr = SHUD_MON_ERR_IO; m->werr_msg = "flush error on " + m->fpath; }
    return m->werr;
}
static int mon_report(shud_mon *m) {
    return m->werr ? shud_fail(m->werr, "shud_mon: %s", m->werr_msg.c_str()) : SHUD_OK;
}
static void mon_push(shud_mon *m, MonTask t) {
    {
        std::lock_guard<std::mutex> lk(m->mu);
        (t.kind == 0 ? m->f_busy : m->i_busy)[t.bank] = true;
        m->tasks[t.kind].push_back(t);
        m->pending++;
    }
    m->cv.notify_all();
}

extern "C" int shud_mon_create(int device, void *stream, shud_mon_t *out) {
    if (!out) return shud_fail(SHUD_ERR_ARG, "null argument");
    *out = nullptr;
    HIP_TRY(hipSetDevice(device));
    shud_mon *m = new shud_mon;
    m->device = device;
    m->stream = (hipStream_t)stream;
    *out = m;                            // a failure below leaves a handle shud_mon_destroy can free
    for (int k = 0; k < 2; k++) m->writer[k] = std::thread(mon_writer, m, k);
    HIP_TRY(hipStreamCreateWithFlags(&m->s_copy, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&m->s_wr, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&m->ev_ik, hipEventDisableTiming));
    for (int b = 0; b < 2; b++) {
        HIP_TRY(hipEventCreateWithFlags(&m->ev_fk[b], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&m->ev_fc[b], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&m->ev_ic[b], hipEventDisableTiming));
    }
    return SHUD_OK;
}

extern "C" int shud_mon_add_flood(shud_mon_t m, const ShudFloodSpec *s) {
    if (!m || !s || !s->path) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (m->have_flood) return shud_fail(SHUD_ERR_ARG, "shud_mon_add_flood: already added");
    if (s->n_riv < 0 || (s->n_riv > 0 && (!s->d_stage || !s->d_qdown || !s->riv_depth || !s->riv_type)))
        return shud_fail(SHUD_ERR_ARG, "shud_mon_add_flood: bad n_riv or missing array");
    HIP_TRY(hipSetDevice(m->device));
    FILE *fp = fopen(s->path, m->resume ? "r+" : "w");               // InitFile
    if (!fp) return shud_fail(SHUD_MON_ERR_IO, "shud_mon_add_flood: cannot open %s: %s", s->path, strerror(errno));
    if (m->resume) {                     // shud_mon_resume: an earlier run's file, kept; its header must be ours
        const std::string want = shud_mon_flood_header();
        std::vector<char> have(want.size());
        if (fread(have.data(), 1, have.size(), fp) != have.size() || memcmp(have.data(), want.data(), want.size()) != 0 ||
            fseek(fp, 0, SEEK_END) != 0) {
            fclose(fp);
            return shud_fail(SHUD_ERR_ARG, "shud_mon_add_flood (resume): %s does not start with the flood header", s->path);
        }
    } else if (fputs(shud_mon_flood_header(), fp) < 0 || fflush(fp) != 0) {
        fclose(fp);
        return shud_fail(SHUD_MON_ERR_IO, "shud_mon_add_flood: cannot write %s", s->path);
    }
    m->ff = fp;
    m->fpath = s->path;
    const int nr = m->nr = s->n_riv;
    m->nb = (nr + kB - 1) / kB;
    m->depth.assign(s->riv_depth, s->riv_depth + nr);
    m->type.assign(s->riv_type, s->riv_type + nr);
    m->d_stage = s->d_stage;
    m->d_qdown = s->d_qdown;
    const size_t n1 = std::max(nr, 1);
    HIP_TRY(hipMalloc(&m->d_depth, n1 * sizeof(double)));
    if (nr) HIP_TRY(hipMemcpy(m->d_depth, m->depth.data(), (size_t)nr * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&m->d_blk, std::max(m->nb, 1) * sizeof(int)));
    for (int b = 0; b < 2; b++) {
        HIP_TRY(hipMalloc(&m->d_rec[b], n1 * sizeof(ShudFloodRec)));
        HIP_TRY(hipMalloc(&m->d_cnt[b], sizeof(int)));
        HIP_TRY(hipHostMalloc(&m->h_rec[b], n1 * sizeof(ShudFloodRec), hipHostMallocDefault));
        HIP_TRY(hipHostMalloc(&m->h_cnt[b], sizeof(int), hipHostMallocDefault));
        *m->h_cnt[b] = 0;
    }
    m->have_flood = true;
    return SHUD_OK;
}

// the three launches of one pass into bank b (compute stream)
static int flood_launch(shud_mon *m, int b) {
    if (m->nr > 0) {
        hipLaunchKernelGGL(k_flood_count, dim3(m->nb), dim3(kB), 0, m->stream, m->d_stage, m->d_depth, m->nr, m->d_blk);
        hipLaunchKernelGGL(k_flood_scan, dim3(1), dim3(kB), 0, m->stream, m->d_blk, m->nb, m->d_cnt[b]);
        hipLaunchKernelGGL(k_flood_scatter, dim3(m->nb), dim3(kB), 0, m->stream, m->d_stage, m->d_qdown, m->d_depth,
                           m->nr, m->d_blk, m->d_rec[b]);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(m->d_cnt[b], 0, sizeof(int), m->stream));
    }
    return SHUD_OK;
}

extern "C" int shud_mon_flood(shud_mon_t m, double t) {
    if (!m) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (!m->have_flood) return shud_fail(SHUD_ERR_ARG, "shud_mon_flood: no flood monitor (shud_mon_add_flood)");
    HIP_TRY(hipSetDevice(m->device));
    const int b = m->fbank;
    {
        std::unique_lock<std::mutex> lk(m->mu);
        m->cv.wait(lk, [&] { return !m->f_busy[b]; });
    }
    int rc = flood_launch(m, b);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(m->ev_fk[b], m->stream));
    HIP_TRY(hipStreamWaitEvent(m->s_copy, m->ev_fk[b], 0));
    HIP_TRY(hipMemcpyAsync(m->h_cnt[b], m->d_cnt[b], sizeof(int), hipMemcpyDeviceToHost, m->s_copy));
    HIP_TRY(hipEventRecord(m->ev_fc[b], m->s_copy));
    m->fbank ^= 1;
    mon_push(m, MonTask{0, b, t});
    return SHUD_OK;
}

extern "C" int64_t shud_mon_flood_rows(shud_mon_t m) {
    if (!m) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (mon_drain(m)) return mon_report(m);
    return m->rows;
}

extern "C" int shud_mon_flood_last(shud_mon_t m) {
    if (!m) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (mon_drain(m)) return mon_report(m);
    return m->last;
}

extern "C" int shud_mon_add_ic(shud_mon_t m, const ShudIcSpec *s) {
    if (!m || !s || !s->path_update) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (m->have_ic) return shud_fail(SHUD_ERR_ARG, "shud_mon_add_ic: already added");
    if (s->update_ic_step < 1)
        return shud_fail(SHUD_ERR_ARG, "shud_mon_add_ic: Update_IC_STEP %d (the reference divides by it: must be >= 1)",
                         s->update_ic_step);
    if (s->n_ele < 0 || s->n_riv < 0 || s->n_lake < 0 ||
        (s->n_ele > 0 && (!s->d_is || !s->d_snow || !s->d_surf || !s->d_unsat || !s->d_gw)) ||
        (s->n_riv > 0 && !s->d_riv) || (s->n_lake > 0 && !s->d_lake))
        return shud_fail(SHUD_ERR_ARG, "shud_mon_add_ic: bad size or missing array");
    HIP_TRY(hipSetDevice(m->device));
    // the directory must take the temporary file every snapshot goes through
    const std::string tmp = std::string(s->path_update) + ".tmp";
    FILE *fp = fopen(tmp.c_str(), "w");
    if (!fp) return shud_fail(SHUD_MON_ERR_IO, "shud_mon_add_ic: cannot open %s: %s", tmp.c_str(), strerror(errno));
    fclose(fp);
    remove(tmp.c_str());
    m->ipath = s->path_update;
    m->step = s->update_ic_step;
    m->src = IcSrc{{s->d_is, s->d_snow, s->d_surf, s->d_unsat, s->d_gw}, s->d_riv, s->d_lake, s->n_ele, s->n_riv,
                   s->n_lake, nullptr};
    m->npack = (size_t)s->n_ele * 5 + s->n_riv + s->n_lake;
    const size_t nb = std::max<size_t>(m->npack, 1) * sizeof(double);
    HIP_TRY(hipMalloc(&m->d_pack, nb));
    for (int b = 0; b < 2; b++) HIP_TRY(hipHostMalloc(&m->h_pack[b], nb, hipHostMallocDefault));
    m->have_ic = true;
    return SHUD_OK;
}

extern "C" int shud_mon_set_ic_order(shud_mon_t m, const int32_t *perm) {
    if (!m || !perm) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (!m->have_ic) return shud_fail(SHUD_ERR_ARG, "shud_mon_set_ic_order: no snapshot monitor (shud_mon_add_ic)");
    const int ne = m->src.ne;
    std::vector<int> inv((size_t)std::max(ne, 1), -1);
    for (int k = 0; k < ne; k++) {
        if (perm[k] < 0 || perm[k] >= ne || inv[perm[k]] >= 0)
            return shud_fail(SHUD_ERR_ARG, "shud_mon_set_ic_order: not a permutation at entry %d", k);
        inv[perm[k]] = k;
    }
    HIP_TRY(hipSetDevice(m->device));
    if (!m->d_inv) HIP_TRY(hipMalloc(&m->d_inv, inv.size() * sizeof(int)));
    // stream-ordered after the pack kernels already enqueued, before the next one
    HIP_TRY(hipMemcpyAsync(m->d_inv, inv.data(), inv.size() * sizeof(int), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    m->src.inv = m->d_inv;
    return SHUD_OK;
}

extern "C" int shud_mon_ic_update(shud_mon_t m, double t) {
    if (!m) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (!m->have_ic) return shud_fail(SHUD_ERR_ARG, "shud_mon_ic_update: no snapshot monitor (shud_mon_add_ic)");
    const unsigned long t_long = (unsigned long)(long)t;             // PrintInit's test
    if (t_long % (unsigned long)m->step) return 0;
    HIP_TRY(hipSetDevice(m->device));
    const int b = m->ibank;
    {
        std::unique_lock<std::mutex> lk(m->mu);
        m->cv.wait(lk, [&] { return !m->i_busy[b]; });
    }
    // the staging buffer is free once the previous snapshot's copy has finished
    if (m->i_copy_pending) HIP_TRY(hipStreamWaitEvent(m->stream, m->ev_ic[b ^ 1], 0));
    const int n = std::max(m->src.ne, std::max(m->src.nr, m->src.nl));
    if (n > 0) {
        hipLaunchKernelGGL(k_ic_pack, dim3((n + kB - 1) / kB), dim3(kB), 0, m->stream, m->src, m->d_pack);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(m->ev_ik, m->stream));
    HIP_TRY(hipStreamWaitEvent(m->s_copy, m->ev_ik, 0));
    if (m->npack)
        HIP_TRY(hipMemcpyAsync(m->h_pack[b], m->d_pack, m->npack * sizeof(double), hipMemcpyDeviceToHost, m->s_copy));
    HIP_TRY(hipEventRecord(m->ev_ic[b], m->s_copy));
    m->ibank ^= 1;
    m->i_copy_pending = true;
    mon_push(m, MonTask{1, b, t});
    return 1;
}

extern "C" int64_t shud_mon_ic_snapshots(shud_mon_t m) {
    if (!m) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (mon_drain(m)) return mon_report(m);
    return m->snaps;
}

extern "C" int shud_mon_flush(shud_mon_t m) {
    if (!m) return shud_fail(SHUD_ERR_ARG, "null argument");
    mon_drain(m);
    return mon_report(m);
}

extern "C" int shud_mon_resume(shud_mon_t m, int on) {
    if (!m) return shud_fail(SHUD_ERR_ARG, "null argument");
    m->resume = on != 0;
    return SHUD_OK;
}

// checkpoint access (shud_ckpt.cpp): the flood file's length with its row counters, and the snapshot counter;
// loading cuts the flood file back to that length
int shud_mon_ckpt_host(shud_mon *m, CkptAr &a, bool check_only) {
    if (mon_drain(m)) return mon_report(m);
    int hf = m->have_flood ? 1 : 0, hi = m->have_ic ? 1 : 0;
    if (!a.same(hf) || !a.same(hi) || !a.same(m->nr))
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: field monitors (flood / snapshots / reaches) differs");
    int64_t rows = m->rows, snaps = m->snaps;
    int last = m->last;
    long long len = (!a.load && m->ff) ? (long long)ftello(m->ff) : -1;
    a.pod(rows); a.pod(snaps); a.pod(last); a.pod(len);
    if (!a.ok) return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: section mon.host is too short");
    if (!a.load) return SHUD_OK;
    if (m->ff && (fseeko(m->ff, 0, SEEK_END) != 0 || ftello(m->ff) < len))
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: %s is shorter than at the checkpoint", m->fpath.c_str());
    if (check_only) return SHUD_OK;
    if (m->ff && (fflush(m->ff) != 0 || ftruncate(fileno(m->ff), len) != 0 || fseeko(m->ff, len, SEEK_SET) != 0))
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt_restore: cannot cut %s back", m->fpath.c_str());
    m->rows = rows; m->snaps = snaps; m->last = last;
    return SHUD_OK;
}

extern "C" double shud_mon_writer_seconds(shud_mon_t m) {
    if (!m) return 0.0;
    mon_drain(m);
    return m->wsec;
}

extern "C" int shud_mon_time_flood(shud_mon_t m, int reps, double *ms_pass) {
    if (!m || !ms_pass || reps < 1) return shud_fail(SHUD_ERR_ARG, "bad argument");
    if (!m->have_flood) return shud_fail(SHUD_ERR_ARG, "shud_mon_time_flood: no flood monitor");
    HIP_TRY(hipSetDevice(m->device));
    if (mon_drain(m)) return mon_report(m);          // both banks idle: bank 0 is free to scribble on
    return shud::time_passes(m->stream, reps, [&]() -> int {
        const int rc = flood_launch(m, 0);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(m->h_cnt[0], m->d_cnt[0], sizeof(int), hipMemcpyDeviceToHost, m->stream));
        return SHUD_OK;
    }, ms_pass);
}

extern "C" int shud_mon_destroy(shud_mon_t m) {
    if (!m) return SHUD_OK;
    (void)hipSetDevice(m->device);
    mon_drain(m);
    const int rc = mon_report(m);
    {
        std::lock_guard<std::mutex> lk(m->mu);
        m->stop = true;
    }
    m->cv.notify_all();
    for (int k = 0; k < 2; k++)
        if (m->writer[k].joinable()) m->writer[k].join();
    (void)hipStreamSynchronize(m->stream);
    if (m->s_copy) (void)hipStreamSynchronize(m->s_copy);
    if (m->s_wr) (void)hipStreamSynchronize(m->s_wr);
    int rc_close = SHUD_OK;
    if (m->ff && fclose(m->ff) != 0 && !rc) rc_close = shud_fail(SHUD_MON_ERR_IO, "shud_mon: close error on %s", m->fpath.c_str());
    if (m->d_depth) (void)hipFree(m->d_depth);
    if (m->d_blk) (void)hipFree(m->d_blk);
    if (m->d_pack) (void)hipFree(m->d_pack);
    if (m->d_inv) (void)hipFree(m->d_inv);
    for (int b = 0; b < 2; b++) {
        if (m->d_rec[b]) (void)hipFree(m->d_rec[b]);
        if (m->d_cnt[b]) (void)hipFree(m->d_cnt[b]);
        if (m->h_rec[b]) (void)hipHostFree(m->h_rec[b]);
        if (m->h_cnt[b]) (void)hipHostFree(m->h_cnt[b]);
        if (m->h_pack[b]) (void)hipHostFree(m->h_pack[b]);
        if (m->ev_fk[b]) (void)hipEventDestroy(m->ev_fk[b]);
        if (m->ev_fc[b]) (void)hipEventDestroy(m->ev_fc[b]);
        if (m->ev_ic[b]) (void)hipEventDestroy(m->ev_ic[b]);
    }
    if (m->ev_ik) (void)hipEventDestroy(m->ev_ik);
    if (m->s_copy) (void)hipStreamDestroy(m->s_copy);
    if (m->s_wr) (void)hipStreamDestroy(m->s_wr);
    delete m;
    return rc ? rc : rc_close;
}
