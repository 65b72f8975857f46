// shud_tables.cpp — create-time planning: everything between "validate the inputs" and "here are the bytes to upload"
// (shud_tables.h).  Runs once per handle and touches no device, so shud_rhs_plan_layout (below) can show on any
// machine what shud_rhs_create would lay out.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "shud_handle.h"
#include "shud_tables.h"
#define SHUD_PT_HOST_TABLES           // the pow_tab tables as host arrays, uploaded with the class table
#include "shud_pow_tab.h"

using namespace shud;

// Run-time switches read from the environment (A/B measurements and tests).  Each is parsed strictly: a value that is
// not an integer in [lo, hi] is ignored with a warning, and a value that takes effect is announced once per process on
// stderr — a stray variable in a user's environment cannot silently change kernel selection.
int env_knob(const char *name, int def, int lo, int hi) {
    const char *v = getenv(name);
    if (!v || !*v) return def;
    char *end = nullptr;
    const long x = strtol(v, &end, 10);
    static std::vector<std::string> said;
    const bool first = std::find(said.begin(), said.end(), std::string(name)) == said.end();
    if (first) said.push_back(name);
    if (*end || x < lo || x > hi) {
        if (first) fprintf(stderr, "shud_rhs: ignoring %s=%s (expected an integer in [%d, %d])\n", name, v, lo, hi);
        return def;
    }
    if (first && x != def) fprintf(stderr, "shud_rhs: %s=%ld in effect (default %d)\n", name, x, def);
    return (int)x;
}

namespace {

bool lake_ele(const ShudMeshSoA *m, int i) { return m->ilake && m->ilake[i] > 0; }

// CSR of the items 0..n-1 by group: idx[off[g] .. off[g + 1]) are the items with key(i) == g, ascending (a stable
// counting sort); an item with a negative key belongs to no group
template <class Key>
void group_by(int n, int ngroups, Key key, std::vector<int> &off, std::vector<int> &idx) {
    off.assign(ngroups + 1, 0);
    for (int i = 0; i < n; i++)
        if (const int g = key(i); g >= 0) off[g + 1]++;
    for (int g = 0; g < ngroups; g++) off[g + 1] += off[g];
    idx.resize(off[ngroups]);
    std::vector<int> fill(off.begin(), off.end() - 1);
    for (int i = 0; i < n; i++)
        if (const int g = key(i); g >= 0) idx[fill[g]++] = i;
}
// every group of such a CSR in the order `less` (partitioned handles: local ids -> the global summation order)
template <class Less>
void sort_groups(const std::vector<int> &off, std::vector<int> &idx, Less less) {
    for (size_t g = 0; g + 1 < off.size(); g++) std::sort(idx.begin() + off[g], idx.begin() + off[g + 1], less);
}

// The reference exits on these at run time; we reject them up front.  Fills the scalars of T.
int validate(const ShudMeshSoA *m, const ShudParamsSoA *p, const ShudRhsOptions *opt, const ShudPartition *part,
             MeshTables &T) {
    const int NE = m->num_ele, NR = m->num_riv, NS = m->num_seg;
    if (NE < 0 || NR < 0 || NS < 0) return shud_fail(SHUD_ERR_ARG, "negative sizes");
    T.mode = opt ? opt->mode : SHUD_MODE_SERIAL;
    if (T.mode != SHUD_MODE_SERIAL && T.mode != SHUD_MODE_OMP) return shud_fail(SHUD_ERR_ARG, "bad mode %d", T.mode);
    T.open = (m->close_boundary == 0);
    T.n_own = part ? part->n_own_ele : NE;
    T.n_segghost = part ? part->n_segghost_ele : 0;
    T.n_own_riv = part ? part->n_own_riv : NR;
    if (T.n_own < 0 || T.n_own + T.n_segghost > NE || T.n_own_riv < 0 || T.n_own_riv > NR)
        return shud_fail(SHUD_ERR_ARG, "partition counts inconsistent with mesh sizes");
    if (!m->nabr || !m->area || !m->z_surf || !m->z_bottom || !m->edge || !m->dist2nabor || !m->avg_rough)
        return shud_fail(SHUD_ERR_ARG, "missing element geometry array");
    if (T.open && (!m->dist2edge || !m->rough)) return shud_fail(SHUD_ERR_ARG, "open boundary needs dist2edge and rough");
    if (NR && (!m->riv_down || !m->riv_length || !m->riv_bed_slope || !m->riv_dist2down || !m->riv_avg_rough ||
               !m->riv_depth || !m->riv_bottom_width || !m->riv_bankslope || !m->riv_ksath || !m->riv_bedthick))
        return shud_fail(SHUD_ERR_ARG, "missing river array");
    if (NS && (!m->seg_ele || !m->seg_riv || !m->seg_length || !m->seg_cwr)) return shud_fail(SHUD_ERR_ARG, "missing segment array");
    const double *pp[17] = {p->aquifer_depth, p->macD, p->macKsatH, p->geo_vAreaF, p->KsatH, p->KsatV,
                            p->infKsatV, p->hAreaF, p->macKsatV, p->ThetaS, p->ThetaR, p->Beta,
                            p->infD, p->Sy, p->RzD, p->VegFrac, p->ImpAF};
    for (int k = 0; k < 17; k++)
        if (!pp[k]) return shud_fail(SHUD_ERR_ARG, "missing parameter array #%d", k);
    for (long long q = 0; q < 3LL * NE; q++)
        if (m->nabr[q] < -1 || m->nabr[q] >= NE) return shud_fail(SHUD_ERR_ARG, "nabr[%lld]=%d out of range", q, m->nabr[q]);
    // lakes: on when any iLake > 0 (MD_readin.cpp:262-263); serial semantics, packed layout.  Partitioned:
    // the plan (shud_partition.h) puts a lake's elements and bank elements on one rank and numbers its lakes
    // locally, so every lake sum is formed from owned elements and owned or ghost reaches
    for (int i = 0; i < NE && !T.lakeon; i++) T.lakeon = lake_ele(m, i);
    if (T.lakeon) {
        if (T.mode != SHUD_MODE_SERIAL)
            return shud_fail(SHUD_ERR_UNSUPPORTED, "lakes: the OMP path has no lake physics (MD_f_omp.cpp)");
        T.NL = m->num_lake;
        if (T.NL <= 0 || !m->lake_bathy_off || !m->lake_bathy_y || !m->lake_bathy_a)
            return shud_fail(SHUD_ERR_ARG, "lake elements present but no lake bathymetry (num_lake %d)", m->num_lake);
        for (int l = 0; l < T.NL; l++)
            if (m->lake_bathy_off[l + 1] <= m->lake_bathy_off[l])
                return shud_fail(SHUD_ERR_ARG, "lake %d has an empty bathymetry table", l + 1);
        for (int i = 0; i < NE; i++)
            if (m->ilake[i] > T.NL) return shud_fail(SHUD_ERR_ARG, "element %d: iLake %d > num_lake", i, m->ilake[i]);
    }
    for (int r = 0; r < NR; r++) {
        int d = m->riv_down[r];
        if (T.lakeon && d <= -4) {               // toLake = (-3 - down) - 1 (MD_Lake.cpp:46-50)
            if ((-3 - d) - 1 >= T.NL)
                return shud_fail(SHUD_ERR_ARG, "reach %d flows into lake %d > num_lake", r, -3 - d);
            continue;
        }
        if (d >= NR || (d < 0 && d < -4))
            return shud_fail(SHUD_ERR_ARG, "Fatal Error: River Routing Boundary Condition Type Is Wrong! (reach %d down %d)", r, d);
    }
    for (int s = 0; s < NS; s++)
        if (m->seg_ele[s] < 0 || m->seg_ele[s] >= NE || m->seg_riv[s] < 0 || m->seg_riv[s] >= NR)
            return shud_fail(SHUD_ERR_ARG, "segment %d references element/reach out of range", s);
    return 0;
}

// packed element flags, BC columns and their maxima
int flag_tables(const ShudMeshSoA *m, MeshTables &T) {
    const int NE = m->num_ele, NR = m->num_riv;
    T.eflags.resize(NE);
    for (int i = 0; i < NE; i++) {
        int ibc = m->ibc ? m->ibc[i] : 0, iss = m->iss ? m->iss[i] : 0;
        if (ibc < -32768 || ibc > 32767) return shud_fail(SHUD_ERR_ARG, "iBC out of range at %d", i);
        T.eflags[i] = (ibc & 0xffff) | ((iss > 0 ? 1 : iss < 0 ? 2 : 0) << 16);
        int &mx = T.max_col[ibc < 0 ? 1 : 0];              // a positive column reads eyBC, a negative one eqBC
        mx = std::max(mx, std::abs(ibc));
    }
    T.riv_bc.assign(NR, 0);
    for (int r = 0; r < NR; r++) {
        const int bc = T.riv_bc[r] = m->riv_bc ? m->riv_bc[r] : 0;
        int &mx = T.max_col[bc < 0 ? 3 : 2];               // ryBC, rqBC
        mx = std::max(mx, std::abs(bc));
    }
    return 0;
}

// segment CSR by element (stable: ascending reference index inside an element), and the interior prefix n_int
int segment_tables(const ShudMeshSoA *m, const ShudPartition *part, MeshTables &T) {
    const int NE = m->num_ele, NS = m->num_seg;
    group_by(NS, NE, [&](int s) { return m->seg_ele[s]; }, T.seg_off, T.seg_perm);
    T.seg_riv.resize(NS); T.seg_len.resize(NS); T.seg_cwr.resize(NS);
    for (int k = 0; k < NS; k++) {
        const int s = T.seg_perm[k];
        T.seg_riv[k] = m->seg_riv[s];
        T.seg_len[k] = m->seg_length[s];
        T.seg_cwr[k] = m->seg_cwr[s];
    }
    // only elements < ncomp compute their segments; segments of pure ghosts must not be needed
    const int ncomp = T.n_own + T.n_segghost;
    for (int s = 0; s < NS; s++)
        if (m->seg_ele[s] >= ncomp && m->seg_riv[s] < T.n_own_riv)
            return shud_fail(SHUD_ERR_ARG, "segment %d of an owned reach belongs to a non-computed ghost element", s);
    // partitioned: owned elements [0, n_int) read no ghost data (all lateral neighbours owned, all their
    // segments' reaches owned); they run while the halo exchange is in flight (eval_device)
    if (part) {
        int i = 0;
        for (; i < T.n_own; i++) {
            bool dep = false;
            for (int j = 0; j < 3 && !dep; j++) dep = m->nabr[(size_t)j * NE + i] >= T.n_own;
            for (int k = T.seg_off[i]; k < T.seg_off[i + 1] && !dep; k++) dep = T.seg_riv[k] >= T.n_own_riv;
            if (dep) break;
        }
        T.n_int = i;
    }
    return 0;
}

// per reach: its segments (ascending reference order), its upstream reaches, its downstream code
void reach_tables(const ShudMeshSoA *m, const ShudPartition *part, MeshTables &T) {
    const int NR = m->num_riv, NS = m->num_seg, nor = T.n_own_riv;
    std::vector<int> by_reach, pos_of(NS);
    group_by(NS, NR, [&](int s) { return m->seg_riv[s]; }, T.reach_off, by_reach);
    for (int k = 0; k < NS; k++) pos_of[T.seg_perm[k]] = k;
    // the owned reaches' segments as element-sorted positions; the river kernel may read a whole 8-position batch
    // past the end
    T.rseg_pos.assign((size_t)T.reach_off[nor] + 8, 0);
    for (int q = 0; q < T.reach_off[nor]; q++) T.rseg_pos[q] = pos_of[by_reach[q]];
    // ascending reach order (MD_f.cpp:236-240); in a partition, ascending GLOBAL reach id
    group_by(NR, nor, [&](int r) { return m->riv_down[r] < nor ? m->riv_down[r] : -1; }, T.up_off, T.up_idx);
    if (part && part->riv_gid)
        sort_groups(T.up_off, T.up_idx, [&](int a, int b) { return part->riv_gid[a] < part->riv_gid[b]; });
    // reach codes as the kernels see them: a reach into a lake uses the zero-depth-gradient formula (-3)
    T.riv_down.assign(m->riv_down, m->riv_down + NR);
    if (T.lakeon)
        for (int r = 0; r < NR; r++)
            if (T.riv_down[r] <= -4) T.riv_down[r] = -3;
}

// Segments per batch in the river kernel: a wave issues SB flux gathers + its position loads per batch and runs
// as many batches as its lane with the most segments needs; pick the batch size that issues fewer loads over the
// owned reaches' 64-reach waves (6 or 8: 16-B + 8-B or two 16-B position loads)
int choose_riv_sb(const int *reach_off, int nr) {
    long long cost6 = 0, cost8 = 0;
    for (int w = 0; w < nr; w += 64) {
        int mx = 0;
        for (int r = w; r < nr && r < w + 64; r++) mx = std::max(mx, reach_off[r + 1] - reach_off[r]);
        cost6 += (long long)((mx + 5) / 6) * (6 + 2);
        cost8 += (long long)((mx + 7) / 8) * (8 + 2);
    }
    return cost6 < cost8 ? 6 : 8;
}

// Identities the packed records rely on; a mesh without them takes the SoA kernel.
bool packed_qualifies(const ShudMeshSoA *m, const ShudParamsSoA *p, const MeshTables &T) {
    if (!env_knob("SHUD_RHS_PACKED", 1, 0, 1)) return false;     // 0: the SoA kernel (tests, A/B)
    const int NE = m->num_ele, NR = m->num_riv;
    if (!m->rough || NE == 0) return false;
    // avgRough must be the reference's 0.5*(Rough_i + Rough_nabr) / Rough_i (Element.cpp:249-265).  Owned
    // elements only: a ghost never computes lateral fluxes, and its neighbours outside the rank's local mesh
    // appear as boundary edges (-1) while its avgRough is the global one
    for (int j = 0; j < 3; j++)
        for (int i = 0; i < T.n_own; i++) {
            const int nb = m->nabr[(size_t)j * NE + i];
            const double want = nb >= 0 ? 0.5 * (m->rough[i] + m->rough[nb]) : m->rough[i];
            if (!(m->avg_rough[(size_t)j * NE + i] == want)) return false;
        }
    // the packed kernel addresses its element / segment streams with 32-bit byte offsets (at(), shud_ele_packed.hip)
    if ((uint64_t)48 * NE >= (1ull << 32) || (uint64_t)48 * m->num_seg >= (1ull << 32) ||
        (uint64_t)24 * NE + 8ull * NR >= (1ull << 32))
        return false;
    for (int r = 0; r < NR; r++)                                   // 16-bit segment count in the reach index word
        if (T.reach_off[r + 1] - T.reach_off[r] > 0xffff) return false;
    // AquiferDepth == z_surf - z_bottom (InitElement after rmSinks, Model_Data.cpp:262-264), |iBC| fits int8,
    // <= 63 segments per element
    for (int i = 0; i < NE; i++) {
        if (!(p->aquifer_depth[i] == m->z_surf[i] - m->z_bottom[i])) return false;
        const int ibc = (int16_t)(T.eflags[i] & 0xffff);
        if (ibc > 127 || ibc < -127) return false;
        if (T.seg_off[i + 1] - T.seg_off[i] > 63) return false;
    }
    return true;
}

// Distinct fixed-length tuples of 64-bit words (bit patterns: two doubles are the same key when their bits are), each
// numbered in first-seen order: open addressing over a power-of-two slot table, the tuples stored flat.  The class
// search below runs it over every element several times per handle (one pass per candidate hybrid field set), so it
// avoids per-element heap keys (std::string keys of 144 B cost seconds at 10M elements).
class TupleSet {
  public:
    explicit TupleSet(int k) : k_(k), slots_(1024, -1) {}     // k <= 32
    int size() const { return (int)(words_.size() / k_); }
    const uint64_t *tuple(int id) const { return &words_[(size_t)id * k_]; }
    // id of the tuple at p (k 8-byte words, any type: copied as bits), inserted if new
    int insert(const void *p) {
        uint64_t t[32];
        memcpy(t, p, (size_t)k_ * 8);
        if ((size_t)(size() + 1) * 2 > slots_.size()) grow();
        size_t j = hash(t) & (slots_.size() - 1);
        for (;; j = (j + 1) & (slots_.size() - 1)) {
            const int id = slots_[j];
            if (id < 0) break;
            if (!memcmp(tuple(id), t, (size_t)k_ * 8)) return id;
        }
        const int id = size();
        slots_[j] = id;
        words_.insert(words_.end(), t, t + k_);
        return id;
    }

  private:
    uint64_t hash(const uint64_t *t) const {
        uint64_t h = 0x9e3779b97f4a7c15ull;
        for (int q = 0; q < k_; q++) {                  // splitmix64 finaliser per word, chained
            uint64_t x = t[q] + h;
            x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
            x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
            h = x ^ (x >> 31);
        }
        return h;
    }
    void grow() {
        std::vector<int> old;
        old.swap(slots_);
        slots_.assign(old.size() * 2, -1);
        for (int id : old) {
            if (id < 0) continue;
            size_t j = hash(tuple(id)) & (slots_.size() - 1);
            while (slots_[j] >= 0) j = (j + 1) & (slots_.size() - 1);
            slots_[j] = id;
        }
    }
    int k_;
    std::vector<int> slots_;
    std::vector<uint64_t> words_;
};

// the primary class fields of element i, with the fields in `mask` zeroed
void primary_fields(const ShudMeshSoA *m, const ShudParamsSoA *p, int i, uint32_t mask, double *r) {
    r[CF_macD] = p->macD[i]; r[CF_macKsatH] = p->macKsatH[i]; r[CF_vAreaF] = p->geo_vAreaF[i];
    r[CF_KsatH] = p->KsatH[i]; r[CF_KsatV] = p->KsatV[i]; r[CF_infKsatV] = p->infKsatV[i];
    r[CF_hAreaF] = p->hAreaF[i]; r[CF_macKsatV] = p->macKsatV[i]; r[CF_ThetaS] = p->ThetaS[i];
    r[CF_ThetaR] = p->ThetaR[i]; r[CF_Beta] = p->Beta[i]; r[CF_infD] = p->infD[i]; r[CF_Sy] = p->Sy[i];
    r[CF_RzD] = p->RzD[i]; r[CF_VegFrac] = p->VegFrac[i]; r[CF_ImpAF] = p->ImpAF[i];
    r[CF_depression] = m->depression ? m->depression[i] : 0.0002;
    r[CF_rough] = m->rough[i];
    for (int f = 0; f < CF_NPRIMARY; f++)
        if (mask >> f & 1) r[f] = 0.;
}

// Distinct parameter tuples -> class ids: cls [NE], table [class][field], and the streamed fields hmask of the hybrid
// layout (0: none).  False when no class table fits.
bool class_search(const ShudMeshSoA *m, const ShudParamsSoA *p, bool lakeon, std::vector<int> &cls,
                  std::vector<std::vector<double>> &table, uint32_t &hmask) {
    const int NE = m->num_ele;
    cls.resize(NE);
    std::vector<double> r(CF_NPRIMARY);
    // the distinct tuples of the fields outside `mask`, counting stops past `cap`
    auto count_tuples = [&](uint32_t mask, int cap) {
        TupleSet seen(CF_NPRIMARY);
        for (int i = 0; i < NE && seen.size() <= cap; i++) {
            primary_fields(m, p, i, mask, r.data());
            seen.insert(r.data());
        }
        return seen.size();
    };
    // classes of the fields outside `mask`; false past 32768 classes
    auto build_classes = [&](uint32_t mask) {
        table.clear();
        TupleSet ids(CF_NPRIMARY);
        for (int i = 0; i < NE; i++) {
            primary_fields(m, p, i, mask, r.data());
            const int id = ids.insert(r.data());
            if (id == (int)table.size()) {
                if (id >= 32768) return false;
                table.push_back(r);
            }
            cls[i] = id;
        }
        return true;
    };
    const bool fits = build_classes(0);
    // Hybrid layout (per-element-calibrated models): when the full tuples exceed one workgroup's LDS table, stream up
    // to kHybMax fields per element (8 B each) and keep the rest in the LDS class table — the fields that split the
    // classes of the non-streamable fields the most first, among those the kernel reads directly (no host-derived
    // class constant depends on them; Sy's reciprocal is replaced by the IEEE division, the same bits).
    // SHUD_RHS_HYB=0: off (A/B); =2: KsatH streamed even when the classes fit (timing the hybrid path on any model).
    hmask = 0;
    const int hyb = env_knob("SHUD_RHS_HYB", 1, 0, 2);
    if (hyb == 2 && !lakeon) {
        hmask = 1u << CF_KsatH;
    } else {
        const uint32_t streamable = 1u << CF_macD | 1u << CF_macKsatH | 1u << CF_vAreaF | 1u << CF_KsatH |
                                    1u << CF_KsatV | 1u << CF_Sy | 1u << CF_RzD | 1u << CF_depression | 1u << CF_rough;
        if (!lakeon && hyb != 0 && (!fits || (int)table.size() > kLdsClassMax) &&
            count_tuples(streamable, kLdsClassMax) <= kLdsClassMax) {
            // base classes: the tuples of the fields that cannot be streamed; then, per streamable field, how many
            // (base class, value) pairs it makes — the fields that split the base classes most are streamed first
            TupleSet bid(CF_NPRIMARY);
            std::vector<int> base(NE);
            for (int i = 0; i < NE; i++) {
                primary_fields(m, p, i, streamable, r.data());
                base[i] = bid.insert(r.data());
            }
            std::vector<std::pair<size_t, int>> split;       // (distinct (base, value) pairs, field)
            for (int f = 0; f < CF_NPRIMARY; f++) {
                if (!(streamable >> f & 1)) continue;
                TupleSet pairs(2);                           // (base class, field value bits)
                for (int i = 0; i < NE && pairs.size() <= 1 << 20; i++) {
                    primary_fields(m, p, i, 0, r.data());
                    uint64_t key[2];
                    key[0] = (uint64_t)base[i];
                    memcpy(&key[1], &r[f], 8);
                    pairs.insert(key);
                }
                if (pairs.size() > bid.size()) split.push_back({(size_t)pairs.size(), f});
            }
            std::stable_sort(split.begin(), split.end(),
                             [](const std::pair<size_t, int> &a, const std::pair<size_t, int> &b) {
                                 return a.first > b.first;
                             });
            for (int k = 0; k < (int)split.size() && k < kHybMax; k++) {
                hmask |= 1u << split[k].second;
                if (count_tuples(hmask, kLdsClassMax) <= kLdsClassMax) break;
                if (k + 1 == kHybMax || k + 1 == (int)split.size()) hmask = 0;   // not enough: no hybrid layout
            }
        }
    }
    return hmask ? build_classes(hmask) : fits;
}

// The class table as the kernel stages it: the stored fields of every class, the derived ones computed here, then
// pow_tab's tables.  False when a class needs the SoA kernel's full pow or plain divisions, or the table is too long.
bool class_table(std::vector<std::vector<double>> &table, PackedTables &P) {
    const int ncls = (int)table.size();
    // beyond what a 256-thread workgroup's LDS copy holds (128 classes) the class table goes to 1024-thread
    // workgroups (up to kLdsClassMaxBig = 600 classes, one per CU); beyond that the lookups would be dependent
    // L2 trips.  Measured on syn-10M (tools/class_sweep.py, profiles/r02/class_sweep.log): element kernel 0.65 ms
    // with 33 classes in LDS; from L2 0.83 ms at 132 classes, 1.21 at 495, 1.49 at 1,980, 1.66 at 13,200; the
    // SoA kernel 1.09 ms at any count -> SoA above 600 (SHUD_RHS_L2_CLASS=1 forces the L2 table at any count and
    // disables the 1024-thread LDS kernel, =0 forces SoA above 128: A/B and bench.py many_class)
    const int l2 = env_knob("SHUD_RHS_L2_CLASS", -1, 0, 1);
    const int l2_max = l2 == 1 ? 32768 : l2 == 0 ? kLdsClassMax : kLdsClassMaxBig;
    if (ncls > l2_max) return false;
    P.dp.lds_big = l2 == 1 ? 0 : 1;
    std::vector<double> &ctab = P.ctab;
    ctab.assign((size_t)CF_STRIDE * ncls, 0.0);
    for (int c = 0; c < ncls; c++) {
        std::vector<double> &t = table[c];
        t.resize(CF_COUNT);
        // same expressions, same order as the element kernel (-ffp-contract=off on both sides)
        t[CF_fcmr] = t[CF_ThetaS] * 0.75 - t[CF_ThetaR];
        t[CF_dTh] = t[CF_ThetaS] - t[CF_ThetaR];
        t[CF_ex1] = t[CF_Beta] / (t[CF_Beta] - 1.);
        t[CF_ex2] = (t[CF_Beta] - 1.) / t[CF_Beta];
        // the packed kernel's satKfun uses pow_tab (positive bases, finite exponents: shud_physics.h);
        // any other Beta keeps the SoA layout, whose kernel calls the full pow for it
        if (!(t[CF_Beta] > 1.) || !std::isfinite(t[CF_ex1]) || !std::isfinite(t[CF_ex2])) return false;
        t[CF_pj] = 1. - t[CF_ImpAF];
        t[CF_omh] = 1. - t[CF_hAreaF];
        t[CF_kmax] = t[CF_infKsatV] * (1. - t[CF_hAreaF]) + t[CF_macKsatV] * t[CF_hAreaF];
        t[CF_ekA] = t[CF_infKsatV] * (1. - t[CF_hAreaF]);
        t[CF_ekB] = t[CF_hAreaF] * t[CF_macKsatV];
        // cdiv's range (shud_dev.h cdiv_divisor_ok); otherwise plain divisions in the SoA kernel
        if (!cdiv_divisor_ok(t[CF_fcmr]) || !cdiv_divisor_ok(t[CF_dTh]) || !cdiv_divisor_ok(t[CF_infD]) ||
            !cdiv_divisor_ok(t[CF_Sy]))
            return false;
        t[CF_r_fcmr] = 1. / t[CF_fcmr];
        t[CF_r_dTh] = 1. / t[CF_dTh];
        t[CF_r_infD] = 1. / t[CF_infD];
        t[CF_r_Sy] = 1. / t[CF_Sy];
        for (int f = 0; f < CF_COUNT; f++)
            if (cf_stored(f)) ctab[(size_t)c * CF_STRIDE + cf_pos(f)] = t[f];
    }
    // pow_tab's tables (shud_pow_tab.h) after the class table, 16-B aligned: one buffer, one LDS copy per workgroup
    const int pt_off = ((int)ctab.size() + 1) & ~1;
    ctab.resize((size_t)pt_off + kPowTabDoubles, 0.0);
#if SHUD_PT_COMPACT
    static_assert(sizeof shud_pt_clogtab == 8 * kPowTabLogDoubles, "pow_tab");
    memcpy(&ctab[pt_off], shud_pt_clogtab, sizeof shud_pt_clogtab);
#else
    static_assert(kPowTabLogDoubles == 4 * SHUD_PT_LOG_N && sizeof shud_pt_logtab == 8 * kPowTabLogDoubles, "pow_tab");
    memcpy(&ctab[pt_off], shud_pt_logtab, sizeof shud_pt_logtab);
#endif
    static_assert(kPowTabDoubles == kPowTabLogDoubles + 2 * SHUD_PT_EXP_N, "pow_tab table size");
    memcpy(&ctab[pt_off + kPowTabLogDoubles], shud_pt_exptab, sizeof shud_pt_exptab);
    P.dp.ncls = ncls; P.dp.pt_off = pt_off; P.dp.ntab = (int)ctab.size();
    return true;
}

struct SharePlan {                     // per element of [0, lim)
    std::vector<signed char> pub, rcv;             // the slot it publishes / receives, -1: none
    std::vector<std::array<signed char, 3>> e;     // the reference slot evaluated first, second, last
};
// In-tile edge sharing (shud_ele_packed.hip, SH) over elements [0, lim).  An interior edge between two elements of one 256-element tile whose fluxes are exactly antisymmetric (same edge
// length and Dist2Nabor bits from both sides, same depression, positive finite avgRough, neither a lake element) is
// evaluated by one of them and read by the other from LDS.  Greedy in element order: every element publishes at most
// one edge and receives at most one, never both directions of one edge.
SharePlan share_plan(const ShudMeshSoA *m, int lim) {
    const int NE = m->num_ele;
    SharePlan sp;
    sp.pub.assign(lim, -1); sp.rcv.assign(lim, -1); sp.e.resize(lim);
    std::vector<signed char> &pub = sp.pub, &rcv = sp.rcv;
    for (int i = 0; i < lim; i++) {
        for (int k = 0; k < 3 && rcv[i] < 0; k++) {
            const int v = m->nabr[(size_t)k * NE + i];
            if (v < 0 || v >= lim || v == i || (v / kShareTile) != (i / kShareTile) || pub[v] >= 0) continue;
            int kk = -1, hits = 0;
            for (int q = 0; q < 3; q++)
                if (m->nabr[(size_t)q * NE + v] == i) { kk = q; hits++; }
            if (hits != 1 || pub[i] == k) continue;
            const size_t a = (size_t)k * NE + i, b = (size_t)kk * NE + v;
            const double ar = m->avg_rough[a];
            if (memcmp(&m->edge[a], &m->edge[b], 8) || memcmp(&m->dist2nabor[a], &m->dist2nabor[b], 8) ||
                (m->depression && memcmp(&m->depression[i], &m->depression[v], 8)) ||   // NULL: 0.0002 everywhere
                memcmp(&ar, &m->avg_rough[b], 8) ||
                !(ar > 0. && std::isfinite(ar)) || lake_ele(m, i) || lake_ele(m, v))
                continue;
            pub[v] = (signed char)kk;
            rcv[i] = (signed char)k;
        }
    }
    // The evaluation order (shud_dev.h kEvoShift): first the published slot (else the lowest slot that is not the
    // received one), last the received slot (else the highest remaining one).
    for (int i = 0; i < lim; i++) {
        const int p = pub[i], r = rcv[i];
        const int e0 = p >= 0 ? p : (r == 0 ? 1 : 0), e2 = r >= 0 ? r : (e0 == 2 ? 1 : 2);
        sp.e[i] = {(signed char)e0, (signed char)(3 - e0 - e2), (signed char)e2};
    }
    return sp;
}

// The 16-byte element, segment and reach records of DevPacked and its remaining scalars.
void packed_records(const ShudMeshSoA *m, const ShudParamsSoA *p, const MeshTables &T, const std::vector<int> &cls,
                    uint32_t hmask, PackedTables &P) {
    const int NE = m->num_ele, NR = m->num_riv, NS = m->num_seg, nor = T.n_own_riv;
    // Sharing covers elements [0, lim): a single-GPU handle's all, a partitioned handle's interior prefix (its
    // ghost-free launch tiles from element 0); the instantiations without sharing that can run on such a handle
    // (diagnostics, ghosts) evaluate every edge themselves and only decode the order.
    // Only for handles that take the LSP instantiations (class + pow tables small enough, no lakes, no hybrid
    // layout): the other instantiations read seg_first with a 31-bit mask (shud_ele_packed.hip ele_body).
    const int lim = T.n_int > 0 ? T.n_int : (T.n_own == NE ? NE : 0);
    SharePlan sp;
    if (lim > 1 && !hmask && !T.lakeon && lsp_lds_bytes((int)P.ctab.size()) <= kLspLdsMax && NS < (1 << 26) &&
        env_knob("SHUD_RHS_SHARE", 1, 0, 1))
        sp = share_plan(m, lim);
    P.n_shared = (int)std::count_if(sp.rcv.begin(), sp.rcv.end(), [](signed char r) { return r >= 0; });
    // meta's neighbours and the ged planes are stored in evaluation order, so every pass of the sharing kernel reads
    // one plane, coalesced, with a literal slot; every other reader goes back through evo_stored().  seg_first bits
    // 26-30 carry the order; an element outside the plan keeps the reference order and zero bits.
    P.zz.resize(NE); P.meta.resize(NE); P.ged.resize(3 * (size_t)NE); P.seg_first.resize(NE);
    for (int i = 0; i < NE; i++) {
        P.zz[i] = make_double2(m->z_surf[i], m->z_bottom[i]);
        const int nseg = T.seg_off[i + 1] - T.seg_off[i];
        const unsigned cf = (unsigned)(T.eflags[i] & 0xff) | ((unsigned)((T.eflags[i] >> 16) & 3) << 8) |
                            ((unsigned)nseg << 10) | ((unsigned)cls[i] << 16) | (lake_ele(m, i) ? 0x80000000u : 0u);
        int e[3] = {0, 1, 2};
        unsigned evo = 0;
        if (i < (int)sp.e.size()) {
            for (int s = 0; s < 3; s++) e[s] = sp.e[i][s];
            evo = (evo_encode(e) << kEvoShift) | (sp.pub[i] >= 0 ? kEvoPub0 : 0u) | (sp.rcv[i] >= 0 ? kEvoRcv2 : 0u);
        }
        P.meta[i] = make_int4(m->nabr[(size_t)e[0] * NE + i], m->nabr[(size_t)e[1] * NE + i],
                              m->nabr[(size_t)e[2] * NE + i], (int)cf);
        for (int s = 0; s < 3; s++)
            P.ged[(size_t)s * NE + i] =
                make_double2(m->edge[(size_t)e[s] * NE + i], m->dist2nabor[(size_t)e[s] * NE + i]);
        P.seg_first[i] = T.seg_off[i] | (int)evo;
    }
    DevPacked &D = P.dp;
    if (hmask) {                                                     // the streamed fields, per element
        for (int f = 0; f < CF_NPRIMARY; f++)
            if (hmask >> f & 1) D.hslot1[f] = (signed char)++D.nh;
        D.hs = D.nh == 1 ? 1 : D.nh == 2 ? 2 : 4;
        P.hv.assign((size_t)D.hs * NE, 0.0);
        double rr[CF_NPRIMARY];
        for (int i = 0; i < NE; i++) {
            primary_fields(m, p, i, 0, rr);
            for (int f = 0; f < CF_NPRIMARY; f++)
                if (D.hslot1[f]) P.hv[(size_t)D.hs * i + D.hslot1[f] - 1] = rr[f];
        }
        D.hnb = (hmask & (1u << CF_macD | 1u << CF_macKsatH | 1u << CF_vAreaF | 1u << CF_KsatH | 1u << CF_rough)) != 0;
    }
    // element-sorted segments {length, Cwr} (their reach: MeshTables::seg_riv); per reach one 32-B record with the
    // statics the segment fluxes read, one 64-B record of its own, and its index word rv_u (shud_dev.h)
    P.sg_lc.resize(NS);
    for (int k = 0; k < NS; k++) P.sg_lc[k] = make_double2(T.seg_len[k], T.seg_cwr[k]);
    P.rrec.resize(2 * (size_t)NR); P.rv.resize(4 * (size_t)NR); P.rv_u.resize(NR);
    auto int_pair = [](int32_t a, int32_t b) {                       // two ints in the bits of one double
        const int32_t two[2] = {a, b}; double bits; memcpy(&bits, two, sizeof bits); return bits;
    };
    for (int r = 0; r < NR; r++) {
        P.rrec[2 * (size_t)r] = make_double2(m->riv_depth[r], m->riv_ksath[r]);
        P.rrec[2 * (size_t)r + 1] = make_double2(m->riv_bedthick[r], int_pair(T.riv_bc[r], 0));
        P.rv[4 * (size_t)r + 0] = make_double2(m->riv_bottom_width[r], m->riv_bankslope[r]);
        P.rv[4 * (size_t)r + 1] = make_double2(m->riv_length[r], m->riv_bed_slope[r]);
        P.rv[4 * (size_t)r + 2] = make_double2(m->riv_dist2down[r], m->riv_avg_rough[r]);
        P.rv[4 * (size_t)r + 3] = make_double2(m->riv_depth[r], int_pair(T.riv_down[r], T.riv_bc[r]));
        const int cnt = T.reach_off[r + 1] - T.reach_off[r], start = cnt ? T.reach_off[r] : 0;
        int4 u = make_int4(start, cnt, 0, 0);                        // ghosts: segments only
        if (r < nor) {
            const int o = T.up_off[r], n = T.up_off[r + 1] - o;
            u = n <= 2 ? make_int4(start, cnt | (n << 16), n > 0 ? T.up_idx[o] : 0, n > 1 ? T.up_idx[o + 1] : 0)
                       : make_int4(start, cnt | (3 << 16), o, n);
        }
        P.rv_u[r] = u;
    }
    D.riv_sb = choose_riv_sb(T.reach_off.data(), nor);
    if (const int sb = env_knob("SHUD_RIV_SB", 0, 6, 8); sb == 6 || sb == 8) D.riv_sb = sb;   // tests: both batch sizes
    // QrivDown pre-pass slots (shud_dev.h DevPacked::qdown); SHUD_RHS_QD=0: the river kernel recomputes (tests, A/B)
    if (NR > 0 && env_knob("SHUD_RHS_QD", 1, 0, 1)) D.nqd = NR;
    D.qd_pm = env_knob("SHUD_QD_POS", 1000, 0, 1000);
    D.qd_pm_fold = env_knob("SHUD_QD_POS_FOLD", 1000, 0, 1000);
}

// Lakes: lake / bank-edge / inflow lists in the reference's summation orders.
int lake_tables(const ShudMeshSoA *m, const ShudPartition *part, const HostTables &H, LakeTables &L) {
    const int NE = m->num_ele, NR = m->num_riv, NL = H.mesh.NL;
    const int NO = H.mesh.n_own;               // lake and bank elements are owned (partition plan)
    if (!H.packed)
        return shud_fail(SHUD_ERR_UNSUPPORTED, "lakes need the packed layout (mesh did not qualify or SHUD_RHS_PACKED=0)");
    if (H.pk.dp.ncls > 128) return shud_fail(SHUD_ERR_UNSUPPORTED, "lakes: more than 128 parameter classes");
    L.lake_of.assign(NE, -1);
    for (int i = 0; i < NE; i++) {
        if (!lake_ele(m, i)) continue;
        if (i >= NO) return shud_fail(SHUD_ERR_ARG, "lake element %d is a ghost (partition splits a lake group)", i);
        L.lake_of[i] = m->ilake[i] - 1;
    }
    group_by(NE, NL, [&](int i) { return L.lake_of[i]; }, L.ele_off, L.ele_idx);
    // bank edges: a non-lake element's edge whose neighbour is a lake element (lakenabr, MD_Lake.cpp:131-143);
    // ascending element, then edge: the reference's order (item 3 i + j, stored as pos = j * NE + i)
    auto bank_lake = [&](int q) -> int {
        const int i = q / 3, nb = m->nabr[(size_t)(q % 3) * NE + i];
        return i < NO && !lake_ele(m, i) && nb >= 0 ? L.lake_of[nb] : -1;
    };
    group_by(3 * NE, NL, bank_lake, L.bank_off, L.bank_pos);
    for (int &q : L.bank_pos) q = (q % 3) * NE + q / 3;
    group_by(NR, NL, [&](int r) { return m->riv_down[r] <= -4 ? (-3 - m->riv_down[r]) - 1 : -1; }, L.rin_off, L.rin_idx);
    // partitioned: local order is [interior | boundary | ghosts] / [owned | ghosts], so put every lake list in
    // global order (the single-GPU summation order, hence bit-identical sums)
    if (part && part->ele_gid && part->riv_gid) {
        const int32_t *eg = part->ele_gid, *rg = part->riv_gid;
        sort_groups(L.ele_off, L.ele_idx, [&](int a, int b) { return eg[a] < eg[b]; });
        sort_groups(L.bank_off, L.bank_pos, [&](int a, int b) {
            const int ia = a % NE, ib = b % NE;                     // pos = j*NE + i: element, then edge
            return eg[ia] != eg[ib] ? eg[ia] < eg[ib] : a / NE < b / NE;
        });
        sort_groups(L.rin_off, L.rin_idx, [&](int a, int b) { return rg[a] < rg[b]; });
    }
    for (int l = 0; l < NL; l++)
        if (L.ele_off[l + 1] == L.ele_off[l]) return shud_fail(SHUD_ERR_ARG, "lake %d has no lake element", l + 1);
    return 0;
}

}  // namespace

int shud::build_tables(const ShudMeshSoA *m, const ShudParamsSoA *p, const ShudRhsOptions *opt,
                       const ShudPartition *part, HostTables *out) {
    MeshTables &T = out->mesh;
    int rc;
    if ((rc = validate(m, p, opt, part, T)) || (rc = flag_tables(m, T)) || (rc = segment_tables(m, part, T))) return rc;
    reach_tables(m, part, T);
    std::vector<int> cls;
    std::vector<std::vector<double>> table;           // [class][field]
    uint32_t hmask = 0;
    out->packed = packed_qualifies(m, p, T) && class_search(m, p, T.lakeon, cls, table, hmask) &&
                  class_table(table, out->pk);
    if (out->packed) packed_records(m, p, T, cls, hmask, out->pk);
    return T.lakeon ? lake_tables(m, part, *out, out->lake) : 0;
}

extern "C" int shud_rhs_plan_layout(const ShudMeshSoA *mesh, const ShudParamsSoA *par, const ShudRhsOptions *opt,
                                    const ShudPartition *part, ShudLayoutInfo *info, int32_t *edge_plan,
                                    int32_t *stored_nabr) {
    if (!mesh || !par || !info) return shud_fail(SHUD_ERR_ARG, "null argument");
    HostTables H;
    if (const int rc = build_tables(mesh, par, opt, part, &H)) return rc;
    const PackedTables &P = H.pk;
    *info = ShudLayoutInfo{H.packed ? 1 : 0, H.packed ? P.dp.ncls : 0, H.packed ? P.dp.nh : 0,
                           H.packed ? P.n_shared : 0, H.mesh.n_int, H.packed ? P.dp.riv_sb : 0};
    const size_t NE = (size_t)mesh->num_ele;
    for (size_t i = 0; i < NE; i++) {
        if (edge_plan) edge_plan[i] = H.packed ? (P.seg_first[i] >> kEvoShift) & 31 : 0;
        if (!stored_nabr) continue;
        const int nb[3] = {H.packed ? P.meta[i].x : mesh->nabr[i], H.packed ? P.meta[i].y : mesh->nabr[NE + i],
                           H.packed ? P.meta[i].z : mesh->nabr[2 * NE + i]};
        for (int s = 0; s < 3; s++) stored_nabr[s * NE + i] = nb[s];
    }
    return SHUD_OK;
}
