// shud_order.cpp — element locality ordering without a device (include/shud_order.h): the planner, the appliers
// that carry a model into the planned numbering, and the host gather for any other per-element array.
#include "shud_order.h"
#include "shud_dev.h"                              // kShareTile: the tile SHUD_ORDER_TILES fills is share_plan's

#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

int shud_fail(int code, const char *fmt, ...);    // shud_rhs.cpp

struct shud_ordered {
    std::vector<std::vector<int32_t>> iv;
    std::vector<std::vector<double>> dv;
};

static bool has_lakes(const ShudMeshSoA *m) {
    if (m->num_lake > 0) return true;
    if (m->ilake)
        for (int i = 0; i < m->num_ele; i++)
            if (m->ilake[i] > 0) return true;
    return false;
}

static int check_perm(const int32_t *p, int n) {
    std::vector<char> seen((size_t)std::max(n, 1), 0);
    for (int k = 0; k < n; k++) {
        if (p[k] < 0 || p[k] >= n || seen[p[k]]) return shud_fail(SHUD_ERR_ARG, "order: not a permutation at entry %d", k);
        seen[p[k]] = 1;
    }
    return SHUD_OK;
}

static int check_nabr(const ShudMeshSoA *m) {
    const size_t n3 = 3 * (size_t)m->num_ele;
    for (size_t k = 0; k < n3; k++)
        if (m->nabr[k] >= m->num_ele) return shud_fail(SHUD_ERR_ARG, "order: nabr[%zu] = %d out of range", k, m->nabr[k]);
    return SHUD_OK;
}

extern "C" int shud_order_plan(const ShudMeshSoA *m, int kind, const int32_t *user_perm, int32_t *perm) {
    if (!m || !perm || m->num_ele < 0) return shud_fail(SHUD_ERR_ARG, "null argument");
    const int NE = m->num_ele;
    if (kind == SHUD_ORDER_IDENTITY) {
        std::iota(perm, perm + NE, 0);
        return SHUD_OK;
    }
    if (kind == SHUD_ORDER_USER) {
        if (!user_perm) return shud_fail(SHUD_ERR_ARG, "SHUD_ORDER_USER without user_perm");
        int rc = check_perm(user_perm, NE);
        if (rc) return rc;
        std::copy(user_perm, user_perm + NE, perm);
        return SHUD_OK;
    }
    if (kind != SHUD_ORDER_BFS && kind != SHUD_ORDER_TILES)
        return shud_fail(SHUD_ERR_ARG, "unknown order kind %d", kind);
    if (!m->nabr) return shud_fail(SHUD_ERR_ARG, "null nabr");
    int rc = check_nabr(m);
    if (rc) return rc;
    // component starts in ascending (number of neighbours, index): a counting sort by degree is stable in index
    std::vector<int32_t> starts((size_t)NE);
    {
        int cnt[5] = {0, 0, 0, 0, 0};
        std::vector<unsigned char> deg((size_t)NE);
        for (int i = 0; i < NE; i++) {
            int d = 0;
            for (int j = 0; j < 3; j++) d += m->nabr[(size_t)j * NE + i] >= 0;
            deg[i] = (unsigned char)d;
            cnt[d + 1]++;
        }
        for (int d = 0; d < 4; d++) cnt[d + 1] += cnt[d];
        for (int i = 0; i < NE; i++) starts[cnt[deg[i]]++] = i;
    }
    std::vector<char> seen((size_t)std::max(NE, 1), 0);
    int head = 0, tail = 0;                        // perm itself is the FIFO: [head, tail) is queued
    if (kind == SHUD_ORDER_TILES) {
        // pockets of the same search, each capped at the room left in the sharing tile it starts in; a neighbour
        // met at the cap seeds a later pocket.  seen: 1 = placed, 2 = waiting in seeds (at most once, so NE slots)
        std::vector<int32_t> seeds((size_t)NE);
        int sh = 0, st = 0, si = 0;
        while (tail < NE) {
            int r = -1;
            while (sh < st && r < 0) {
                const int v = seeds[sh++];
                if (seen[v] != 1) r = v;
            }
            while (r < 0) {
                const int v = starts[si++];
                if (seen[v] != 1) r = v;
            }
            const int end = tail + (shud::kShareTile - tail % shud::kShareTile);   // one past the pocket's last slot
            seen[r] = 1;
            perm[tail++] = r;
            while (head < tail) {
                const int i = perm[head++];
                for (int j = 0; j < 3; j++) {
                    const int v = m->nabr[(size_t)j * NE + i];
                    if (v < 0 || seen[v] == 1) continue;
                    if (tail < end) {
                        seen[v] = 1;
                        perm[tail++] = v;
                    } else if (!seen[v]) {
                        seen[v] = 2;
                        seeds[st++] = v;
                    }
                }
            }
        }
        return SHUD_OK;
    }
    for (int s = 0; s < NE; s++) {
        const int r = starts[s];
        if (seen[r]) continue;
        seen[r] = 1;
        perm[tail++] = r;
        while (head < tail) {
            const int i = perm[head++];
            for (int j = 0; j < 3; j++) {
                const int v = m->nabr[(size_t)j * NE + i];
                if (v >= 0 && !seen[v]) {
                    seen[v] = 1;
                    perm[tail++] = v;
                }
            }
        }
    }
    return SHUD_OK;
}

extern "C" int shud_order_gather_host(const int32_t *perm, int32_t n, size_t eb, int32_t planes, const void *src,
                                      void *dst) {
    if (!perm || !src || !dst || n < 0 || planes < 0 || eb == 0 || src == dst)
        return shud_fail(SHUD_ERR_ARG, "shud_order_gather_host: bad argument");
    const char *s = (const char *)src;
    char *d = (char *)dst;
    for (int p = 0; p < planes; p++) {
        const size_t base = (size_t)p * n;
        if (eb == 8) {
            const uint64_t *s8 = (const uint64_t *)src + base;
            uint64_t *d8 = (uint64_t *)dst + base;
            for (int k = 0; k < n; k++) d8[k] = s8[perm[k]];
        } else if (eb == 4) {
            const uint32_t *s4 = (const uint32_t *)src + base;
            uint32_t *d4 = (uint32_t *)dst + base;
            for (int k = 0; k < n; k++) d4[k] = s4[perm[k]];
        } else {
            for (int k = 0; k < n; k++) memcpy(d + (base + k) * eb, s + (base + (size_t)perm[k]) * eb, eb);
        }
    }
    return SHUD_OK;
}

extern "C" int shud_order_apply(const ShudMeshSoA *m, const ShudParamsSoA *par, const int32_t *perm,
                                shud_ordered_t *out, ShudMeshSoA *mo, ShudParamsSoA *po) {
    if (!m || !perm || !out || !mo || (par && !po)) return shud_fail(SHUD_ERR_ARG, "null argument");
    if (has_lakes(m)) return shud_fail(SHUD_ERR_UNSUPPORTED, "element ordering does not support lake models");
    const int NE = m->num_ele, NS = m->num_seg;
    int rc = check_perm(perm, NE);
    if (!rc && m->nabr) rc = check_nabr(m);
    if (rc) return rc;
    if (m->seg_ele)
        for (int s = 0; s < NS; s++)
            if (m->seg_ele[s] >= NE) return shud_fail(SHUD_ERR_ARG, "order: seg_ele[%d] out of range", s);
    shud_ordered *o = new shud_ordered();
    std::vector<int32_t> inv((size_t)NE);
    for (int k = 0; k < NE; k++) inv[perm[k]] = k;
    auto gd = [&](const double *src, int planes) -> const double * {
        if (!src) return nullptr;
        o->dv.emplace_back((size_t)planes * NE);
        for (int p = 0; p < planes; p++)
            for (int k = 0; k < NE; k++) o->dv.back()[(size_t)p * NE + k] = src[(size_t)p * NE + perm[k]];
        return o->dv.back().data();
    };
    auto gi = [&](const int32_t *src, int planes) -> const int32_t * {
        if (!src) return nullptr;
        o->iv.emplace_back((size_t)planes * NE);
        for (int p = 0; p < planes; p++)
            for (int k = 0; k < NE; k++) o->iv.back()[(size_t)p * NE + k] = src[(size_t)p * NE + perm[k]];
        return o->iv.back().data();
    };
    *mo = *m;                                       // reaches, segments (but seg_ele), lake tables, scalars: shared
    if (m->nabr) {
        int32_t *nb = const_cast<int32_t *>(gi(m->nabr, 3));
        for (size_t k = 0; k < 3 * (size_t)NE; k++)
            if (nb[k] >= 0) nb[k] = inv[nb[k]];
        mo->nabr = nb;
    }
    mo->area = gd(m->area, 1); mo->z_surf = gd(m->z_surf, 1); mo->z_bottom = gd(m->z_bottom, 1);
    mo->depression = gd(m->depression, 1); mo->rough = gd(m->rough, 1);
    mo->edge = gd(m->edge, 3); mo->dist2nabor = gd(m->dist2nabor, 3); mo->dist2edge = gd(m->dist2edge, 3);
    mo->avg_rough = gd(m->avg_rough, 3);
    mo->ibc = gi(m->ibc, 1); mo->iss = gi(m->iss, 1); mo->ilake = gi(m->ilake, 1);
    if (m->seg_ele) {
        o->iv.emplace_back((size_t)NS);
        for (int s = 0; s < NS; s++) o->iv.back()[s] = m->seg_ele[s] >= 0 ? inv[m->seg_ele[s]] : m->seg_ele[s];
        mo->seg_ele = o->iv.back().data();
    }
    if (par) {
        const double *const *src = (const double *const *)par;
        const double **dst = (const double **)po;
        for (size_t f = 0; f < sizeof(ShudParamsSoA) / sizeof(double *); f++) dst[f] = gd(src[f], 1);
    }
    *out = o;
    return SHUD_OK;
}

extern "C" int shud_order_free(shud_ordered_t o) {
    delete o;
    return SHUD_OK;
}
