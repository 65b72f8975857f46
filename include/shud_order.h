/*
 * shud_order.h — element locality ordering: a planner, appliers, and handles that run in an internal
 * element order while the caller keeps its own.
 *
 * The permutation is ELEMENT-ONLY: reaches, segments, lake ids and each element's three edge slots keep the
 * caller's order.  Every element's own operation order and every river / junction sum are then unchanged, so
 * an ordered handle returns the bits of a plain one (tests/test_gpu_renumber.py); what changes is
 * which elements share a 256-element tile (in-tile edge sharing) and how the neighbour gathers hit L2.
 *
 * Convention: perm[k] is the caller's index of internal element k; inv[c] the internal index of caller
 * element c.  One rule covers the ABI of an ordered handle: HOST pointers are in the caller's numbering,
 * DEVICE pointers are in the internal numbering.
 *
 * Lake models are refused (SHUD_ERR_UNSUPPORTED): a lake sums over its elements in element order.
 */
#ifndef SHUD_ORDER_H
#define SHUD_ORDER_H

#include "shud_rhs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SHUD_ORDER_IDENTITY 0
#define SHUD_ORDER_USER     1   /* user_perm[NE], validated as a permutation (SHUD_ERR_ARG otherwise)       */
#define SHUD_ORDER_BFS      2   /* breadth-first over nabr (below)                                          */
#define SHUD_ORDER_TILES    3   /* breadth-first pockets that each stop at a sharing-tile border (below)    */

/* shud_rhs_permute: direction and shape */
#define SHUD_PERM_TO_INTERNAL 0 /* dst[k] = src[perm[k]]                                                    */
#define SHUD_PERM_TO_CALLER   1 /* dst[c] = src[inv[c]]                                                     */
#define SHUD_PERM_STATE 0       /* [sf|us|gw|riv]: three element blocks permuted, the reach tail copied     */
#define SHUD_PERM_ELE   1       /* [NE]                                                                     */
#define SHUD_PERM_ELE3  2       /* [3*NE] edge-major: each plane permuted                                   */

/* ---- device-free (libshud_rhs.so, beside the table builder) ---- */
/* perm[NE]: new element k is old perm[k].  SHUD_ORDER_BFS: components start from the unvisited elements in
 * ascending (number of nabr >= 0 slots, index); the queue is FIFO; an element's unvisited neighbours are
 * enqueued in slot order 0, 1, 2 when first seen.
 * SHUD_ORDER_TILES: the same search, cut into pockets that never cross a border of the T-element sharing tile
 * (T = 256, the tile of the in-tile edge sharing), so that neighbours stay inside one tile at any mesh size (a
 * breadth-first front of an N-element mesh is ~sqrt(N) wide and outgrows the tile above ~65k elements):
 *     starts = elements ascending by (number of nabr >= 0 slots, index)        as SHUD_ORDER_BFS
 *     done[] = false; out = []; seeds = FIFO
 *     while len(out) < NE:
 *         s = the first not-done element popped from seeds; if seeds runs empty, the next not-done element of starts
 *         cap = T - (len(out) mod T)                      room left in the tile being filled
 *         done[s] = true; q = FIFO [s]; n = 1
 *         while q not empty:
 *             i = q.pop_front(); out.append(i)
 *             for slot in 0, 1, 2:
 *                 v = nabr[slot][i]
 *                 if v >= 0 and not done[v]:
 *                     if n < cap: done[v] = true; q.push_back(v); n += 1
 *                     else:       seeds.push_back(v)      a seed for a later tile; skipped when popped if done by then
 *     perm = out
 * A pocket that runs dry before cap leaves its tile to be filled from the next seed (that tile is then disconnected).
 * Tiles are visited breadth-first over tiles (the seeds are FIFO).  The planner keeps seeds free of duplicates with a
 * flag, which gives the same order (a later duplicate is always done when popped): memory is O(NE). */
int shud_order_plan(const ShudMeshSoA *mesh, int kind, const int32_t *user_perm, int32_t *perm);

/* The model under perm, in library-owned storage: every [NE] array gathered, every [3*NE] edge-major array
 * gathered per plane, nabr and seg_ele remapped through the inverse, everything else shared with the input
 * (which must outlive the result).  NULL inputs stay NULL.  par / par_out may be NULL. */
typedef struct shud_ordered *shud_ordered_t;
int shud_order_apply(const ShudMeshSoA *mesh, const ShudParamsSoA *par, const int32_t *perm,
                     shud_ordered_t *out, ShudMeshSoA *mesh_out, ShudParamsSoA *par_out);
int shud_order_free(shud_ordered_t o);

/* Any other per-element host array (ET mesh and parameters, ShudStepInputs arrays, y0, IS / snow):
 * dst[p*n + k] = src[p*n + perm[k]] for p < planes, elements of elem_bytes bytes.  src != dst. */
int shud_order_gather_host(const int32_t *perm, int32_t n, size_t elem_bytes, int32_t planes, const void *src,
                           void *dst);

/* ---- ordered handles ---- */
/* shud_rhs_create, with the device side in the planned order.  Transparent (caller's numbering) on every host
 * pointer: shud_rhs_eval(SHUD_WHERE_HOST), shud_rhs_cvrhs, the [NE] arrays of shud_rhs_set_step_inputs and every
 * array of shud_rhs_sync_diagnostics.  Device-pointer evals, shud_rhs_device_array, the ET prelude and the
 * integrator's device vectors are in the internal numbering; shud_rhs_permute carries vectors across.
 * ShudErr of an ordered handle is that of a plain one: first_index is the lowest offending element in the CALLER's
 * numbering (the kernels' error report maps each flagged element and takes the minimum over caller indices), so exit
 * code and message, which compare these indices, agree too. */
int shud_rhs_create_ordered(const ShudMeshSoA *mesh, const ShudParamsSoA *par, const ShudRhsOptions *opt, int kind,
                            const int32_t *user_perm, shud_rhs_t *out);
/* kind and, where not NULL, perm_host[NE] / inv_host[NE].  A plain handle reports SHUD_ORDER_IDENTITY. */
int shud_rhs_order(shud_rhs_t h, int *kind, int32_t *perm_host, int32_t *inv_host);
/* Stream-ordered on the handle's stream, device pointers, d_src != d_dst.  On a plain (or identity) handle: a copy. */
int shud_rhs_permute(shud_rhs_t h, int dir, int what, const double *d_src, double *d_dst);

#ifdef __cplusplus
}
#endif
#endif /* SHUD_ORDER_H */
