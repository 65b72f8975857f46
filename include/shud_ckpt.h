/* shud_ckpt.h — C-ABI of the exact checkpoint / resume of a device run.
 *
 * The reference can only warm-start (<prj>.cfg.ic.update + INIT_MODE 3): five state arrays, a new CVODE at order 1.
 * A checkpoint holds everything a continued run reads before it overwrites it — the integrator's Nordsieck history,
 * controller and deferred completion (shud_ode.h), the RHS handle's carried state, step inputs and replay buffer
 * (shud_rhs.h), the ET prelude's carried state and day-mean queues (shud_et.h), the output set's accumulators and
 * file lengths (shud_out.h) and the monitors' counters (shud_mon.h) — so that stop, new process, shud_ckpt_restore,
 * continue gives bit for bit the states, counters and files of the uninterrupted run.
 *
 * shud_ckpt_snapshot is called between two shud_ode_solve calls, after that step's export and monitors.  One
 * batched device pass (shud_ckpt.hip) copies every live device buffer of the listed objects into one staging slab in
 * HBM and forms each section's checksum; the host scalars are copied; the call returns.  The slab then drains
 * through two pinned banks and a writer thread into <path>.tmp, which is flushed and renamed onto <path>: a process
 * killed during a checkpoint leaves the previous one intact.  A second snapshot waits for the first one's drain.
 *
 * File format (version 1, little-endian, every field naturally aligned, no padding):
 *   ShudCkptInfo                      fixed header (below); hdr_c0 / hdr_c1 = checksum of header + section table
 *                                     taken with those two fields zero
 *   ShudCkptSection[n_sections]       {name, offset, words, c0, c1}; offset in 8-byte words from the payload start
 *   payload                           payload_words 8-byte words: host-scalar sections ("*.host"), then the image
 *                                     of the staging slab (device buffers in the handle's internal numbering)
 * Checksum of a section of n words w_i: c0 = sum w_i, c1 = sum (i + 1) w_i, both mod 2^64.
 *
 * Refused with SHUD_ERR_UNSUPPORTED: partitioned handles, output sets with a NetCDF sink, and a run with a
 * water-balance object (ShudCkptParts.wb non-NULL: shud_wb keeps accumulators of its own, which no checkpoint holds).
 * Any mismatch between a file and the objects given to shud_ckpt_restore returns SHUD_ERR_ARG with a message
 * (shud_rhs_last_error_string) that names the field, and leaves the objects untouched and usable: nothing of them
 * is written, allocated or cut back before every check has passed.  The one failure after that point is
 * SHUD_ERR_HIP from the verification of the upload (the uploaded buffers' sums against the section table): the
 * device buffers then hold the file's bytes and the scalars the objects' own, and the objects must not be used.
 */
#ifndef SHUD_CKPT_H
#define SHUD_CKPT_H

#include <stdint.h>

#include "shud_mon.h"
#include "shud_ode.h"
#include "shud_out.h"
#include "shud_rhs.h"
#include "shud_wb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SHUD_CKPT_MAGIC "SHUDCKP1"
#define SHUD_CKPT_VERSION 1
#define SHUD_CKPT_NAME_LEN 24
#define SHUD_CKPT_MAX_SECTIONS 512
#define SHUD_CKPT_LAYOUT_SOA 0
#define SHUD_CKPT_LAYOUT_PACKED 1
#define SHUD_CKPT_LAYOUT_HYBRID 2

typedef struct {
    char     magic[8];                     /* SHUD_CKPT_MAGIC                                                    */
    uint32_t version, abi_version;         /* SHUD_CKPT_VERSION, shud_rhs_abi_version()                          */
    uint32_t n_sections, header_bytes;     /* header_bytes = sizeof(ShudCkptInfo) + n_sections * sizeof(Section) */
    int32_t  ne, nr, ns, nl;               /* 0 without an RHS handle (shud_ode_create_fn)                       */
    int64_t  ny;
    int32_t  mode, layout;                 /* SHUD_MODE_*, SHUD_CKPT_LAYOUT_*                                    */
    int32_t  n_classes, n_streamed, n_shared, order_kind;
    int32_t  have_rhs, have_et, have_ode, have_out, have_mon, ode_lazy;   /* ode_lazy: SHUD_ODE_LAZY_* settings  */
    uint64_t perm_c0, perm_c1;             /* checksum of perm[] (as int32 pairs); 0 for a plain handle          */
    uint64_t statics_c0, statics_c1;       /* fingerprint of the handle's static device tables                   */
    double   ode_reltol, ode_abstol, ode_init_step, ode_min_step, ode_max_step_inv;
    int64_t  ode_max_num_steps;
    int32_t  ode_maxl, ode_max_order;
    double   t;                            /* model time of the snapshot                                         */
    int64_t  step;                         /* solver-step index of the snapshot                                  */
    uint64_t payload_words;
    uint64_t hdr_c0, hdr_c1;
} ShudCkptInfo;

typedef struct {
    char     name[SHUD_CKPT_NAME_LEN];     /* NUL-padded                                                         */
    uint64_t offset, words, c0, c1;
} ShudCkptSection;

typedef struct shud_ckpt *shud_ckpt_t;
/* rhs may be NULL for a shud_ode_create_fn integrator; out and mon may be NULL; wb: the run's water-balance object,
 * if it has one — named so that the checkpoint is refused (SHUD_ERR_UNSUPPORTED) instead of silently incomplete */
typedef struct { shud_rhs_t rhs; shud_ode_t ode; shud_out_t out; shud_mon_t mon; shud_wb_t wb; } ShudCkptParts;

/* staging slab (sized at the first snapshot), copy stream, pinned banks, writer thread; stream (hipStream_t; NULL =
 * the default stream) carries the pack pass — normally the compute stream of the objects; an object on another
 * stream is made to wait for the pass (an event), so its next step cannot overwrite a buffer still being read */
int shud_ckpt_create(int device, void *stream, shud_ckpt_t *out);
int shud_ckpt_snapshot(shud_ckpt_t c, const ShudCkptParts *p, double t, int64_t step, const char *path);
/* the last snapshot's file is complete and renamed into place; returns the writer's first failure */
int shud_ckpt_flush(shud_ckpt_t c);
int shud_ckpt_destroy(shud_ckpt_t c);
/* device-free: the header; magic, version, sizes and the header checksum are checked */
int shud_ckpt_info(const char *path, ShudCkptInfo *info);
/* device-free: entry k of the section table (0 <= k < n_sections) */
int shud_ckpt_section(const char *path, int32_t k, ShudCkptSection *sec);
/* device-free: every section's checksum; a failure names the section */
int shud_ckpt_verify(const char *path);
/* The objects are built as for a new run (same mesh, parameters, options, order, ET attach, controls added after
 * shud_out_resume, monitors after shud_mon_resume), then take the file's state.  *t and *step receive the
 * snapshot's time and solver-step index. */
int shud_ckpt_restore(const char *path, const ShudCkptParts *p, double *t, int64_t *step);

/* container primitives (device-free; the tests' synthetic section sets go through them) */
void shud_ckpt_checksum(const uint64_t *w, uint64_t n, uint64_t *c0, uint64_t *c1);
/* writes <path>.tmp, flushes it and renames it onto <path>; info's n_sections, header_bytes, payload_words and
 * checksums are filled in here; section k is words[k] 8-byte words at data[k] */
int shud_ckpt_write_sections(const char *path, const ShudCkptInfo *info, int32_t n, const char *const *names,
                             const uint64_t *const *data, const uint64_t *words);
/* copies section `name` into out (cap words); *words receives its length.  SHUD_ERR_ARG if absent or cap is short */
int shud_ckpt_read_section(const char *path, const char *name, uint64_t *out, uint64_t cap, uint64_t *words);

/* test / measurement entries, in the style of shud_out_time_nc */
/* One launch of the pack kernel over nseg segments: segment k is words[k] 8-byte words taken from src (host,
 * concatenated), placed on the device 16-byte aligned plus 8 * misalign[k] bytes.  The destination slab is laid out
 * as a snapshot lays it out, with `guard` extra words before, between and after the segments, prefilled with
 * `fill`; slab (host, slab_cap words) receives the whole slab afterwards, dst_off[k] each segment's offset in it and
 * *slab_words its length.  verify != 0: a null destination (checksums only; the slab keeps the fill).  c0 / c1
 * receive the device sums. */
int shud_ckpt_pack_test(int32_t nseg, const uint64_t *src, const int64_t *words, const int32_t *misalign,
                        int32_t guard, uint64_t fill, int32_t verify, uint64_t *slab, int64_t slab_cap,
                        int64_t *slab_words, int64_t *dst_off, uint64_t *c0, uint64_t *c1);
/* ms of one pack pass over the live objects (HIP events, `reps` passes after a warm-up) and the bytes it moves */
int shud_ckpt_time_pack(shud_ckpt_t c, const ShudCkptParts *p, int reps, double *ms_pass, int64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif /* SHUD_CKPT_H */
