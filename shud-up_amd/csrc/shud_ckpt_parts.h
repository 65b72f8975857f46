// shud_ckpt_parts.h — internal: what each object (shud_ode.cpp, shud_et.cpp, shud_out.hip, shud_mon.hip) hands to the
// checkpoint unit (shud_ckpt.cpp), and the container's reader (shud_ckpt_fmt.cpp).  Not part of the C-ABI.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <vector>

#include "shud_ckpt.h"

struct CkptDev {                         // one live device buffer of an object
    char name[SHUD_CKPT_NAME_LEN];
    void *p;
    size_t bytes;                        // whole 8-byte words go through the pack kernel, a 4-byte tail beside them
};

// host scalars: saving appends them to buf, loading reads them back in the same order
struct CkptAr {
    bool load = false, ok = true;
    std::vector<uint8_t> buf;
    size_t pos = 0;
    void raw(void *p, size_t n) {
        if (!load) {
            const uint8_t *b = (const uint8_t *)p;
            buf.insert(buf.end(), b, b + n);
        } else if (pos + n <= buf.size()) {
            memcpy(p, buf.data() + pos, n);
        } else {
            ok = false;
        }
        pos += n;
    }
    template <class T> void pod(T &v) {
        static_assert(std::is_trivially_copyable<T>::value, "pod");
        raw(&v, sizeof(T));
    }
    // a value that must be the same in the file and in the object (loading compares instead of assigning)
    template <class T> bool same(const T &v) {
        T x = v;
        pod(x);
        return !load || memcmp(&x, &v, sizeof(T)) == 0;
    }
};

struct CkptPart {
    std::vector<CkptDev> dev;
    void add(const char *name, const void *p, size_t bytes) {
        if (!p) return;
        CkptDev d{};
        strncpy(d.name, name, SHUD_CKPT_NAME_LEN - 1);
        d.p = const_cast<void *>(p);
        d.bytes = bytes;
        dev.push_back(d);
    }
};

struct shud_ode;
struct shud_out;
struct shud_mon;
struct shud_rhs;

// Each object lists its live device buffers (…_ckpt_dev) and passes its host scalars through an archive
// (…_ckpt_host: saving when !ar.load; loading assigns them — called only after every check has passed).
// …_ckpt_check: SHUD_OK, or the reason this object cannot be checkpointed / does not match the header.
int shud_ode_ckpt_check(shud_ode *o, ShudCkptInfo *hdr, bool restore);   // save: fills the ode_* fields; restore: compares
int shud_ode_ckpt_dev(shud_ode *o, CkptPart &p);                         // synchronizes the integrator's stream first
int shud_ode_ckpt_host(shud_ode *o, CkptAr &ar);
void *shud_ode_ckpt_stream(shud_ode *o);                                 // the integrator's hipStream_t
int shud_et_ckpt_dev(shud_rhs *h, CkptPart &p);
int shud_et_ckpt_host(shud_rhs *h, CkptAr &ar, bool check_only);         // check_only (load): compare the settings only
// section et.queues.host: int32 head_surf, size_surf, head_sub, size_sub, n_of_day, then double time_start
int shud_et_ckpt_queues(shud_rhs *h, CkptAr &ar);
int shud_out_ckpt_check(shud_out *o);
void *shud_out_ckpt_stream(shud_out *o);
int shud_out_ckpt_dev(shud_out *o, CkptPart &p);                         // drains and flushes the writers first
int shud_out_ckpt_host(shud_out *o, CkptAr &ar, bool check_only);        // load: cuts the files back and seeks
int shud_mon_ckpt_host(shud_mon *m, CkptAr &ar, bool check_only);        // drains and flushes first

// container (shud_ckpt_fmt.cpp)
struct CkptFile {
    ShudCkptInfo hdr{};
    std::vector<ShudCkptSection> table;
    std::vector<uint64_t> payload;       // empty when read with payload = false
    const ShudCkptSection *find(const char *name) const {
        for (const auto &s : table)
            if (strncmp(s.name, name, SHUD_CKPT_NAME_LEN) == 0) return &s;
        return nullptr;
    }
};
// header + table checked (magic, version, sizes, header checksum); payload: read it and check every section
int shud_ckpt_fmt_read(const char *path, bool payload, CkptFile *f);
// header checksum into hdr (over header + table with the checksum fields zero)
void shud_ckpt_fmt_seal(ShudCkptInfo *hdr, const ShudCkptSection *table);
