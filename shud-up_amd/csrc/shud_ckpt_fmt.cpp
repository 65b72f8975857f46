// shud_ckpt_fmt.cpp — device-free container of a checkpoint (include/shud_ckpt.h): header, section table, payload;
// writer, reader and verifier.  Plain C++ (no HIP include), like shud_mon_fmt.cpp: links into libshud_rhs.so, where
// shud_ckpt.cpp calls it, and compiles into a stand-alone host program (which supplies shud_fail).
#include <errno.h>
#include <stdio.h>
#include <unistd.h>

#include "shud_ckpt_parts.h"

int shud_fail(int code, const char *fmt, ...);       // shud_rhs.cpp: message for shud_rhs_last_error_string()

static_assert(sizeof(ShudCkptInfo) == 224 && sizeof(ShudCkptSection) == 56, "checkpoint header layout");

extern "C" void shud_ckpt_checksum(const uint64_t *w, uint64_t n, uint64_t *c0, uint64_t *c1) {
    uint64_t a = 0, b = 0;
    for (uint64_t i = 0; i < n; i++) {
        a += w[i];
        b += (i + 1) * w[i];
    }
    if (c0) *c0 = a;
    if (c1) *c1 = b;
}

void shud_ckpt_fmt_seal(ShudCkptInfo *hdr, const ShudCkptSection *table) {
    hdr->hdr_c0 = hdr->hdr_c1 = 0;
    const size_t nh = sizeof(ShudCkptInfo) / 8, nt = (size_t)hdr->n_sections * sizeof(ShudCkptSection) / 8;
    std::vector<uint64_t> w(nh + nt);
    memcpy(w.data(), hdr, sizeof(ShudCkptInfo));
    if (nt) memcpy(w.data() + nh, table, nt * 8);
    shud_ckpt_checksum(w.data(), w.size(), &hdr->hdr_c0, &hdr->hdr_c1);
}

static std::string sec_name(const ShudCkptSection &s) {
    return std::string(s.name, strnlen(s.name, SHUD_CKPT_NAME_LEN));
}

int shud_ckpt_fmt_read(const char *path, bool payload, CkptFile *f) {
    if (!path || !f) return shud_fail(SHUD_ERR_ARG, "shud_ckpt: null argument");
    FILE *fp = fopen(path, "rb");
    if (!fp) return shud_fail(SHUD_ERR_ARG, "shud_ckpt: cannot open %s: %s", path, strerror(errno));
    struct Closer { FILE *fp; ~Closer() { fclose(fp); } } closer{fp};
    ShudCkptInfo &h = f->hdr;
    if (fread(&h, sizeof(h), 1, fp) != 1) return shud_fail(SHUD_ERR_ARG, "shud_ckpt: %s: truncated header", path);
    if (memcmp(h.magic, SHUD_CKPT_MAGIC, 8) != 0) return shud_fail(SHUD_ERR_ARG, "shud_ckpt: %s: wrong magic", path);
    if (h.version != SHUD_CKPT_VERSION)
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt: %s: format version %u, this build reads %d", path, h.version,
                         SHUD_CKPT_VERSION);
    if (h.n_sections > SHUD_CKPT_MAX_SECTIONS ||
        h.header_bytes != sizeof(ShudCkptInfo) + (size_t)h.n_sections * sizeof(ShudCkptSection))
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt: %s: header field n_sections / header_bytes damaged", path);
    f->table.resize(h.n_sections);
    if (h.n_sections && fread(f->table.data(), sizeof(ShudCkptSection), h.n_sections, fp) != h.n_sections)
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt: %s: truncated section table", path);
    ShudCkptInfo chk = h;
    shud_ckpt_fmt_seal(&chk, f->table.data());
    if (chk.hdr_c0 != h.hdr_c0 || chk.hdr_c1 != h.hdr_c1)
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt: %s: header checksum mismatch", path);
    for (const auto &s : f->table)
        if (s.offset > h.payload_words || s.words > h.payload_words - s.offset)
            return shud_fail(SHUD_ERR_ARG, "shud_ckpt: %s: section %s lies outside the payload", path, sec_name(s).c_str());
    // the file's length is part of the format: a short file is a torn write
    if (fseeko(fp, 0, SEEK_END) != 0) return shud_fail(SHUD_ERR_ARG, "shud_ckpt: %s: seek failed", path);
    const off_t len = ftello(fp);
    if ((uint64_t)len != h.header_bytes + 8 * h.payload_words)
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt: %s: file is %lld bytes, header says %llu (truncated?)", path,
                         (long long)len, (unsigned long long)(h.header_bytes + 8 * h.payload_words));
    f->payload.clear();
    if (!payload) return SHUD_OK;
    f->payload.resize(h.payload_words);
    if (fseeko(fp, h.header_bytes, SEEK_SET) != 0 ||
        (h.payload_words && fread(f->payload.data(), 8, h.payload_words, fp) != h.payload_words))
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt: %s: truncated payload", path);
    for (const auto &s : f->table) {
        uint64_t c0, c1;
        shud_ckpt_checksum(f->payload.data() + s.offset, s.words, &c0, &c1);
        if (c0 != s.c0 || c1 != s.c1)
            return shud_fail(SHUD_ERR_ARG, "shud_ckpt: %s: section %s: checksum mismatch (corrupted payload)", path,
                             sec_name(s).c_str());
    }
    return SHUD_OK;
}

extern "C" int shud_ckpt_info(const char *path, ShudCkptInfo *info) {
    if (!info) return shud_fail(SHUD_ERR_ARG, "shud_ckpt_info: null argument");
    CkptFile f;
    const int rc = shud_ckpt_fmt_read(path, false, &f);
    if (rc) return rc;
    *info = f.hdr;
    return SHUD_OK;
}

extern "C" int shud_ckpt_section(const char *path, int32_t k, ShudCkptSection *sec) {
    if (!sec) return shud_fail(SHUD_ERR_ARG, "shud_ckpt_section: null argument");
    CkptFile f;
    const int rc = shud_ckpt_fmt_read(path, false, &f);
    if (rc) return rc;
    if (k < 0 || k >= (int32_t)f.table.size()) return shud_fail(SHUD_ERR_ARG, "shud_ckpt_section: no section %d", k);
    *sec = f.table[k];
    return SHUD_OK;
}

extern "C" int shud_ckpt_verify(const char *path) {
    CkptFile f;
    return shud_ckpt_fmt_read(path, true, &f);
}

extern "C" int shud_ckpt_read_section(const char *path, const char *name, uint64_t *out, uint64_t cap,
                                      uint64_t *words) {
    if (!name) return shud_fail(SHUD_ERR_ARG, "shud_ckpt_read_section: null argument");
    CkptFile f;
    const int rc = shud_ckpt_fmt_read(path, true, &f);
    if (rc) return rc;
    const ShudCkptSection *s = f.find(name);
    if (!s) return shud_fail(SHUD_ERR_ARG, "shud_ckpt_read_section: %s has no section %s", path, name);
    if (words) *words = s->words;
    if (s->words > cap || (s->words && !out))
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt_read_section: section %s has %llu words, room for %llu", name,
                         (unsigned long long)s->words, (unsigned long long)cap);
    if (s->words) memcpy(out, f.payload.data() + s->offset, 8 * s->words);
    return SHUD_OK;
}

extern "C" int shud_ckpt_write_sections(const char *path, const ShudCkptInfo *info, int32_t n, const char *const *names,
                                        const uint64_t *const *data, const uint64_t *words) {
    if (!path || !info || n < 0 || n > SHUD_CKPT_MAX_SECTIONS || (n > 0 && (!names || !data || !words)))
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt_write_sections: bad argument");
    ShudCkptInfo h = *info;
    memcpy(h.magic, SHUD_CKPT_MAGIC, 8);
    h.version = SHUD_CKPT_VERSION;
    h.n_sections = (uint32_t)n;
    h.header_bytes = (uint32_t)(sizeof(ShudCkptInfo) + (size_t)n * sizeof(ShudCkptSection));
    std::vector<ShudCkptSection> table((size_t)n);
    uint64_t off = 0;
    for (int k = 0; k < n; k++) {
        ShudCkptSection &s = table[k];
        memset(&s, 0, sizeof(s));
        if (!names[k] || (words[k] && !data[k])) return shud_fail(SHUD_ERR_ARG, "shud_ckpt_write_sections: section %d", k);
        strncpy(s.name, names[k], SHUD_CKPT_NAME_LEN - 1);
        s.offset = off;
        s.words = words[k];
        shud_ckpt_checksum(data[k], words[k], &s.c0, &s.c1);
        off += words[k];
    }
    h.payload_words = off;
    shud_ckpt_fmt_seal(&h, table.data());
    const std::string tmp = std::string(path) + ".tmp";
    FILE *fp = fopen(tmp.c_str(), "wb");
    if (!fp) return shud_fail(SHUD_ERR_ARG, "shud_ckpt: cannot open %s: %s", tmp.c_str(), strerror(errno));
    bool ok = fwrite(&h, sizeof(h), 1, fp) == 1;
    if (ok && n) ok = fwrite(table.data(), sizeof(ShudCkptSection), (size_t)n, fp) == (size_t)n;
    for (int k = 0; ok && k < n; k++)
        if (words[k]) ok = fwrite(data[k], 8, words[k], fp) == words[k];
    if (ok) ok = fflush(fp) == 0 && fsync(fileno(fp)) == 0;
    if (fclose(fp) != 0) ok = false;
    if (!ok || rename(tmp.c_str(), path) != 0) {
        remove(tmp.c_str());
        return shud_fail(SHUD_ERR_ARG, "shud_ckpt: cannot write %s: %s", path, strerror(errno));
    }
    return SHUD_OK;
}
