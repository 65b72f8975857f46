// ckpt_fmt_check.cpp — the checkpoint container (csrc/shud_ckpt_fmt.cpp) as a stand-alone host program, for a
// sanitizer pass without a device: writes a section set, reads it back, then verifies truncated copies (every 97th
// length) and copies with one flipped bit (every 61st byte); each of them must be refused.  CPU only:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ishud-up_amd/csrc \
//       shud-up_amd/csrc/shud_ckpt_fmt.cpp tools/ckpt_fmt_check.cpp -o /tmp/ckpt_fmt_check && /tmp/ckpt_fmt_check [dir]
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "shud_ckpt.h"

static char g_msg[512];
int shud_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    return code;
}

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : "/tmp";
    const std::string path_s = dir + "/ckpt_fmt_check.ckpt", bad_s = dir + "/ckpt_fmt_check.bad";
    const char *path = path_s.c_str();
    std::vector<uint64_t> a(0), b(1, 42), c(1025);
    for (size_t i = 0; i < c.size(); i++) c[i] = i * 0x9E3779B97F4A7C15ull;
    const char *names[3] = {"zero", "one", "a.name.that.is.much.longer.than.the.field"};
    const uint64_t *data[3] = {nullptr, b.data(), c.data()};
    const uint64_t words[3] = {0, 1, 1025};
    ShudCkptInfo info = {};
    info.step = 7;
    if (shud_ckpt_write_sections(path, &info, 3, names, data, words)) { printf("write: %s\n", g_msg); return 1; }
    if (shud_ckpt_verify(path)) { printf("verify: %s\n", g_msg); return 1; }
    ShudCkptInfo got;
    if (shud_ckpt_info(path, &got) || got.step != 7 || got.n_sections != 3) { printf("info: %s\n", g_msg); return 1; }
    std::vector<uint64_t> out(2000);
    uint64_t n = 0;
    if (shud_ckpt_read_section(path, "one", out.data(), out.size(), &n) || n != 1 || out[0] != 42) return 2;
    if (shud_ckpt_read_section(path, "a.name.that.is.much.lon", out.data(), out.size(), &n) || n != 1025) return 3;
    if (shud_ckpt_read_section(path, "one", out.data(), 0, &n) == 0) return 4;
    // damaged copies: every prefix length class and a flipped byte at a stride
    FILE *fp = fopen(path, "rb");
    std::vector<unsigned char> raw(1 << 16);
    const size_t len = fread(raw.data(), 1, raw.size(), fp);
    fclose(fp);
    const char *bad = bad_s.c_str();
    int refused = 0, tried = 0;
    for (size_t cut = 0; cut < len; cut += 97) {
        fp = fopen(bad, "wb");
        fwrite(raw.data(), 1, cut, fp);
        fclose(fp);
        tried++;
        refused += shud_ckpt_verify(bad) != 0;
    }
    for (size_t at = 0; at < len; at += 61) {
        std::vector<unsigned char> r(raw.begin(), raw.begin() + len);
        r[at] ^= 0x40;
        fp = fopen(bad, "wb");
        fwrite(r.data(), 1, len, fp);
        fclose(fp);
        tried++;
        refused += shud_ckpt_verify(bad) != 0;
    }
    remove(path);
    remove(bad);
    printf("refused %d of %d damaged files\n", refused, tried);
    return refused == tried ? 0 : 5;
}
