// shud_gpu_util.hpp — what shud_gpu.cpp and shud_gpu_part.cpp share: the output directory, the environment switches
// and the report of a failed library call.
#pragma once
#include <strings.h>
#include <sys/stat.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "shud_rhs.h"

// mkdir -p; 0 when the directory exists afterwards
static inline int mkdirs(const std::string &d) {
    std::string cur;
    for (size_t i = 0; i <= d.size(); i++) {
        if ((i == d.size() || d[i] == '/') && !cur.empty()) mkdir(cur.c_str(), 0755);
        if (i < d.size()) cur += d[i];
    }
    struct stat st;
    return stat(d.c_str(), &st) == 0 ? 0 : -1;
}

// env_truthy (WaterBalanceDiag.cpp:21-36): unset, "", "0", "false" and "off" (any case) are false
static inline bool env_truthy(const char *s) {
    if (s == nullptr || s[0] == '\0') return false;
    if (strcmp(s, "0") == 0) return false;
    if (strcasecmp(s, "false") == 0) return false;
    if (strcasecmp(s, "off") == 0) return false;
    return true;
}

// "<what>: <the library's last error>[ <more>]" on stderr -> 1, the exit code of an input / solver / device error
static inline int fail(const char *what, const char *more = nullptr) {
    if (more) fprintf(stderr, "%s: %s %s\n", what, shud_rhs_last_error_string(), more);
    else fprintf(stderr, "%s: %s\n", what, shud_rhs_last_error_string());
    return 1;
}
