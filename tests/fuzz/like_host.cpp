// like_host -- drives the pattern compiler and the shared matcher of
// csrc/fls_strmatch.hpp on the CPU (tests/test_like_host.py builds it with
// -fsanitize=address,undefined).
//
// Input file: one triple per line, `<string hex> <pattern hex> <escape>`, an
// empty byte string written `-`, escape 0 for none.  One output line each:
//   <status> <ntok> <min_len> <prefix hex or -> <ends_anyn> <exact> <match>
// status 0 ok / 1 trailing escape / 2 too many tokens (then the rest is 0 - 0 0 0).
// The string and the tokens are copied into exact-size heap blocks, so a read
// one byte outside [ptr, ptr + len) or past the tokens is an ASan report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "fls_strmatch.hpp"

static std::string unhex(const std::string &h) {
    std::string out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((char)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

static std::string hex(const std::string &s) {
    if (s.empty()) return "-";
    static const char *d = "0123456789abcdef";
    std::string out;
    for (unsigned char c : s) {
        out.push_back(d[c >> 4]);
        out.push_back(d[c & 15]);
    }
    return out;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: like_host <triples file>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "like_host: cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string sh, ph;
        unsigned esc = 0;
        if (!(ls >> sh >> ph >> esc)) {
            fprintf(stderr, "like_host: bad line '%s'\n", line.c_str());
            return 2;
        }
        const std::string s = unhex(sh), p = unhex(ph);
        uint8_t *pb = (uint8_t *)malloc(p.size() ? p.size() : 1);
        if (!p.empty()) memcpy(pb, p.data(), p.size());
        fls::CompiledPattern cp;
        const int rc = fls::pattern_compile(pb, p.size(), esc, cp);
        free(pb);
        if (rc != fls::PAT_OK) {
            printf("%d 0 0 - 0 0 0\n", rc);
            continue;
        }
        uint8_t *sb = (uint8_t *)malloc(s.size() ? s.size() : 1);
        if (!s.empty()) memcpy(sb, s.data(), s.size());
        uint16_t *tb = (uint16_t *)malloc(cp.tok.size() ? cp.tok.size() * 2 : 2);
        if (!cp.tok.empty()) memcpy(tb, cp.tok.data(), cp.tok.size() * 2);
        // (a zero-length block still has one allocated byte: lengths are passed exactly)
        const bool m = fls::like_match(s.empty() ? sb + 1 : sb, (uint32_t)s.size(), cp.tok.empty() ? tb + 1 : tb,
                                       (uint32_t)cp.tok.size());
        printf("0 %zu %u %s %d %d %d\n", cp.tok.size(), cp.min_len, hex(cp.prefix).c_str(), cp.ends_anyn ? 1 : 0,
               cp.exact ? 1 : 0, m ? 1 : 0);
        free(sb);
        free(tb);
    }
    return 0;
}
