// tuning_dump -- prints what read_decode_tuning() (csrc/fls_tuning.hpp) makes
// of the environment, one `name=value` line per field, and the blocks-per-CU
// cap decode_grid_size takes.  Each argument is one environment to do so
// under, "NAME=VALUE,NAME=VALUE" (or empty) set over the process's own and
// unset again, with a "--" line after each; without arguments, the process's
// own.  tests/test_tuning.py builds it with -fsanitize=address,undefined and
// compares every line with the hooks' documented parse.
#include <cstdio>
#include <vector>

#include "fls_tuning.hpp"

static void hook(const char *name, const fls::StrictHook &h) {
    printf("%s.given=%d\n%s.ok=%d\n%s.text=%s\n", name, (int)h.given, name, (int)h.ok, name, h.text.c_str());
}

static void dump() {
    const fls::DecodeTuning t = fls::read_decode_tuning();
    const fls::DecodeTuning::List &l = t.list;
    const fls::DecodeTuning::Launch &x = t.launch;
#define F(s, f) printf(#s "." #f "=%d\n", (int)s.f)
    F(l, flags); F(l, static_pct); F(l, tail_pieces); F(l, blocks_per_cu); F(l, guided_min_vecs);
    F(l, guided_factor); F(l, dict_wg); F(l, dict_wg_min_vecs_per_cu); F(l, dict_wg_streams);
    F(x, fsst_seg); F(x, overlap_decode_bpc); F(x, overlap_fsst_wpc); F(x, overlap_min_vecs_per_cu);
    F(x, overlap_decode_prio); F(x, overlap_cu_split); F(x, overlap_guided); F(x, fused);
    F(x, fused_fsst16_given); F(x, fused_fsst16); F(x, fused_piece); F(x, fused_wpc); F(x, fused_static_pct);
    F(x, fused_min_vecs_per_cu); F(x, fused_static_first); F(x, fused_halving); F(x, fused_tail);
    F(x, fused_tail_split); F(x, fused_x); F(x, fsst_variant); F(x, fsst_seg_cap); F(x, fsst_wpc); F(x, fsst_piece);
#undef F
    hook("x.fused_x_hook", x.fused_x_hook);
    hook("x.fsst_variant_hook", x.fsst_variant_hook);
    printf("blocks_per_cu_cap=%d\n", fls::blocks_per_cu_cap());
    // the key's own comparison, against the defaults
    printf("list_is_default=%d\n", (int)(l == fls::DecodeTuning().list));
}

int main(int argc, char **argv) {
    if (argc < 2) dump();
    for (int i = 1; i < argc; ++i) {
        std::vector<std::string> names;
        const std::string spec = argv[i];
        for (size_t p = 0; p < spec.size();) {
            const size_t end = std::min(spec.find(',', p), spec.size()), eq = spec.find('=', p);
            if (eq >= end) return 2;
            names.push_back(spec.substr(p, eq - p));
            setenv(names.back().c_str(), spec.substr(eq + 1, end - eq - 1).c_str(), 1);
            p = end + 1;
        }
        dump();
        printf("--\n");
        for (const std::string &n : names) unsetenv(n.c_str());
    }
    return 0;
}
