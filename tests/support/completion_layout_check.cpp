// Stand-alone check of step_layout::CompOut in simple_mip_solver_amd/csrc/step_layout.h (built and run by
// tests/test_completion_abi.py), in the manner of cube_layout_check.cpp: the fields lie in the documented order, do
// not overlap, are aligned to their element size, end where bytes() says, bytes() is what the engine allocates per
// step buffer (an objective, a status and a pivot count for each point of two blocks of cap points), and every field
// is written through view() into a buffer of exactly bytes() bytes, so a sanitizer build catches a view that leaves it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <type_traits>

#include "step_layout.h"

using namespace step_layout;

static int g_fail = 0, g_checks = 0;

static void expect(bool ok, const char *what, size_t cap) {
    g_checks++;
    if (!ok && g_fail++ < 20) std::fprintf(stderr, "FAIL CompOut(%zu): %s\n", cap, what);
}

int main() {
    for (size_t cap : {(size_t)1, (size_t)3, (size_t)32, (size_t)65, (size_t)8192}) {
        const CompOut l(cap);
        char *p = (char *)std::malloc(l.bytes());
        const auto v = l.view(p);
        expect(l.obj == 0 && l.status == 16 * cap, "obj at 0, status behind 2 cap objectives", cap);
        expect(l.pivots == l.status + 8 * cap && l.end == l.pivots + 8 * cap, "pivots behind 2 cap statuses, then the end", cap);
        expect(l.obj % 8 == 0 && l.status % 4 == 0 && l.pivots % 4 == 0, "a field is misaligned", cap);
        expect(l.bytes() == l.end && l.bytes() == 32 * cap, "bytes() is not 16 per point of two blocks", cap);
        expect((char *)v.obj == p + l.obj && (char *)v.status == p + l.status && (char *)v.pivots == p + l.pivots,
               "view() disagrees with the offsets", cap);
        std::memset(v.obj, 0x5a, 16 * cap);
        std::memset(v.status, 0x5a, 8 * cap);
        std::memset(v.pivots, 0x5a, 8 * cap);
        v.pivots[2 * cap - 1] = 7;   // (the last element of the last field: the cube block's last point)
        expect(p[l.bytes() - 4] == 7, "the last pivot count is not the last word", cap);
        bool all = true;
        for (size_t k = 0; k + 4 < l.bytes(); k++) all = all && p[k] == 0x5a;
        expect(all, "the fields leave a gap", cap);
        std::free(p);
    }
    static_assert(std::is_same<decltype(CompOut(1).view((const char *)nullptr).obj), const double *>::value, "const view");
    static_assert(std::is_same<decltype(CompOut(1).view((const char *)nullptr).pivots), const int32_t *>::value, "const view");
    std::printf("completion_layout: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
