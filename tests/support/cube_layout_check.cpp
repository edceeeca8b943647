// Stand-alone check of step_layout::CubeOut in simple_mip_solver_amd/csrc/step_layout.h (built and run by
// tests/test_cube_search_abi.py), in the manner of wr_layout_check.cpp: the fields lie in the documented order, do
// not overlap, are aligned to their element size, end where bytes() says, bytes() is what the engine allocates per
// step buffer (an objective, and a status and two counts for each of the cube search, the lift and the local
// search, per point), and every field is written through view() into a buffer of exactly bytes() bytes, so a sanitizer
// build catches a view that leaves it.
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
    if (!ok && g_fail++ < 20) std::fprintf(stderr, "FAIL CubeOut(%zu): %s\n", cap, what);
}

int main() {
    for (size_t cap : {(size_t)1, (size_t)3, (size_t)32, (size_t)65, (size_t)8192}) {
        const CubeOut l(cap);
        char *p = (char *)std::malloc(l.bytes());
        const auto v = l.view(p);
        expect(l.obj == 0 && l.status == 8 * cap, "obj at 0, status behind cap objectives", cap);
        expect(l.counts == l.status + 4 * cap && l.lift_status == l.counts + 8 * cap, "counts, then lift_status", cap);
        expect(l.lift_moves == l.lift_status + 4 * cap && l.ls_status == l.lift_moves + 8 * cap, "lift_moves, then ls_status", cap);
        expect(l.ls_moves == l.ls_status + 4 * cap && l.end == l.ls_moves + 8 * cap, "ls_moves, then the end", cap);
        expect(l.obj % 8 == 0 && l.status % 4 == 0 && l.counts % 4 == 0 && l.lift_status % 4 == 0 && l.lift_moves % 4 == 0 &&
                   l.ls_status % 4 == 0 && l.ls_moves % 4 == 0, "a field is misaligned", cap);
        expect(l.bytes() == l.end && l.bytes() == 44 * cap, "bytes() is not 44 per point", cap);
        expect((char *)v.obj == p + l.obj && (char *)v.status == p + l.status && (char *)v.counts == p + l.counts &&
                   (char *)v.lift_status == p + l.lift_status && (char *)v.lift_moves == p + l.lift_moves &&
                   (char *)v.ls_status == p + l.ls_status && (char *)v.ls_moves == p + l.ls_moves, "view() disagrees with the offsets", cap);
        std::memset(v.obj, 0x5a, 8 * cap);
        std::memset(v.status, 0x5a, 4 * cap);
        std::memset(v.counts, 0x5a, 8 * cap);
        std::memset(v.lift_status, 0x5a, 4 * cap);
        std::memset(v.lift_moves, 0x5a, 8 * cap);
        std::memset(v.ls_status, 0x5a, 4 * cap);
        std::memset(v.ls_moves, 0x5a, 8 * cap);
        v.ls_moves[2 * cap - 1] = 7;   // (the last element of the last field)
        expect(p[l.bytes() - 4] == 7, "the last move count is not the last word", cap);
        bool all = true;
        for (size_t k = 0; k + 4 < l.bytes(); k++) all = all && p[k] == 0x5a;
        expect(all, "the fields leave a gap", cap);
        std::free(p);
    }
    static_assert(std::is_same<decltype(CubeOut(1).view((const char *)nullptr).obj), const double *>::value, "const view");
    static_assert(std::is_same<decltype(CubeOut(1).view((const char *)nullptr).ls_moves), const int32_t *>::value, "const view");
    std::printf("cube_layout: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
