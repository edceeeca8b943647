// Stand-alone check of mipx::LpdiveOut in simple_mip_solver_amd/csrc/lpdive_kernels.hip.h (built and run by
// tests/test_lp_dive_layout.py), in the manner of completion_layout_check.cpp: the fields lie in the documented order,
// do not overlap, are aligned to their element size, end where bytes() says, every pointer of view(base) is base + the
// public offset of its field, and every field is written through view() into a buffer of exactly bytes() bytes, so a
// sanitizer build catches a view that leaves it.  The header holds kernels beside the layout, so this file is
// compiled as HIP, host side only: no device code is made and no HIP call is issued.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <type_traits>

#include "lpdive_kernels.hip.h"

using mipx::LpdiveOut;

static int g_fail = 0, g_checks = 0;

static void expect(bool ok, const char *what, size_t cap) {
    g_checks++;
    if (!ok && g_fail++ < 20) std::fprintf(stderr, "FAIL LpdiveOut(%zu): %s\n", cap, what);
}

int main() {
    for (size_t cap : {(size_t)1, (size_t)3, (size_t)257}) {
        const LpdiveOut l(cap);
        char *p = (char *)std::malloc(l.bytes());
        const auto v = l.view(p);
        expect(l.obj == 0 && l.status == 8 * cap, "obj at 0, status behind cap objectives", cap);
        expect(l.rounds == l.status + 4 * cap && l.fixings == l.rounds + 4 * cap && l.flips == l.fixings + 4 * cap &&
                   l.pivots == l.flips + 4 * cap && l.end == l.pivots + 4 * cap,
               "status, rounds, fixings, flips, pivots: cap words each, then the end", cap);
        expect(l.obj % 8 == 0 && l.status % 4 == 0 && l.rounds % 4 == 0 && l.fixings % 4 == 0 && l.flips % 4 == 0 &&
                   l.pivots % 4 == 0,
               "a field is misaligned", cap);
        expect(l.bytes() == l.end && l.bytes() == 28 * cap, "bytes() is not 28 per point", cap);
        expect((char *)v.obj == p + l.obj, "view().obj is not base + obj", cap);
        expect((char *)v.status == p + l.status, "view().status is not base + status", cap);
        expect((char *)v.rounds == p + l.rounds, "view().rounds is not base + rounds", cap);
        expect((char *)v.fixings == p + l.fixings, "view().fixings is not base + fixings", cap);
        expect((char *)v.flips == p + l.flips, "view().flips is not base + flips", cap);
        expect((char *)v.pivots == p + l.pivots, "view().pivots is not base + pivots", cap);
        std::memset(v.obj, 0x5a, 8 * cap);
        std::memset(v.status, 0x5a, 4 * cap);
        std::memset(v.rounds, 0x5a, 4 * cap);
        std::memset(v.fixings, 0x5a, 4 * cap);
        std::memset(v.flips, 0x5a, 4 * cap);
        std::memset(v.pivots, 0x5a, 4 * cap);
        v.pivots[cap - 1] = 7;   // (the last element of the last field)
        expect(p[l.bytes() - 4] == 7, "the last pivot count is not the last word", cap);
        bool all = true;
        for (size_t k = 0; k + 4 < l.bytes(); k++) all = all && p[k] == 0x5a;
        expect(all, "the fields leave a gap", cap);
        std::free(p);
    }
    static_assert(std::is_same<decltype(LpdiveOut(1).view((const char *)nullptr).obj), const double *>::value, "const view");
    static_assert(std::is_same<decltype(LpdiveOut(1).view((const char *)nullptr).pivots), const int32_t *>::value, "const view");
    static_assert(std::is_same<decltype(LpdiveOut(1).view((char *)nullptr).status), int32_t *>::value, "mutable view");
    std::printf("lpdive_layout: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
