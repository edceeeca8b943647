// Stand-alone check of simple_mip_solver_amd/csrc/step_layout.h (built and run by tests/test_step_layout.py).
// For every layout and grid point: the fields lie in the documented order, do not overlap, are aligned to their
// element size, end where bytes() says, and bytes() is the size the engine allocated before the layouts had a
// definition (the formulas below are transcribed from that code).  Every field is then written through view()
// into a buffer of exactly bytes() bytes, so a sanitizer build catches a view that leaves it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "step_layout.h"

using namespace step_layout;

static int g_fail = 0, g_checks = 0;

struct Field { const char *name; size_t off, elem, count; const void *ptr; };

static void expect(bool ok, const char *layout, const char *what, const char *field = "") {
    g_checks++;
    if (!ok && g_fail++ < 20) std::fprintf(stderr, "FAIL %s: %s %s\n", layout, what, field);
}

// fields: in the documented order, with the pointers view() gave for a buffer at base
static void check(const char *layout, const std::vector<Field> &f, size_t bytes, size_t expected, char *base) {
    size_t end = 0;
    for (size_t i = 0; i < f.size(); i++) {
        expect(f[i].off >= end, layout, "out of order or overlapping:", f[i].name);
        expect(f[i].off % f[i].elem == 0, layout, "misaligned:", f[i].name);
        expect(f[i].ptr == base + f[i].off, layout, "view() disagrees with the offset of", f[i].name);
        end = f[i].off + f[i].elem * f[i].count;
        if (end <= bytes) std::memset(base + f[i].off, 0x5a, f[i].elem * f[i].count);
    }
    expect(end == bytes, layout, "bytes() is not the end of the last field");
    expect(bytes == expected, layout, "bytes() is not the size the engine allocated");
}

struct Buf {   // exactly n bytes (malloc aligns them for any field)
    char *p;
    explicit Buf(size_t n) : p((char *)std::malloc(n)) {}
    ~Buf() { std::free(p); }
};

int main() {
    const size_t batches[] = {1, 2, 3, 64, 1024}, levels[] = {1, 2, 9}, caps[] = {1, 7}, pers[] = {2, 18};
    const size_t ask_cap = 2048, ask_size = 16, open_size = 32;   // kAskCap, ScoreArgs::Ask, OpenEntry
    for (size_t MB : batches) {
        for (size_t L : levels) {
            for (size_t ac : {ask_cap, caps[0], caps[1]}) {
                const StepPack s(L, MB, ac, ask_size);
                const size_t OB = L * MB, DB = (L > 1 ? L - 1 : 1) * MB;
                const size_t ask_off = (OB * (2 * 8 + 5 * 4) + DB * (8 + 2 * 4) + 15) / 16 * 16;   // layout_pack
                Buf b(s.bytes());
                const auto v = s.view(b.p);
                check("StepPack", {{"obj", s.obj, 8, OB, v.obj}, {"bval", s.bval, 8, OB, v.bval}, {"dval", s.dval, 8, DB, v.dval},
                                   {"status", s.status, 4, OB, v.status}, {"bidx", s.bidx, 4, OB, v.bidx}, {"mipf", s.mipf, 4, OB, v.mipf},
                                   {"nprobe", s.nprobe, 4, OB, v.nprobe}, {"npiv", s.npiv, 4, OB, v.npiv}, {"dvar", s.dvar, 4, DB, v.dvar},
                                   {"ddir", s.ddir, 4, DB, v.ddir}, {"ask_count", s.ask_count, 16, 1, v.ask_count},
                                   {"ask", s.ask, ask_size, ac, v.ask}},
                      s.bytes(), ask_off + 16 + ac * ask_size, b.p);
                expect(s.ask_count == ask_off, "StepPack", "ask_count is not the ask_off of layout_pack");
                // the buffers are allocated for the deepest plunge: every shallower layout fits, and the deepest one
                // fits what mipx_tree_create_ex used to allocate (it counted the dive block once more than needed)
                const StepPack deep(9, MB, ac, ask_size);
                expect(deep.bytes() >= s.bytes(), "StepPack", "levels = 9 is smaller than a shallower layout");
                expect(deep.bytes() <= (9 * MB * (2 * 8 + 5 * 4) + 9 * MB * (8 + 2 * 4) + 15) / 16 * 16 + 16 + ac * ask_size,
                       "StepPack", "levels = 9 exceeds the allocation of mipx_tree_create_ex");
            }
        }
        {
            const CutState c(MB);
            Buf b(c.bytes());
            int32_t *base = (int32_t *)b.p;
            std::vector<Field> f = {{"counters", 0, 4, CutState::kCounters, c.counters(base)}};
            for (int k = 0; k < CutState::kFields; k++) f.push_back({"field", (4 + (size_t)k * MB) * 4, 4, MB, c.field(base, k)});
            check("CutState", f, c.bytes(), (4 + 9 * MB) * 4, b.p);
            expect(c.field(base, 3, MB - 1) == base + 4 + 3 * MB + MB - 1, "CutState", "field(f, k)");
            expect(CutState::kActive == 0 && CutState::kChanged == 1 && CutState::kMaxNcut == 2 && CutState::kNeedTab == 3,
                   "CutState", "counter indices");
            expect(CutState::kStateFields == 7 && CutState::kRowsAfter == 7 && CutState::kDropped == 8, "CutState", "field indices");
        }
        for (size_t per : pers) {
            const ParentBlock p(MB, per);
            Buf b(p.bytes());
            const auto v = p.view(b.p);
            check("ParentBlock", {{"par_d", p.par_d, 8, 2 * MB, v.par_d}, {"par_i", p.par_i, 4, 4 * MB, v.par_i},
                                  {"budget", p.budget, 4, per * MB, v.budget}},
                  p.bytes(), 2 * MB * 8 + (4 * MB + per * MB) * 4, b.p);
            for (size_t n : caps) {   // the table block of n columns: tab_off2 + 8 n + 32 n (mipx_tree_create_ex)
                const size_t tab_bytes = (17 * n + 7) / 8 * 8 + 8 * n + 32 * n;
                const FinishBlock fb(tab_bytes, per, MB, open_size);
                Buf fbuf(fb.bytes());
                const auto fv = fb.view(fbuf.p);
                check("FinishBlock", {{"summary", fb.summary, 8, 16, fv.summary}, {"table", fb.table, 8, tab_bytes / 8, fv.table},
                                      {"open", fb.open, open_size, per * MB, fv.open}, {"dead", fb.dead, 4, per * MB, fv.dead}},
                      fb.bytes(), 128 + (tab_bytes + 31) / 32 * 32 + per * MB * (open_size + 4), fbuf.p);
                expect(fb.summary == 0 && fb.table == 128, "FinishBlock", "summary at 0, table at 128");
            }
        }
        for (size_t cap : {caps[0], caps[1], MB}) {
            const HeurOut h(cap);
            Buf hb(h.bytes());
            const auto hv = h.view(hb.p);
            check("HeurOut", {{"obj", h.obj, 8, cap, hv.obj}, {"status", h.status, 4, cap, hv.status}, {"moves", h.moves, 4, 2 * cap, hv.moves}},
                  h.bytes(), cap * 20, hb.p);
            const PropOut p(cap);
            Buf pb(p.bytes());
            const auto pv = p.view(pb.p);
            check("PropOut", {{"status", p.status, 4, cap, pv.status}, {"changed", p.changed, 4, cap, pv.changed},
                              {"rounds", p.rounds, 4, cap, pv.rounds}, {"capped", p.capped, 4, cap, pv.capped}},
                  p.bytes(), cap * 16, pb.p);
            const PairList l(cap);
            Buf lb(l.bytes());
            const auto lv = l.view(lb.p);
            check("PairList", {{"parent_slot", l.parent_slot, 4, cap, lv.parent_slot}, {"parent_pos", l.parent_pos, 4, cap, lv.parent_pos},
                               {"var", l.var, 4, cap, lv.var}, {"child_slot", l.child_slot, 4, 2 * cap, lv.child_slot}},
                  l.bytes(), cap * 20, lb.p);
        }
    }
    // a view of a read-only buffer is read-only
    static_assert(std::is_same<decltype(HeurOut(1).view((const char *)nullptr).obj), const double *>::value, "const view");
    std::printf("step_layout: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
