// Stand-alone check of the records in simple_mip_solver_amd/csrc/finish_records.h (built and run by
// tests/test_finish_abi.py) against the NumPy dtypes of simple_mip_solver_amd/_ffi.py: the test passes, per record,
// its name, the dtype's item size and the offset of every field in declaration order; each must be the struct's sizeof
// and offsetof.
//   finish_layout_check OpenEntry 32 0 8 16 20 24 28  PcSample 32 0 4 8 16 24  FinishSummary 128 0 4 ... 80
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "finish_records.h"

using namespace mipx;

static int g_fail = 0, g_checks = 0;

static void expect(bool ok, const char *record, const char *what, long want, long got) {
    g_checks++;
    if (!ok && g_fail++ < 20) std::fprintf(stderr, "FAIL %s: %s is %ld in the struct, %ld in the dtype\n", record, what, want, got);
}

static void check(const char *record, size_t size, const std::vector<std::pair<const char *, size_t>> &fields, char **&arg, char **end) {
    if (arg == end) { g_checks++; g_fail++; std::fprintf(stderr, "FAIL %s: no item size given\n", record); return; }
    const long got_size = std::atol(*arg++);
    expect(got_size == (long)size, record, "sizeof", (long)size, got_size);
    for (const auto &f : fields) {
        if (arg == end) { g_checks++; g_fail++; std::fprintf(stderr, "FAIL %s: no offset given for %s\n", record, f.first); return; }
        const long got = std::atol(*arg++);
        expect(got == (long)f.second, record, f.first, (long)f.second, got);
    }
}

int main(int argc, char **argv) {
    char **arg = argv + 1, **end = argv + argc;
    int records = 0;
    while (arg != end) {
        const char *name = *arg++;
        records++;
        if (!std::strcmp(name, "OpenEntry"))
            check(name, sizeof(OpenEntry),
                  {{"key", offsetof(OpenEntry, key)}, {"bval", offsetof(OpenEntry, bval)}, {"slot", offsetof(OpenEntry, slot)},
                   {"depth", offsetof(OpenEntry, depth)}, {"bidx_dir", offsetof(OpenEntry, bidx_dir)},
                   {"anchor", offsetof(OpenEntry, anchor)}}, arg, end);
        else if (!std::strcmp(name, "PcSample"))
            check(name, sizeof(PcSample),
                  {{"var_dir", offsetof(PcSample, var_dir)}, {"status", offsetof(PcSample, status)}, {"obj", offsetof(PcSample, obj)},
                   {"bound", offsetof(PcSample, bound)}, {"vc", offsetof(PcSample, vc)}}, arg, end);
        else if (!std::strcmp(name, "FinishSummary"))
            check(name, sizeof(FinishSummary),
                  {{"host_path", offsetof(FinishSummary, host_path)}, {"n_open", offsetof(FinishSummary, n_open)},
                   {"n_dead", offsetof(FinishSummary, n_dead)}, {"n_samples", offsetof(FinishSummary, n_samples)},
                   {"unbounded", offsetof(FinishSummary, unbounded)}, {"incumbent_pos", offsetof(FinishSummary, incumbent_pos)},
                   {"n_deferred", offsetof(FinishSummary, n_deferred)}, {"pad0", offsetof(FinishSummary, pad0)},
                   {"evaluated", offsetof(FinishSummary, evaluated)}, {"dives", offsetof(FinishSummary, dives)},
                   {"pivots", offsetof(FinishSummary, pivots)}, {"closed_min", offsetof(FinishSummary, closed_min)},
                   {"primal", offsetof(FinishSummary, primal)}, {"primal_before", offsetof(FinishSummary, primal_before)},
                   {"pad", offsetof(FinishSummary, pad)}}, arg, end);
        else {
            g_checks++; g_fail++;
            std::fprintf(stderr, "FAIL: unknown record %s\n", name);
            break;
        }
    }
    if (records != 3) { g_fail++; std::fprintf(stderr, "FAIL: %d records given, 3 expected\n", records); }
    std::printf("finish_layout: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
