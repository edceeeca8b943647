// finish_records.h -- the records the device finish hands to the host (finish_kernels.hip.h): plain structs, no
// HIP, so that host-compiled code can see them (tests/support/finish_layout_check.cpp checks sizeof and offsetof
// against the NumPy dtypes of simple_mip_solver_amd/_ffi.py).
#pragma once
#include <stdint.h>

namespace mipx {

struct OpenEntry {       // one new open node, as the host's queue and node table need it
    double key;          // its inherited bound (the parent's LP objective)
    double bval;
    int32_t slot, depth, bidx_dir, anchor;   // bidx_dir = 2 * branching variable + direction
};
static_assert(sizeof(OpenEntry) == 32, "OpenEntry layout");

struct PcSample {        // one pseudo-cost update (pseudo_cost.py:68-100), in the order they are applied
    int32_t var_dir;     // 2 * variable + direction (0 left, 1 right)
    int32_t status;      // LP status of the child the sample comes from
    double obj, bound, vc;   // its objective, its parent's bound, the variable change
};
static_assert(sizeof(PcSample) == 32, "PcSample layout");

struct FinishSummary {
    int32_t host_path;           // 1: probe requests were filed -- the host path finishes the step
    int32_t n_open, n_dead, n_samples;
    int32_t unbounded, incumbent_pos;   // output position of the step's best improving integral node, -1: none
    int32_t n_deferred, pad0;           // nodes that filed probe requests: left to the host, after everything else
    int64_t evaluated, dives, pivots;
    double closed_min, primal;   // lowest value among the step's closed leaves; the incumbent value after the step
    double primal_before;        // ... and before it: what the step's decisions compared against
    int64_t pad[6];
};
static_assert(sizeof(FinishSummary) == 128, "FinishSummary layout");

}  // namespace mipx
