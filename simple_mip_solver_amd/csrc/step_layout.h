// step_layout.h -- the packed buffers that carry a step of the tree engine between device and host, each
// defined once.  A layout takes the dimensions that fix it, holds the byte offset of every field (public, in
// field order) and gives bytes(); view(base) returns typed pointers into any base address, so allocation, the
// device launch and the host read-back share one piece of arithmetic.  Plain C++17, no HIP: fields that hold a
// kernel struct (a probe request, an open entry, the finish summary) are byte pointers and their element size
// comes in as an argument (tree_engine.hip.h ties those arguments to the kernel types).
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace step_layout {

// T with the constness of Base: a view of a const buffer is read-only
template <class T, class Base> using Like = std::conditional_t<std::is_const<Base>::value, const T, T>;
template <class T, class Base> Like<T, Base> *at(Base *base, size_t off) {
    return reinterpret_cast<Like<T, Base> *>(reinterpret_cast<Like<char, Base> *>(base) + off);
}
inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Step read-back (d_pack / h_pack), ONE copy per step: per output position (levels x max_batch: the batch, then
// its dive children level by level) [obj | bval], per dive decision ((levels - 1 or 1) x max_batch) [dval], then
// [status | bidx | mipf | nprobe | npiv] and [dvar | ddir] likewise, then on a 16-byte boundary the probe
// requests: a 16-byte slot for their counter and ask_cap entries of ask_size bytes.
struct StepPack {
    size_t obj, bval, dval, status, bidx, mipf, nprobe, npiv, dvar, ddir, ask_count, ask, end;
    StepPack(size_t levels, size_t max_batch, size_t ask_cap, size_t ask_size) {
        const size_t OB = levels * max_batch, DB = (levels > 1 ? levels - 1 : 1) * max_batch;
        obj = 0; bval = obj + 8 * OB; dval = bval + 8 * OB;
        status = dval + 8 * DB; bidx = status + 4 * OB; mipf = bidx + 4 * OB; nprobe = mipf + 4 * OB; npiv = nprobe + 4 * OB;
        dvar = npiv + 4 * OB; ddir = dvar + 4 * DB;
        ask_count = round_up(ddir + 4 * DB, 16); ask = ask_count + 16; end = ask + ask_cap * ask_size;
    }
    size_t bytes() const { return end; }
    template <class Base> struct View {
        Like<double, Base> *obj, *bval, *dval;
        Like<int32_t, Base> *status, *bidx, *mipf, *nprobe, *npiv, *dvar, *ddir, *ask_count;
        Like<char, Base> *ask;
    };
    template <class Base> View<Base> view(Base *b) const {
        return {at<double>(b, obj), at<double>(b, bval), at<double>(b, dval), at<int32_t>(b, status), at<int32_t>(b, bidx),
                at<int32_t>(b, mipf), at<int32_t>(b, nprobe), at<int32_t>(b, npiv), at<int32_t>(b, dvar), at<int32_t>(b, ddir),
                at<int32_t>(b, ask_count), at<char>(b, ask)};
    }
};

// Cut-round state on the host (h_cs), int32: the round's four counters, then nine per-node fields of max_batch
// entries each -- the seven state fields the device keeps behind one another (rounds and the six GMIC counters),
// the cut rows the node ends with, and the cuts it dropped.
struct CutState {
    enum Counter { kActive = 0, kChanged = 1, kMaxNcut = 2, kNeedTab = 3, kCounters = 4 };
    enum Field { kStateFields = 7, kRowsAfter = 7, kDropped = 8, kFields = 9 };
    size_t max_batch;
    explicit CutState(size_t max_batch_) : max_batch(max_batch_) {}
    size_t bytes() const { return (kCounters + kFields * max_batch) * 4; }
    template <class I> I *counters(I *base) const { return base; }
    template <class I> I *field(I *base, int f, size_t k = 0) const { return base + kCounters + (size_t)f * max_batch + k; }
};

// Parent block (d_par / h_par) of a device-finished step of B nodes: [par_d: dual_bound | b_val] (f64),
// [par_i: b_idx | b_dir | depth | anchor] (i32), [budget: per pool rows per node] (i32).
struct ParentBlock {
    size_t par_d, par_i, budget, end;
    ParentBlock(size_t B, size_t per) : par_d(0), par_i(2 * B * 8), budget(par_i + 4 * B * 4), end(budget + per * B * 4) {}
    size_t bytes() const { return end; }
    template <class Base> struct View { Like<double, Base> *par_d; Like<int32_t, Base> *par_i, *budget; };
    template <class Base> View<Base> view(Base *b) const { return {at<double>(b, par_d), at<int32_t>(b, par_i), at<int32_t>(b, budget)}; }
};

// Device-finish block on the host (h_fin): the summary, the table block at 128, then on a 32-byte boundary
// per x max_batch open entries of open_size bytes and as many dead rows (i32).
struct FinishBlock {
    size_t summary, table, open, dead, end;
    FinishBlock(size_t tab_bytes, size_t per, size_t max_batch, size_t open_size)
        : summary(0), table(128), open(table + round_up(tab_bytes, 32)), dead(open + per * max_batch * open_size),
          end(dead + per * max_batch * 4) {}
    size_t bytes() const { return end; }
    template <class Base> struct View { Like<char, Base> *summary, *table, *open; Like<int32_t, Base> *dead; };
    template <class Base> View<Base> view(Base *b) const { return {at<char>(b, summary), at<char>(b, table), at<char>(b, open), at<int32_t>(b, dead)}; }
};

// Primal heuristic output, cap points: [obj] (f64) [status] (i32) [moves: repair, lift per point] (i32).
struct HeurOut {
    size_t obj, status, moves, end;
    explicit HeurOut(size_t cap) : obj(0), status(8 * cap), moves(status + 4 * cap), end(moves + 8 * cap) {}
    size_t bytes() const { return end; }
    template <class Base> struct View { Like<double, Base> *obj; Like<int32_t, Base> *status, *moves; };
    template <class Base> View<Base> view(Base *b) const { return {at<double>(b, obj), at<int32_t>(b, status), at<int32_t>(b, moves)}; }
};

// Local search output behind the heuristic's, cap points: [status] (i32) [moves: singles, pairs per point] (i32).
struct LsOut {
    size_t status, moves, end;
    explicit LsOut(size_t cap) : status(0), moves(4 * cap), end(12 * cap) {}
    size_t bytes() const { return end; }
    template <class Base> struct View { Like<int32_t, Base> *status, *moves; };
    template <class Base> View<Base> view(Base *b) const { return {at<int32_t>(b, status), at<int32_t>(b, moves)}; }
};

// Fix-and-propagate dive output behind the heuristic's, cap points: [obj] (f64: the dive's, then the lifted one)
// [status] (i32) [counts: fixings, tries per point] (i32), what the heuristic's second pass over the dive's feasible
// points gives [lift_status | lift_moves: repair, lift per point] (i32), and what the local search gives on those
// [ls_status | ls_moves: singles, pairs per point] (i32).
struct FpOut {
    size_t obj, status, counts, lift_status, lift_moves, ls_status, ls_moves, end;
    explicit FpOut(size_t cap)
        : obj(0), status(8 * cap), counts(status + 4 * cap), lift_status(counts + 8 * cap), lift_moves(lift_status + 4 * cap),
          ls_status(lift_moves + 8 * cap), ls_moves(ls_status + 4 * cap), end(ls_moves + 8 * cap) {}
    size_t bytes() const { return end; }
    template <class Base> struct View {
        Like<double, Base> *obj;
        Like<int32_t, Base> *status, *counts, *lift_status, *lift_moves, *ls_status, *ls_moves;
    };
    template <class Base> View<Base> view(Base *b) const {
        return {at<double>(b, obj), at<int32_t>(b, status), at<int32_t>(b, counts), at<int32_t>(b, lift_status),
                at<int32_t>(b, lift_moves), at<int32_t>(b, ls_status), at<int32_t>(b, ls_moves)};
    }
};

// Weighted row repair output behind the heuristic's, cap points: [obj] (f64: the repaired point's, then the lifted
// one) [status] (i32) [counts: moves, bumps per point] (i32), what the heuristic's second pass over the feasible ones
// gives [lift_status | lift_moves: repair, lift per point] (i32), and what the local search gives on those
// [ls_status | ls_moves: singles, pairs per point] (i32).
struct WrOut {
    size_t obj, status, counts, lift_status, lift_moves, ls_status, ls_moves, end;
    explicit WrOut(size_t cap)
        : obj(0), status(8 * cap), counts(status + 4 * cap), lift_status(counts + 8 * cap), lift_moves(lift_status + 4 * cap),
          ls_status(lift_moves + 8 * cap), ls_moves(ls_status + 4 * cap), end(ls_moves + 8 * cap) {}
    size_t bytes() const { return end; }
    template <class Base> struct View {
        Like<double, Base> *obj;
        Like<int32_t, Base> *status, *counts, *lift_status, *lift_moves, *ls_status, *ls_moves;
    };
    template <class Base> View<Base> view(Base *b) const {
        return {at<double>(b, obj), at<int32_t>(b, status), at<int32_t>(b, counts), at<int32_t>(b, lift_status),
                at<int32_t>(b, lift_moves), at<int32_t>(b, ls_status), at<int32_t>(b, ls_moves)};
    }
};

// Cube search output beside the heuristic's, cap points (the points themselves lie in a block of their own, not in
// the heuristic's slots): [obj] (f64: the picked code's, then the lifted one) [status] (i32) [counts: k, code per
// point] (i32), what the heuristic's pass over the FOUND points gives [lift_status | lift_moves: repair, lift per
// point] (i32), and what the local search gives on those [ls_status | ls_moves: singles, pairs per point] (i32).
struct CubeOut {
    size_t obj, status, counts, lift_status, lift_moves, ls_status, ls_moves, end;
    explicit CubeOut(size_t cap)
        : obj(0), status(8 * cap), counts(status + 4 * cap), lift_status(counts + 8 * cap), lift_moves(lift_status + 4 * cap),
          ls_status(lift_moves + 8 * cap), ls_moves(ls_status + 4 * cap), end(ls_moves + 8 * cap) {}
    size_t bytes() const { return end; }
    template <class Base> struct View {
        Like<double, Base> *obj;
        Like<int32_t, Base> *status, *counts, *lift_status, *lift_moves, *ls_status, *ls_moves;
    };
    template <class Base> View<Base> view(Base *b) const {
        return {at<double>(b, obj), at<int32_t>(b, status), at<int32_t>(b, counts), at<int32_t>(b, lift_status),
                at<int32_t>(b, lift_moves), at<int32_t>(b, ls_status), at<int32_t>(b, ls_moves)};
    }
};

// Completion output (include/mipx_complete.h), room for two blocks of cap points: [obj] (f64) [status] (i32) [pivots]
// (i32), 2 cap entries each.  A step of P <= cap points uses the first P entries of a field for the heuristic's block
// and, with the cube search on, the next P for the cube's (the launch's positions).  The completed points
// themselves lie in a block of their own, in the same order.
struct CompOut {
    size_t obj, status, pivots, end;
    explicit CompOut(size_t cap) : obj(0), status(16 * cap), pivots(status + 8 * cap), end(pivots + 8 * cap) {}
    size_t bytes() const { return end; }
    template <class Base> struct View {
        Like<double, Base> *obj;
        Like<int32_t, Base> *status, *pivots;
    };
    template <class Base> View<Base> view(Base *b) const {
        return {at<double>(b, obj), at<int32_t>(b, status), at<int32_t>(b, pivots)};
    }
};

// Bound propagation output, cap nodes: [status | changed | rounds | capped], i32 each.
struct PropOut {
    size_t status, changed, rounds, capped, end;
    explicit PropOut(size_t cap) : status(0), changed(4 * cap), rounds(8 * cap), capped(12 * cap), end(16 * cap) {}
    size_t bytes() const { return end; }
    template <class Base> struct View { Like<int32_t, Base> *status, *changed, *rounds, *capped; };
    template <class Base> View<Base> view(Base *b) const {
        return {at<int32_t>(b, status), at<int32_t>(b, changed), at<int32_t>(b, rounds), at<int32_t>(b, capped)};
    }
};

// Reduced-cost tightening of a step, levels x max_batch branching parents (level p's at p * max_batch ..), i32:
// what goes up [slot | pos] (the parents' pool rows and output positions), what comes down [status | changed].
struct RcOut {
    size_t max_batch, slot, pos, status, changed, end;
    RcOut(size_t levels, size_t max_batch_)
        : max_batch(max_batch_), slot(0), pos(4 * levels * max_batch_), status(8 * levels * max_batch_),
          changed(12 * levels * max_batch_), end(16 * levels * max_batch_) {}
    size_t bytes() const { return end; }
    size_t in_bytes() const { return status; }             // the lists, in front
    size_t level(size_t p) const { return p * max_batch; } // first entry of level p in every field
    template <class Base> struct View { Like<int32_t, Base> *slot, *pos, *status, *changed; };
    template <class Base> View<Base> view(Base *b) const {
        return {at<int32_t>(b, slot), at<int32_t>(b, pos), at<int32_t>(b, status), at<int32_t>(b, changed)};
    }
};

// Branching list of count parents, i32: [parent_slot | parent_pos | var | child_slot (left, right per parent)].
struct PairList {
    size_t parent_slot, parent_pos, var, child_slot, end;
    explicit PairList(size_t count) : parent_slot(0), parent_pos(4 * count), var(8 * count), child_slot(12 * count), end(20 * count) {}
    size_t bytes() const { return end; }
    template <class Base> struct View { Like<int32_t, Base> *parent_slot, *parent_pos, *var, *child_slot; };
    template <class Base> View<Base> view(Base *b) const {
        return {at<int32_t>(b, parent_slot), at<int32_t>(b, parent_pos), at<int32_t>(b, var), at<int32_t>(b, child_slot)};
    }
};

}  // namespace step_layout
