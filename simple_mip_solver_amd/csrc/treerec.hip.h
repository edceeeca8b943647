// treerec.hip.h -- state of the tree record (include/mipx_treerec.h).  Included by tree_engine.hip.h in front
// of mipx_tree; the host side that needs the tree is in treerec_api.hip.h.
//
// Per node id, beside the node table's NodeRec: parent, LP verdict, flags, objective -- 14 bytes, vectors that
// exist only while recording is on (NodeRec keeps its size).  The device mirror (TrNode, 16 bytes per node)
// is append-only: a query uploads the entries created since the last one.

struct TreeRec {
    bool on = false;
    std::vector<int32_t> parent;      // per node id (-1 root)
    std::vector<int8_t> status;       // -1 never solved, else the node LP's Clp code
    std::vector<uint8_t> flags;       // MIPX_TR_MIP_FEASIBLE | HAS_CHILDREN | CLOSED_AT_POP | PROBED (OPEN is derived)
    std::vector<double> obj;
    std::vector<int8_t> root_v;       // the root's optimal basis codes (n + m), kept once
    bool have_root = false;
    // device mirror and the root's rows
    mipx::TrNode *d_nodes = nullptr;
    int64_t d_cap = 0, d_count = 0;
    double *d_root = nullptr;         // [l | u]
    int8_t *d_root_v = nullptr;
    bool root_v_up = false;
    // the last query's ids and bounds stay on the device; the re-solve's block beside them
    int64_t *d_ids = nullptr;
    double *d_l = nullptr, *d_u = nullptr;
    int64_t qcap = 0;
    char *d_solve = nullptr;
    size_t solve_bytes = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int64_t materialised = 0, resolved = 0;
    double query_us = 0.0;

    void root() { parent.assign(1, -1); status.assign(1, -1); flags.assign(1, 0); obj.assign(1, 0.0); }
    void child(int64_t of) {
        parent.push_back((int32_t)of); status.push_back(-1); flags.push_back(0); obj.push_back(0.0);
        flags[(size_t)of] |= MIPX_TR_HAS_CHILDREN;
    }
    void solved(int64_t id, int st, double o, bool mipf, bool probed) {
        status[(size_t)id] = (int8_t)st;
        obj[(size_t)id] = o;
        flags[(size_t)id] |= (uint8_t)((mipf && (st == 0 || st == 2) ? MIPX_TR_MIP_FEASIBLE : 0) | (probed ? MIPX_TR_PROBED : 0));
    }
    void closed(int64_t id) { flags[(size_t)id] |= MIPX_TR_CLOSED_AT_POP; }
};
