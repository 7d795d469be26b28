// Host-only tables of a closed-form topology handle (not part of the public ABI): everything eg_topo_create uploads, built by
// plain arithmetic over Topo with no HIP call, so that a CPU program can look at it (tests/native/topo_tables_check.cpp).
#pragma once
#include <vector>

#include "common.h"

namespace eg {

struct TopoTables {
    std::vector<float> dis;                  // [n_nodes] (deg + 1)^-1/2
    std::vector<TileDesc> tiles;             // 2-D patch table of one frame, pyramid order
    std::vector<SegDesc> segs;               // [8 * tiles] per-segment descriptors
    std::vector<float> pats;                 // [n_pats * 128] distinct weight patterns
    std::vector<float> patsq;                // [n_pats * 64] the same patterns in quad layout
    std::vector<int> conn_table;             // [conn_chunks][4] = {level index, first row, rows, 0}
    std::vector<int> h_rowptr, h_colidx;     // hybrid topologies: the CSR of one frame (empty otherwise)
    int conn_chunks = 0;
    int n_pats = 0;
    int kid_rows = 0;                        // rows per frame of the child-sum side buffer, 0 when the topology does not qualify
    int flat = 0;                            // eg_graph::flat
    int hybrid = 0;                          // eg_graph::hybrid
};

// EG_OK, or EG_ERR_ARG / EG_ERR_UNSUPPORTED with the message set
int build_topo(int frame, int naux, int main_only, int coord_nodes, int conn_nodes, int diag_main, int diag_aux, Topo& T);
int build_topo_tables(const Topo& T, TopoTables& out);

}  // namespace eg
