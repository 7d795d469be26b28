// Host-side check of the closed-form topology tables under AddressSanitizer + UBSan (CPU only; built and run by
// tests/test_topo_tables.py).  Calls build_topo / build_topo_tables (csrc/topo_tables.h) directly -- no handle, no device -- for
// every configuration of the input file, prints a digest line per configuration (compared with tests/golden/topo_tables.json by
// the pytest side) and checks the invariants the layer kernels rely on.
// Input (argv[1]): per configuration one line "frame naux main_only coord conn diag_main diag_aux n_nodes deg[0] .. deg[n_nodes - 1]",
// the degrees (no self loop) counted from echoglad_amd/topology.py's edge list.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "../../echoglad_amd/csrc/topo_tables.h"

using namespace eg;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { std::printf("FAIL: " __VA_ARGS__); std::printf("\n"); ++failures; } } while (0)

static unsigned long long fnv1a(const void* p, size_t n) {
    unsigned long long h = 0xcbf29ce484222325ull;
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}

template <class V>
static void digest(const char* name, const V& v) {
    std::printf(" %s %zu %016llx", name, v.size(), fnv1a(v.data(), v.size() * sizeof(v[0])));
}

// the patches cover every node of the frame exactly once
static void check_cover(const Topo& T, const TopoTables& tt) {
    std::vector<int> hits((size_t)T.n_nodes, 0);
    for (const TileDesc& td : tt.tiles) {
        EXPECT(td.level >= 0 && td.level < T.n_desc, "patch level %d", td.level);
        const LevelDesc& d = T.desc[td.level];
        for (int tr = 0; tr < td.nrows; ++tr)
            for (int u = 0; u < td.ncols; ++u) {
                const int n = d.base + (td.r0 + tr) * d.side + td.c0 + u;
                EXPECT(n >= d.base && n < d.end, "patch node %d outside its level [%d, %d)", n, d.base, d.end);
                if (n >= 0 && n < T.n_nodes) ++hits[(size_t)n];
            }
    }
    int bad = 0;
    for (int n = 0; n < T.n_nodes; ++n) bad += hits[(size_t)n] != 1;
    EXPECT(bad == 0, "%d nodes are not covered exactly once", bad);
}

static void check_segments(const Topo& T, const TopoTables& tt) {
    EXPECT(tt.segs.size() == 8 * tt.tiles.size(), "segs.size() %zu != 8 * %zu", tt.segs.size(), tt.tiles.size());
    EXPECT(tt.n_pats >= 1 && tt.pats.size() == (size_t)128 * tt.n_pats, "pats.size() %zu, n_pats %d", tt.pats.size(), tt.n_pats);
    EXPECT(tt.patsq.size() == (size_t)64 * tt.n_pats, "patsq.size() %zu, n_pats %d", tt.patsq.size(), tt.n_pats);
    if (tt.segs.size() != 8 * tt.tiles.size()) return;
    const int hi8 = T.n_nodes - 8, last = T.n_nodes - 1;
    for (size_t i = 0; i < tt.segs.size(); ++i) {
        const SegDesc& s = tt.segs[i];
        EXPECT(s.pat >= 0 && s.pat < tt.n_pats, "segment %zu: pat %d of %d", i, s.pat, tt.n_pats);
        // the consumers' epilogue addresses rows n_first .. n_first + cnt - 1; its running-maximum form reads and writes them through
        // plain pointers (no buffer descriptor drops a row outside the frame) and repeats segment 0 of the patch for an absent one
        EXPECT(s.cnt >= 0 && s.cnt <= 8, "segment %zu: cnt %d", i, s.cnt);
        if (s.cnt > 0) EXPECT(s.n_first >= 0 && s.n_first + s.cnt <= T.n_nodes, "segment %zu: rows %d .. + %d outside the frame", i, s.n_first, s.cnt);
        if (i % 8 == 0) EXPECT(s.cnt > 0, "patch %zu: segment 0 holds no node", i / 8);
        if (s.mode != 1) continue;
        for (int v : {s.up0, s.down0, s.par0, s.c0, s.c1, s.c2, s.c3}) EXPECT(v >= 0 && v <= hi8, "segment %zu: run base %d outside [0, %d]", i, v, hi8);
        for (int v : {s.left, s.right}) EXPECT(v >= 0 && v <= last, "segment %zu: edge row %d outside [0, %d]", i, v, last);
    }
    if (tt.kid_rows <= 0) return;
    // a pair of aux rows that reads child sums takes runs of 8 side-buffer rows from each row's first node
    for (size_t t = 0; t < tt.tiles.size(); ++t) {
        const LevelDesc& d = T.desc[tt.tiles[t].level];
        if (d.kind != KIND_AUX) continue;
        for (int tr = 0; tr < 8; tr += 2) {
            const SegDesc& sa = tt.segs[t * 8 + tr];
            const SegDesc& sb = tt.segs[t * 8 + tr + 1];
            if (!sa.pad0) continue;
            bool kids = false;
            for (const SegDesc* s : {&sa, &sb}) {
                const int idx = s->n_first - d.base, r = idx / d.side, c0 = idx - r * d.side;
                kids = kids || (r >= d.clo && r < d.chi && c0 < d.chi && c0 + 8 > d.clo);
            }
            if (kids) EXPECT(sa.n_first + 8 <= tt.kid_rows && sb.n_first + 8 <= tt.kid_rows, "patch %zu rows %d, %d: child-sum run past kid_rows %d (%d, %d)",
                             t, tr, tr + 1, tt.kid_rows, sa.n_first, sb.n_first);
        }
    }
}

static void check_dis(const TopoTables& tt, const std::vector<int>& deg) {
    EXPECT(tt.dis.size() == deg.size(), "dis.size() %zu != n_nodes %zu", tt.dis.size(), deg.size());
    if (tt.dis.size() != deg.size()) return;
    int bad = 0;
    for (size_t n = 0; n < deg.size(); ++n) {
        const float want = (float)(1.0 / std::sqrt((double)(deg[n] + 1)));
        bad += std::memcmp(&want, &tt.dis[n], sizeof(float)) != 0;
    }
    EXPECT(bad == 0, "dis differs from (float)(1 / sqrt(deg + 1)) at %d nodes", bad);
}

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: topo_tables_check <configurations file>\n"); return 2; }
    std::ifstream in(argv[1]);
    int a[7], n_nodes, n_cfg = 0;
    while (in >> a[0] >> a[1] >> a[2] >> a[3] >> a[4] >> a[5] >> a[6] >> n_nodes) {
        std::vector<int> deg((size_t)(n_nodes > 0 ? n_nodes : 0));
        for (int& d : deg) in >> d;
        if (!in) { std::printf("FAIL: truncated input\n"); return 2; }
        ++n_cfg;
        std::printf("cfg %d %d %d %d %d %d %d", a[0], a[1], a[2], a[3], a[4], a[5], a[6]);
        Topo T;
        TopoTables tt;
        if (build_topo(a[0], a[1], a[2], a[3], a[4], a[5], a[6], T) != EG_OK || build_topo_tables(T, tt) != EG_OK) {
            std::printf(" REJECTED\n");
            ++failures;
            continue;
        }
        digest("dis", tt.dis); digest("tiles", tt.tiles); digest("segs", tt.segs); digest("pats", tt.pats); digest("patsq", tt.patsq);
        digest("conn_table", tt.conn_table); digest("h_rowptr", tt.h_rowptr); digest("h_colidx", tt.h_colidx);
        std::printf(" n_pats %d kid_rows %d flat %d hybrid %d conn_chunks %d\n", tt.n_pats, tt.kid_rows, tt.flat, tt.hybrid, tt.conn_chunks);
        EXPECT(T.n_nodes == n_nodes, "n_nodes %d, topology.py says %d", T.n_nodes, n_nodes);
        check_cover(T, tt);
        check_segments(T, tt);
        check_dis(tt, deg);
    }
    std::printf("topo_tables_check: %d failure(s) over %d configurations\n", failures, n_cfg);
    return failures ? 1 : 0;
}
