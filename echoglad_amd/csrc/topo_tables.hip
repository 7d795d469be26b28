// Host-only half of a closed-form topology handle: the level descriptors (build_topo) and every table the layer kernels read
// (build_topo_tables).  No kernel and no HIP call in this file; graph.hip uploads what it builds.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <map>
#include <vector>

#include "topo_tables.h"

namespace eg {

#ifdef EG_DEBUG_TOPO
#define EG_DEBUG_TOPO_ON 1          // -DEG_DEBUG_TOPO: why a handle has no child-sum side buffer, on stderr
#else
#define EG_DEBUG_TOPO_ON 0
#endif

// Python floor division
static inline int floordiv(int a, int b) {
    int q = a / b;
    if ((a % b != 0) && ((a < 0) != (b < 0))) --q;
    return q;
}

// Python `range(len)[start:stop]` with step 1 -> [lo, hi)
static inline void py_slice(int len, int start, int stop, int& lo, int& hi) {
    lo = start < 0 ? (len + start < 0 ? 0 : len + start) : (start > len ? len : start);
    hi = stop < 0 ? (len + stop < 0 ? 0 : len + stop) : (stop > len ? len : stop);
    if (hi < lo) hi = lo;
}

int build_topo(int frame, int naux, int main_only, int coord_nodes, int conn_nodes, int diag_main, int diag_aux, Topo& T) {
    if (frame < 2 || frame > 4096) return set_error(EG_ERR_ARG, "frame must be in [2, 4096]");
    if (!main_only && (naux < 1 || naux + 1 > MAX_LEVELS)) return set_error(EG_ERR_ARG, "naux out of range");
    T = Topo{};
    T.n_aux = main_only ? 0 : naux;
    T.n_conn = (!main_only && conn_nodes) ? naux + 1 : 0;     // datasets.py:1450-1456: only inside `if not use_main_graph_only`
    int nid = T.n_conn;
    T.diag_main = diag_main ? 1 : 0;
    T.diag_aux = (!main_only && diag_aux) ? 1 : 0;
    for (int k = 1; k <= T.n_aux; ++k) {
        T.base[k - 1] = nid;
        T.side[k - 1] = 1 << k;
        nid += (1 << k) * (1 << k);
    }
    T.n_levels = T.n_aux + 1;
    T.base[T.n_levels - 1] = nid;
    T.side[T.n_levels - 1] = frame;
    nid += frame * frame;
    T.coord_base = nid;
    if (!main_only && coord_nodes) nid += 4;       // datasets.py:1508-1523: only inside `if not use_main_graph_only`
    T.n_nodes = nid;
    T.frame = frame;
    T.magic = ((1ull << 40) / (unsigned long long)frame) + 1ull;
    if ((long long)frame * frame >= (1ll << 24)) return set_error(EG_ERR_UNSUPPORTED, "frame too large");
    T.crop0 = 0; T.ncrop = 0;
    if (T.n_aux > 0) {                             // datasets.py:1565-1567, Python slice semantics
        const int p = 1 << T.n_aux;
        const int half = frame / 2;
        const int c0 = floordiv(p - half, 2);
        int lo, hi;
        py_slice(p, c0, c0 + half, lo, hi);
        T.crop0 = lo; T.ncrop = hi - lo;
    }
    // per-level descriptors for the run-based stencil
    T.n_desc = T.n_levels + (T.coord_base < T.n_nodes ? 1 : 0);
    for (int l = 0; l < T.n_levels; ++l) {
        LevelDesc& d = T.desc[l];
        d = LevelDesc{};
        const bool is_main = (l == T.n_levels - 1);
        d.base = T.base[l];
        d.side = T.side[l];
        d.end = is_main ? T.coord_base : T.base[l + 1];
        d.kind = is_main ? 1 : 0;
        d.lg = is_main ? 0 : l + 1;
        if (is_main) {
            if (T.n_aux > 0) { d.pbase = T.base[l - 1]; d.pside = T.side[l - 1]; d.poff = T.crop0; d.plim = 2 * T.ncrop; }
        } else {
            if (l > 0) { d.pbase = T.base[l - 1]; d.pside = T.side[l - 1]; d.poff = 0; d.plim = d.side; }
            d.cbase = T.base[l + 1]; d.cside = T.side[l + 1];
            if (l + 1 < T.n_levels - 1) { d.clo = 0; d.chi = d.side; }
            else { d.clo = T.crop0; d.chi = T.crop0 + T.ncrop; }
        }
    }
    if (T.n_desc > T.n_levels) {
        LevelDesc& d = T.desc[T.n_levels];
        d = LevelDesc{};
        d.base = T.coord_base; d.end = T.n_nodes; d.side = 4; d.kind = 2;
    }
    if (T.n_conn > 0) {                            // the connection nodes' pseudo-level, 8 nodes per (pseudo) row
        if (T.n_desc + 1 > MAX_LEVELS + 1) return set_error(EG_ERR_ARG, "too many levels");
        LevelDesc& d = T.desc[T.n_desc];
        d = LevelDesc{};
        d.base = 0; d.end = T.n_conn; d.side = 8; d.kind = KIND_CONN;
        T.n_desc += 1;
    }
    return EG_OK;
}

static void topo_debug(const char* fmt, ...) {          // -DEG_DEBUG_TOPO only
    if (!EG_DEBUG_TOPO_ON) return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
}

// connection node wired to every node of level l (datasets.py:1512-1515: node g - 1 <-> aux level g, g = 1 .. naux - 1), or -1
static int hub_of_level(const Topo& T, int l) { return (T.n_conn > 0 && l <= T.n_aux - 2) ? l : -1; }

// whether level l is 'grid-diagonal'
static bool level_diag(const Topo& T, int l) { return l == T.n_levels - 1 ? T.diag_main != 0 : T.diag_aux != 0; }

// the up-to-4 diagonal neighbours of node n (datasets.py:1469-1475)
static int diag_ids(const Topo& T, int n, int (&out)[4]) {
    if (n >= T.coord_base || n < T.n_conn) return 0;
    const int l = level_of(T, n);
    if (!level_diag(T, l)) return 0;
    const int side = T.side[l], idx = n - T.base[l], r = idx / side, c = idx - r * side;
    int k = 0;
    for (int dr = -1; dr <= 1; dr += 2)
        for (int dc = -1; dc <= 1; dc += 2)
            if (r + dr >= 0 && r + dr < side && c + dc >= 0 && c + dc < side) out[k++] = n + dr * side + dc;
    return k;
}

// every neighbour of node n (no self loop), sorted: grid stencil + diagonals + the level's connection node; connection nodes:
// the other connection nodes + every node of their level
static void full_row(const Topo& T, int n, std::vector<int>& row) {
    row.clear();
    if (n < T.n_conn) {
        for (int h = 0; h < T.n_conn; ++h) if (h != n) row.push_back(h);
        if (n <= T.n_aux - 2)
            for (int j = T.base[n]; j < T.base[n + 1]; ++j) row.push_back(j);
        return;
    }
    Nbrs nb;
    neighbours(T, n, nb);
    for (int sl = 1; sl < nb.count; ++sl)
        if (nb.valid[sl]) row.push_back(nb.id[sl]);
    int dg[4];
    const int nd = diag_ids(T, n, dg);
    row.insert(row.end(), dg, dg + nd);
    if (n < T.coord_base) {
        const int hub = hub_of_level(T, level_of(T, n));
        if (hub >= 0) row.push_back(hub);
    }
    std::sort(row.begin(), row.end());
}

// (deg + 1)^-1/2 of every node.  Hybrid handles also carry the CSR of one frame (sorted by target, then source): every path but
// the producer/consumer kernel's stencil reads it (common.h eg_graph::hybrid)
static void build_degrees(const Topo& T, bool hybrid, std::vector<float>& dis, std::vector<int>& h_rowptr, std::vector<int>& h_colidx) {
    dis.resize(T.n_nodes);
    if (hybrid) h_rowptr.assign((size_t)T.n_nodes + 1, 0);
    std::vector<int> row;
    for (int n = 0; n < T.n_nodes; ++n) {
        full_row(T, n, row);
        dis[n] = (float)(1.0 / std::sqrt((double)(row.size() + 1)));
        if (!hybrid) continue;
        h_colidx.insert(h_colidx.end(), row.begin(), row.end());
        h_rowptr[(size_t)n + 1] = (int)h_colidx.size();
    }
}

// 2-D patch table.  Order = depth-first post-order over the pyramid of 8x8 patches: the patches under a
// coarse patch are emitted (recursively, 2x2 blocks) before it, so vertical neighbours, parents and
// children are worked on close in time by the workgroups of one XCD and meet in its L2.  Patches that
// the pyramid does not reach (outside the centre crop, or a main-only graph) follow in 2x2-block order.
struct PatchWalk {
    const Topo& T;
    std::vector<TileDesc>& tiles;
    std::vector<std::vector<char>> seen;      // [level][ty * tside + tx]: emitted, or on the stack
    std::vector<int> tside;                   // patches per side of each level

    PatchWalk(const Topo& T_, std::vector<TileDesc>& tiles_) : T(T_), tiles(tiles_), seen(T_.n_levels), tside(T_.n_levels) {
        for (int l = 0; l < T.n_levels; ++l) {
            tside[l] = (T.desc[l].side + 7) / 8;
            seen[l].assign((size_t)tside[l] * tside[l], 0);
        }
    }
    void push(int l, int ty, int tx) {
        const LevelDesc& d = T.desc[l];
        const int r0 = ty * 8, c0 = tx * 8;
        tiles.push_back(TileDesc{l, r0, c0, d.side - r0 < 8 ? d.side - r0 : 8, d.side - c0 < 8 ? d.side - c0 : 8, 0, 0, 0});
    }
    // the pyramid under patch (l0, ty0, tx0), post-order; explicit stack: (level, ty, tx, state)
    void visit(int l0, int ty0, int tx0) {
        struct Item { int l, ty, tx, expanded; };
        std::vector<Item> st;
        st.push_back(Item{l0, ty0, tx0, 0});
        while (!st.empty()) {
            Item it = st.back();
            st.pop_back();
            if (it.l < 0 || it.l >= T.n_levels || it.ty < 0 || it.tx < 0 || it.ty >= tside[it.l] || it.tx >= tside[it.l]) continue;
            char& sn = seen[it.l][(size_t)it.ty * tside[it.l] + it.tx];
            if (it.expanded) { push(it.l, it.ty, it.tx); continue; }
            if (sn) continue;
            sn = 1;
            st.push_back(Item{it.l, it.ty, it.tx, 1});
            const LevelDesc& d = T.desc[it.l];
            if (d.kind != 0) continue;                        // main grid: leaf
            // node range of the children of this patch, in the child level's coordinates
            const int rlo = 2 * (it.ty * 8 - d.clo), rhi = 2 * (it.ty * 8 + 8 - d.clo);
            const int clo = 2 * (it.tx * 8 - d.clo), chi = 2 * (it.tx * 8 + 8 - d.clo);
            const int cl = it.l + 1;
            const int climit = 2 * (d.chi - d.clo);
            const int r_a = rlo < 0 ? 0 : rlo, r_b = rhi > climit ? climit : rhi;
            const int c_a = clo < 0 ? 0 : clo, c_b = chi > climit ? climit : chi;
            if (r_a >= r_b || c_a >= c_b) continue;
            for (int ty = (r_b - 1) / 8; ty >= r_a / 8; --ty)        // reversed: the stack pops them in order
                for (int tx = (c_b - 1) / 8; tx >= c_a / 8; --tx) st.push_back(Item{cl, ty, tx, 0});
        }
    }
};

static void build_patch_order(const Topo& T, std::vector<TileDesc>& tiles) {
    PatchWalk walk(T, tiles);
    if (T.n_aux > 0) walk.visit(0, 0, 0);
    for (int l = 0; l < T.n_levels; ++l) {                    // whatever the pyramid did not reach: 2x2-block order
        const int ts = walk.tside[l];
        for (int by = 0; by < ts; by += 2)
            for (int bx = 0; bx < ts; bx += 2)
                for (int dy = 0; dy < 2; ++dy)
                    for (int dx = 0; dx < 2; ++dx) {
                        const int ty = by + dy, tx = bx + dx;
                        if (ty < ts && tx < ts && !walk.seen[l][(size_t)ty * ts + tx]) { walk.seen[l][(size_t)ty * ts + tx] = 1; walk.push(l, ty, tx); }
                    }
    }
    if (T.coord_base < T.n_nodes) {
        const LevelDesc& d = T.desc[T.n_levels];
        tiles.push_back(TileDesc{T.n_levels, 0, 0, 1, d.end - d.base, 0, 0, 0});
    }
    for (int h0 = 0; h0 < T.n_conn; h0 += 8)           // connection nodes: 8 per pseudo-tile (one segment each)
        tiles.push_back(TileDesc{T.n_desc - 1, h0 / 8, 0, 1, T.n_conn - h0 < 8 ? T.n_conn - h0 : 8, 0, 0, 0});
}

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The pattern of a fast segment: 64 + 64 lane weights, lane (u, s) -> valid(slot s of node u) ? (deg + 1)^-1/2 of that neighbour : 0,
// + {diagonal?, edge weights of the row above (l, r) and below (l, r)}.  (r, c0): the segment's first node in its level.
static void segment_pattern(const Topo& T, const std::vector<float>& dis, const LevelDesc& d, const SegDesc& sd, int r, int c0, bool ldiag,
                            std::vector<float>& w) {
    Nbrs nb;
    for (int lane = 0; lane < 64; ++lane) {
        const int u = lane >> 3, sl = lane & 7;
        const int n = sd.n_first + (u < sd.cnt ? u : sd.cnt - 1);
        neighbours(T, n, nb);
        w[lane] = nb.valid[sl] ? dis[nb.id[sl]] : 0.0f;
        const int sb = 8 + (sl & 1);
        w[64 + lane] = ((sd.aux & 1) && nb.valid[sb]) ? dis[nb.id[sb]] : 0.0f;
    }
    for (int e = 0; e < 5; ++e) w[128 + e] = 0.0f;
    if (ldiag) {                                // the nodes left / right of the 8-node runs above and below
        auto dnode = [&](int rr, int cc) { return (rr >= 0 && rr < d.side && cc >= 0 && cc < d.side) ? dis[d.base + rr * d.side + cc] : 0.0f; };
        w[128] = 1.0f;
        w[129] = dnode(r - 1, c0 - 1); w[130] = dnode(r - 1, c0 + 8);
        w[131] = dnode(r + 1, c0 - 1); w[132] = dnode(r + 1, c0 + 8);
    }
}

// Per-segment descriptors (8 per patch) and the table of distinct weight patterns (128 floats each in `pats`, 5 more in `pat_extra`).
// Interior segments of a level all share one pattern, so the table stays at a few dozen entries.  Patterns are numbered in the
// order a std::map over the 133 floats first meets them.
static void build_segments(const Topo& T, const std::vector<float>& dis, const std::vector<TileDesc>& tiles, std::vector<SegDesc>& segs,
                           std::vector<float>& pats, std::vector<float>& pat_extra) {
    segs.assign(tiles.size() * 8, SegDesc{});
    std::map<std::vector<float>, int> pat_index;
    const int n_frame = T.n_nodes, hi8 = n_frame - 8, last = n_frame - 1;
    std::vector<float> w(128 + 5);
    for (size_t t = 0; t < tiles.size(); ++t) {
        const TileDesc& td = tiles[t];
        const LevelDesc& d = T.desc[td.level];
        for (int tr = 0; tr < 8; ++tr) {
            SegDesc sd{};
            sd.n_first = d.base + (td.r0 + tr) * d.side + td.c0;
            sd.cnt = tr < td.nrows ? td.ncols : 0;
            const int idx = sd.n_first - d.base;
            const bool grid = d.kind == KIND_AUX || d.kind == KIND_MAIN;       // (not the coordinate / connection pseudo-levels)
            const int r = grid ? idx / d.side : 0;
            const int c0 = idx - r * d.side;
            const int cb = d.cbase + 2 * (r - d.clo) * d.cside + 2 * (c0 - d.clo);
            const bool kids = d.kind == KIND_AUX && r >= d.clo && r < d.chi && c0 < d.chi && c0 + 8 > d.clo;   // some node of the segment has children
            // per-node scalar path: coordinate K4, and segments so close to the end of the frame that a run of
            // 8 rows (self / below / children) would have to be clamped while some of its rows are real neighbours
            // (the rows below the LAST grid row are no neighbours: their clamped run carries weight 0)
            const bool below = grid && r < d.side - 1;
            const bool ldiag = grid && level_diag(T, td.level);
            // (a 'grid-diagonal' segment takes the run path only when it is a whole 8-node run: seg_wide.h row_sum3)
            const bool slow = !grid || sd.n_first + 8 > n_frame || (below && sd.n_first + d.side + 8 > n_frame) ||
                              (kids && (cb < 0 || cb + d.cside + 16 > n_frame)) || (ldiag && sd.cnt != 8);
            sd.mode = sd.cnt == 0 ? 0 : (d.kind == KIND_CONN ? 3 : (slow ? 2 : 1));
            sd.aux = (d.kind == KIND_AUX ? 1 : 0) | (ldiag ? 2 : 0) | (d.kind == KIND_AUX ? (hub_of_level(T, td.level) + 1) << 2 : 0);
            if (sd.mode == 1) {
                sd.up0 = clampi(sd.n_first - d.side, 0, hi8);
                sd.down0 = clampi(sd.n_first + d.side, 0, hi8);
                sd.par0 = clampi(d.pbase + (d.poff + (r >> 1)) * d.pside + d.poff + (c0 >> 1), 0, hi8);
                sd.left = clampi(sd.n_first - 1, 0, last);
                sd.right = clampi(sd.n_first + 8, 0, last);
                sd.c0 = clampi(cb, 0, hi8);
                sd.c1 = clampi(cb + 8, 0, hi8);
                sd.c2 = clampi(cb + d.cside, 0, hi8);
                sd.c3 = clampi(cb + d.cside + 8, 0, hi8);
                segment_pattern(T, dis, d, sd, r, c0, ldiag, w);
                auto it = pat_index.find(w);
                if (it == pat_index.end()) {
                    it = pat_index.emplace(w, (int)pat_index.size()).first;
                    pats.insert(pats.end(), w.begin(), w.begin() + 128);
                    pat_extra.insert(pat_extra.end(), w.begin() + 128, w.end());
                }
                sd.pat = it->second;
            }
            segs[t * 8 + tr] = sd;
        }
    }
    if (pats.empty()) { pats.assign(128, 0.0f); pat_extra.assign(5, 0.0f); }
}

// Pairs the patch rows (pad0, pad1 of every even row) and decides whether the handle gets a child-sum side buffer of
// `kid_rows` rows per frame (gcn_layer_ps.hip): anything irregular switches it off.  Returns the verdict.
static bool pair_segments(const Topo& T, const std::vector<TileDesc>& tiles, std::vector<SegDesc>& segs, int kid_rows) {
    bool kidsum_ok = kid_rows > 0;
    for (size_t t = 0; t < tiles.size(); ++t) {
        const TileDesc& td = tiles[t];
        const LevelDesc& d = T.desc[td.level];
        for (int tr = 0; tr < 8; tr += 2) {       // pad0 of an even patch row: it and the next row form a pair (seg_wide.h)
            SegDesc& sa = segs[t * 8 + tr];
            const SegDesc& sb = segs[t * 8 + tr + 1];
            sa.pad0 = sa.mode == 1 && sb.mode == 1 && sa.aux == sb.aux && sa.par0 == sb.par0 && sa.down0 == sb.n_first &&
                      sb.up0 == sa.n_first && sa.cnt == sb.cnt;
            if (sa.cnt <= 0 || !(d.kind == KIND_AUX || d.kind == KIND_MAIN)) continue;
            // pad1 = number of parents whose four children are exactly columns 2j, 2j+1 of this pair of rows
            const int idx = sa.n_first - d.base, r = idx / d.side, c0 = idx - r * d.side;
            int npar = 0;
            if (r < d.plim) {
                const int cend = c0 + sa.cnt < d.plim ? c0 + sa.cnt : d.plim;
                npar = cend > c0 ? (cend - c0) / 2 : 0;
                if (cend > c0 && ((cend - c0) & 1)) { kidsum_ok = false; topo_debug("kidsum off: odd t=%zu tr=%d\n", t, tr); }
            }
            const int par_raw = d.pbase + (d.poff + (r >> 1)) * d.pside + d.poff + (c0 >> 1);
            // ('grid-diagonal' levels of fewer than 8 columns run node by node -- rows pulled through the CSR, children
            //  included -- and never read the side buffer: child sums that nobody writes for THEIR rows are not missed)
            const bool parent_slow = td.level > 0 && level_diag(T, td.level - 1) && T.side[td.level - 1] < 8 && d.kind == KIND_AUX;
            if (npar > 0 && !parent_slow && (!sa.pad0 || par_raw != sa.par0 || par_raw + npar > kid_rows)) {
                kidsum_ok = false;
                topo_debug("kidsum off: parent t=%zu tr=%d level=%d pad0=%d par_raw=%d par0=%d npar=%d kid_rows=%d modes %d %d\n", t, tr, td.level,
                           sa.pad0, par_raw, sa.par0, npar, kid_rows, sa.mode, sb.mode);
            }
            // (par0 is set on the run path alone: a node-by-node segment -- a 'grid-diagonal' level of fewer than 8 columns -- names no
            //  parents.  With npar it stored sums of rows it never staged at rows par0 = 0 .. of the side buffer, the rows of other
            //  nodes; its parents run node by node as well and never read theirs, which keep what the caller put there)
            sa.pad1 = sa.mode == 1 ? npar : 0;
            const bool kids = d.kind == KIND_AUX && ((r >= d.clo && r < d.chi) || (r + 1 >= d.clo && r + 1 < d.chi)) && c0 < d.chi && c0 + 8 > d.clo;
            const bool self_slow = level_diag(T, td.level) && d.side < 8;
            // the pair path reads runs of 8 child-sum rows from each segment's first node: they must stay inside the
            // frame's slice of the side buffer (tiny pyramids only: a 2x2 or 4x4 level right at its end; an over-read
            // past the LAST frame's slice left the allocation and aborted a test run once)
            if (kids && !self_slow && (sa.n_first + 8 > kid_rows || sb.n_first + 8 > kid_rows)) { kidsum_ok = false; topo_debug("kidsum off: 8-row run past the side buffer t=%zu tr=%d\n", t, tr); }
            // a segment that would read the side buffer is not on the pair path
            if (kids && !sa.pad0 && !self_slow) { kidsum_ok = false; topo_debug("kidsum off: kids unpaired t=%zu tr=%d level=%d\n", t, tr, td.level); }
        }
    }
    return kidsum_ok;
}

// The same patterns in "quad" layout for the producer/consumer kernel, which keeps them in LDS: [pattern][row parity
// h][slot 0..7][k 0..3] = weight of (node 2k + h, slot); slot 6 = 1.0 when the node has children.  The outer
// neighbours of a segment's first and last node travel apart from the inner ones (seg_wide.h, segw_rows): node 0's
// left weight and node 7's right weight sit in slot 7 (k = 0 of h = 0, k = 3 of h = 1) and are zero in slots 3 / 4.
static void quad_layout(const std::vector<float>& pats, const std::vector<float>& pat_extra, int n_pats, std::vector<float>& patsq) {
    patsq.assign((size_t)n_pats * 64, 0.0f);
    for (int pi = 0; pi < n_pats; ++pi)
        for (int h = 0; h < 2; ++h)
            for (int sl = 0; sl < 7; ++sl)
                for (int k = 0; k < 4; ++k) {
                    const float w = pats[(size_t)pi * 128 + (2 * k + h) * 8 + sl];
                    const bool outer = (sl == 3 && h == 0 && k == 0) || (sl == 4 && h == 1 && k == 3);
                    patsq[(size_t)pi * 64 + h * 32 + sl * 4 + k] = outer ? 0.0f : (sl < 6 ? w : (w != 0.0f ? 1.0f : 0.0f));
                    if (outer) patsq[(size_t)pi * 64 + h * 32 + 7 * 4 + k] = w;
                }
    for (int pi = 0; pi < n_pats && !pat_extra.empty(); ++pi) {
        const float* ex = &pat_extra[(size_t)pi * 5];
        if (ex[0] == 0.0f) continue;
        // diagonal segment: slots 3 / 4 = edge nodes of the row above / below (seg_wide.h SLOT_EDGE_U / SLOT_EDGE_D), laid out like
        // slot 7: the left edge belongs to node 0 (k = 0 of h = 0), the right edge to node 7 (k = 3 of h = 1)
        for (int h = 0; h < 2; ++h)
            for (int k = 0; k < 4; ++k) { patsq[(size_t)pi * 64 + h * 32 + 3 * 4 + k] = 0.0f; patsq[(size_t)pi * 64 + h * 32 + 4 * 4 + k] = 0.0f; }
        patsq[(size_t)pi * 64 + 0 * 32 + 3 * 4 + 0] = ex[1]; patsq[(size_t)pi * 64 + 1 * 32 + 3 * 4 + 3] = ex[2];
        patsq[(size_t)pi * 64 + 0 * 32 + 4 * 4 + 0] = ex[3]; patsq[(size_t)pi * 64 + 1 * 32 + 4 * 4 + 3] = ex[4];
    }
}

// chunks of <= 256 rows over the levels that hang on a connection node (levels 0 .. naux - 2): the pre-pass (conn.hip) sums
// (deg + 1)^-1/2 x over a chunk per workgroup, then over a level's chunks in order
static void conn_chunk_table(const Topo& T, std::vector<int>& table) {
    for (int l = 0; l <= T.n_aux - 2; ++l)
        for (int r0 = T.base[l]; r0 < T.base[l + 1]; r0 += 256) {
            const int rows = T.base[l + 1] - r0 < 256 ? T.base[l + 1] - r0 : 256;
            table.insert(table.end(), {l, r0, rows, 0});
        }
}

int build_topo_tables(const Topo& T, TopoTables& out) {
    out = TopoTables{};
    out.hybrid = (T.diag_main || T.diag_aux || T.n_conn > 0) ? 1 : 0;      // (any topology whose stencil lives in the producer/consumer kernel only)
    build_degrees(T, out.hybrid != 0, out.dis, out.h_rowptr, out.h_colidx);
    build_patch_order(T, out.tiles);
    std::vector<float> pat_extra;
    build_segments(T, out.dis, out.tiles, out.segs, out.pats, pat_extra);
    const int kid_rows = (T.n_aux > 0 && T.n_levels > 1) ? T.base[T.n_levels - 1] : 0;
    const bool kidsum_ok = pair_segments(T, out.tiles, out.segs, kid_rows);
    out.n_pats = (int)(out.pats.size() / 128);
    topo_debug("topo: %zu tiles, %d patterns, kidsum %d\n", out.tiles.size(), out.n_pats, (int)kidsum_ok);
    quad_layout(out.pats, pat_extra, out.n_pats, out.patsq);
    // chained layers run the producer/consumer kernel, which keeps the pattern table in LDS beside its tile buffers
    const size_t ps_lds = (size_t)(4 * TILE * LDA + 16 + 64 + 2 * TILE + (out.pats.size() / 128) * 64 + 4 * C) * sizeof(float);   // incl. the fused-classifier tables
    out.kid_rows = (kidsum_ok && ps_lds <= 160 * 1024) ? kid_rows : 0;
    out.flat = (T.n_levels == 1 && T.n_desc == 1 && ps_lds <= 160 * 1024) ? 1 : 0;
    if (T.n_conn > 0) {
        conn_chunk_table(T, out.conn_table);
        out.conn_chunks = (int)(out.conn_table.size() / 4);
    }
    return EG_OK;
}

}  // namespace eg
