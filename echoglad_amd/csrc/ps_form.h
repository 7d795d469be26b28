// Which instantiation of the producer/consumer layer kernel (gcn_layer_ps.hip: k_gcn_layer_ps) a call gets, or why it gets none.
// Host only, no HIP: tests/native/ps_form_check.cpp walks every combination of the inputs.
#pragma once
#include <stddef.h>

#include "../../include/echoglad_hip.h"

namespace eg {

// The template arguments of k_gcn_layer_ps, in the template's order.
struct PsForm {
    bool cls, jk;
    int mode;
    bool diag;
    int fold;
    bool split;
};
inline bool operator==(const PsForm& a, const PsForm& b) {
    return a.cls == b.cls && a.jk == b.jk && a.mode == b.mode && a.diag == b.diag && a.fold == b.fold && a.split == b.split;
}

// The forms.  Each has one instantiation, except the four folded ones, which have a second body behind the same form (FSPLIT:
// the products on the bf16 matrix path, gcn_layer_ps_fold_split.hip; eg_launch_layer_ps picks it from the handle's layer_split
// knob when the call brings the pre-split lo planes).  eg_launch_layer_ps grants every body the large dynamic LDS block and
// launches nothing else.
constexpr PsForm PS_FORMS[] = {
    {false, false, 0, false, 0, false}, {false, false, 0, true, 0, false},     // plain eval layer, fp32 chain
    {false, false, 0, false, 0, true},  {false, false, 0, true, 0, true},      // ... split product (gcn_layer_ps_split.hip)
    {false, true, 0, false, 0, false},                                         // ... with the running maximum
    {false, false, 1, false, 0, false}, {false, false, 1, true, 0, false},     // train forward
    {false, false, 2, false, 0, false}, {false, false, 2, true, 0, false},     // dX: the residual a tensor of its own
    {false, false, 3, false, 0, false}, {false, false, 3, true, 0, false},     // ... with the lower layer's sums
    {true, false, 0, false, 0, false},  {true, false, 0, true, 0, false},      // last layer + heads
    {true, true, 0, false, 0, false},                                          // ... on the running maximum
    {true, false, 0, false, 1, false},  {true, false, 0, true, 1, false},      // last layer folded into the heads, with the residual
    {true, false, 0, false, 2, false},  {true, false, 0, true, 2, false},      // ... without
};
inline bool ps_form_listed(const PsForm& f) {
    for (const PsForm& l : PS_FORMS)
        if (l == f) return true;
    return false;
}

// What eg_launch_layer_ps is asked for ...
struct PsCallFacts {
    int residual;                // 0 none, 1 x itself, 2 a tensor of its own
    bool relu, scale, shift;     // (scale / shift: given)
    bool kin, kout;
    bool cls, fold;              // fused heads given; ... with the last layer folded into them (ClsArgs::fold)
    bool jk_in, jk_out;
    bool agg_out, stats_partial;
    bool lower, lower_complete;  // LowerSums given; ... with every pointer set and row_hi >= 1
    bool no_tiles;               // tiles per frame * batch <= 0
};
// ... and on which handle.
struct PsHandleFacts {
    bool topo;                   // a handle, and of kind GRAPH_TOPO
    bool hybrid, flat, kids;     // (kids: kid_rows > 0)
    int layer_impl, layer_split; // the handle's knobs
    int lds_tables;              // floats of the dynamic LDS block in front of s_bn: tile buffers, rings, weight patterns
};

struct PsChoice {
    int rc;                      // EG_OK, EG_ERR_UNSUPPORTED ("use the other kernel") or EG_ERR_ARG (msg set)
    const char* msg;
    bool launch;                 // false with EG_OK: no tiles, nothing to do
    PsForm form;
    size_t lds;                  // bytes of dynamic LDS
};

inline PsChoice ps_choose_form(const PsCallFacts& c, const PsHandleFacts& h) {
    const auto no_launch = [](int rc, const char* msg = nullptr) { return PsChoice{rc, msg, false, PsForm{}, 0}; };
    if (!h.topo) return no_launch(EG_ERR_UNSUPPORTED);
    const bool rsep = c.residual == 2;                            // a residual tensor of its own: MODE 2, plain calls only
    if (c.lower && !rsep) return no_launch(EG_ERR_ARG, "the lower layer's sums go with the dX launch (a residual tensor of its own)");
    if (c.lower && !c.lower_complete) return no_launch(EG_ERR_ARG, "incomplete LowerSums");
    const bool train = c.stats_partial;
    if (rsep && (train || c.kin || c.kout || c.cls || c.jk_in || c.jk_out)) return no_launch(EG_ERR_UNSUPPORTED);
    if (c.agg_out && !train) return no_launch(EG_ERR_ARG, "agg_out goes with stats_partial (train forward)");
    if (train && (c.kout || c.cls || c.jk_in || c.jk_out))
        return no_launch(EG_ERR_ARG, "the train forward writes no child sums (its activation pass does) and takes no heads or running maximum");
    const bool jk = c.jk_in;
    if (c.jk_out != (jk && !c.cls)) return no_launch(EG_ERR_ARG, "jk_out goes with jk_in on a plain layer, the fused heads take jk_in alone");
    const bool chained = c.kin || c.kout || jk;
    if ((c.kin || c.kout) && !h.kids) return no_launch(EG_ERR_UNSUPPORTED);
    if (jk && !h.kids && !h.flat) return no_launch(EG_ERR_UNSUPPORTED);
    if (c.cls && !h.kids && !h.flat) return no_launch(EG_ERR_UNSUPPORTED);
    // plain calls: this kernel by default wherever its fast paths cover the topology -- single-level grids and regular pyramids
    // (child sums available); since the producers were rebuilt (round 3) its unchained form, which pulls the four child rows of
    // an aux node, is faster than the symmetric kernel as well (0.280 vs 0.309 ms per launch at configs[1], round 5) -- and the
    // symmetric kernel on irregular frames; EG_LAYER_IMPL = 0 / 1 forces one of them
    const bool diag = h.hybrid;                                   // 'grid-diagonal' levels: this kernel is the stencil path of such handles
    if (diag && jk) return no_launch(EG_ERR_UNSUPPORTED);            // (the running maximum has no diagonal instantiation: the caller takes it outside)
    if (!chained && !c.cls && !train && !rsep && !diag &&
        (h.layer_impl < 0 ? (h.flat || h.kids) : h.layer_impl != 0) == false) return no_launch(EG_ERR_UNSUPPORTED);
    if (c.no_tiles) return no_launch(EG_OK);
    const bool fold = c.cls && c.fold;                            // (gcn_layer.hip eg_gcn_layer_cls_fold_fwd: no running maximum, no ReLU)
    if (fold && (jk || c.relu || c.scale || c.shift)) return no_launch(EG_ERR_ARG, "the folded heads take no running maximum, ReLU, scale or shift");
    // (the folded form keeps one vector in s_bn; topo_tables.hip checks the larger sum)
    const size_t lds = (size_t)(h.lds_tables + (fold ? EG_CHANNELS : c.cls ? 4 * EG_CHANNELS : 0)) * sizeof(float);
    if (lds > 160 * 1024) return no_launch(EG_ERR_UNSUPPORTED);     // more weight patterns than fit beside the tile buffers
    // the plain eval layer takes the split product (exact 3-piece bf16 split, six piece products) unless EG_LAYER_SPLIT=0 asked
    // for the fp32 chain when the handle was created
    const bool split = h.layer_split != 0;
    PsForm f{};
    f.diag = diag;
    if (train) f.mode = 1;
    else if (rsep && c.lower) f.mode = 3;
    else if (rsep) f.mode = 2;
    else if (fold) { f.cls = true; f.fold = c.residual ? 1 : 2; }
    else if (c.cls) { f.cls = true; f.jk = jk; }
    else if (jk) f.jk = true;
    else f.split = split;
    return PsChoice{EG_OK, nullptr, true, f, lds};
}

}  // namespace eg
