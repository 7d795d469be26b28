// Every combination of the inputs of ps_choose_form (csrc/ps_form.h), one line per combination, in the order of the header line's
// fields (the last one runs fastest).  Ten million lines: a line is the two-digit number of a result, and the distinct results
// follow at the end as "result <number> <text>":
//   F <cls> <jk> <mode> <diag> <fold> <split> <lds bytes>    the form launched
//   OK                                                         nothing to launch (no tiles)
//   U                                                          EG_ERR_UNSUPPORTED: the caller's other kernel
//   A <message>                                                EG_ERR_ARG
// Exit code 1 if a form is returned that PS_FORMS does not list, or one of PS_FORMS is never returned.
// Host only; built with -fsanitize=address,undefined by tests/test_ps_form.py.
#include <stdio.h>

#include <vector>

#include "../../echoglad_amd/csrc/ps_form.h"

using namespace eg;

// floats in front of s_bn: everything fits / the folded heads' one vector still does / no heads do / not even the plain layer does
static const int LDS_TABLES[] = {20000, 160 * 256 - 4 * EG_CHANNELS + 1, 160 * 256 - EG_CHANNELS + 1, 160 * 256 + 1};

int main() {
    printf("fields topo:2 residual:3 lower:3 stats_partial:2 agg_out:2 kin:2 kout:2 heads:3 jk_in:2 jk_out:2 kids:2 flat:2 hybrid:2 "
           "layer_impl:3 no_tiles:2 relu:2 scale:2 shift:2 lds_tables:4 layer_split:2\n");
    constexpr size_t N_FORMS = sizeof(PS_FORMS) / sizeof(PS_FORMS[0]);
    int reached[N_FORMS] = {};
    long long unlisted = 0, lines = 0;
    std::vector<PsChoice> results;                          // the distinct ones, in the order of their first appearance
    std::vector<char> out;
    PsCallFacts c{};
    PsHandleFacts h{};
    for (int topo = 0; topo < 2; ++topo)
    for (c.residual = 0; c.residual < 3; ++c.residual)
    for (int lower = 0; lower < 3; ++lower)                 // none / incomplete / complete
    for (int stats = 0; stats < 2; ++stats)
    for (int agg_out = 0; agg_out < 2; ++agg_out)
    for (int kin = 0; kin < 2; ++kin)
    for (int kout = 0; kout < 2; ++kout)
    for (int heads = 0; heads < 3; ++heads)                 // none / given / given with the last layer folded in
    for (int jk_in = 0; jk_in < 2; ++jk_in)
    for (int jk_out = 0; jk_out < 2; ++jk_out)
    for (int kids = 0; kids < 2; ++kids)
    for (int flat = 0; flat < 2; ++flat)
    for (int hybrid = 0; hybrid < 2; ++hybrid)
    for (h.layer_impl = -1; h.layer_impl < 2; ++h.layer_impl)
    for (int no_tiles = 0; no_tiles < 2; ++no_tiles)
    for (int relu = 0; relu < 2; ++relu)
    for (int scale = 0; scale < 2; ++scale)
    for (int shift = 0; shift < 2; ++shift)
    for (int tables : LDS_TABLES)
    for (h.layer_split = 0; h.layer_split < 2; ++h.layer_split) {
        c.relu = relu; c.scale = scale; c.shift = shift; c.kin = kin; c.kout = kout;
        c.cls = heads > 0; c.fold = heads == 2;
        c.jk_in = jk_in; c.jk_out = jk_out; c.agg_out = agg_out; c.stats_partial = stats;
        c.lower = lower > 0; c.lower_complete = lower == 2;
        c.no_tiles = no_tiles;
        h.topo = topo; h.hybrid = hybrid; h.flat = flat; h.kids = kids; h.lds_tables = tables;
        const PsChoice r = ps_choose_form(c, h);
        ++lines;
        if (r.rc == EG_OK && r.launch) {
            bool listed = false;
            for (size_t i = 0; i < N_FORMS; ++i)
                if (PS_FORMS[i] == r.form) { ++reached[i]; listed = true; }
            if (!listed) ++unlisted;
        }
        size_t k = 0;                                       // (a message is one string literal: the pointer tells them apart)
        while (k < results.size() && !(results[k].rc == r.rc && results[k].msg == r.msg && results[k].launch == r.launch &&
                                       results[k].form == r.form && results[k].lds == r.lds)) ++k;
        if (k == results.size()) results.push_back(r);
        if (k > 99) { printf("more than 100 distinct results\n"); return 2; }
        out.push_back((char)('0' + k / 10)); out.push_back((char)('0' + k % 10)); out.push_back('\n');
    }
    fwrite(out.data(), 1, out.size(), stdout);
    for (size_t k = 0; k < results.size(); ++k) {
        const PsChoice& r = results[k];
        const PsForm& f = r.form;
        printf("result %02zu ", k);
        if (r.rc == EG_ERR_UNSUPPORTED) printf("U\n");
        else if (r.rc == EG_ERR_ARG) printf("A %s\n", r.msg);
        else if (!r.launch) printf("OK\n");
        else printf("F %d %d %d %d %d %d %zu\n", f.cls, f.jk, f.mode, f.diag, f.fold, f.split, r.lds);
    }
    int never = 0;
    for (int n : reached) never += n == 0;
    printf("ps_form_check: %lld combinations, %lld with a form PS_FORMS does not list, %d of %zu forms never chosen\n", lines, unlisted, never,
           N_FORMS);
    return unlisted || never ? 1 : 0;
}
