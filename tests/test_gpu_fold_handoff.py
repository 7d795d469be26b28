"""-m gpu: the hand-off inside the bf16 body of the folded last layer + heads with the residual (k_gcn_layer_ps FSPLIT, FOLD = 1;
DESIGN 3.1c).  The producer waves compute c + h W1s^T for the first EG_FOLD_PROD_RB 16-row blocks of a tile and leave it in place
over those rows of the raw-row tile; the consumer waves start those accumulators from it and run the residual units of the other row
blocks themselves.  A partial that is lost, stale, read from the other buffer or put into another row block is an error of the size
of the term itself, far above the float64 rule (eval_reference.Report) every comparison here uses unless it says bit equality.

One matrix at a time separates the two paths; few tiles per workgroup reach the prologue-only and one-iteration paths of the
producers' meetings; the chained pair at four to five tiles per workgroup reuses both LDS buffers and the in-place region."""
import pytest
import torch

import eval_reference as E
import test_gpu_fold_split as S
from echoglad_amd import ops
from echoglad_amd.nn._heads import fold_last_into_heads

pytestmark = pytest.mark.gpu

DEV, C, F32, F64 = S.DEV, S.C, S.F32, S.F64


def _case(handle, B):
    """(topo, x, folded weights, packed heads on the device) of test_gpu_fold_split's input set with the residual."""
    topo, x, (w, sc, sh), packed, _, _, _ = S._reference(handle, B, 1.0, True)
    pg = {k: v.to(DEV) for k, v in packed.items()}
    fold = fold_last_into_heads(w.to(DEV), sc.to(DEV), sh.to(DEV), pg["w1"], pg["s1"], pg["t1"], True)
    return topo, x, fold, packed, pg


def _rule(name, gots, Eg, B, x, fold, packed):
    """Report's rule for several results of one formula: the float64 and float32 references are computed once."""
    (r64, s64), (r32, _) = (S._folded_eval(Eg, B, x, fold, packed, dt) for dt in (F64, F32))
    rep = E.Report()
    for how, got in gots:
        rep.check(f"{name} {how}", got, r64, r32, s64)
    print(rep.table(name))
    return rep


@pytest.mark.parametrize("which", ["m1 = 0", "w1s = 0"])
@pytest.mark.parametrize("handle,B", S.SHAPES, ids=str)
def test_one_matrix_at_a_time(handle, B, which):
    """m1 = 0, full W1s: the logits come from the producers' partial (row blocks they own) and from the consumers' residual units
    (the rest), and from nothing else.  w1s = 0, full M: the partial is c alone, and every aggregated unit adds to it."""
    g = S._graph(handle)
    topo, x, (m1, w1s, c1), packed, pg = _case(handle, B)
    zero = torch.zeros_like(m1)
    fold = (zero, w1s, c1) if which == "m1 = 0" else (m1, zero, c1)
    full = ops.gcn_layer_cls_fold_fwd(g, B, x.to(DEV), (m1, w1s, c1), True, pg)
    xg = x.to(DEV)
    kin = E.kidsum(topo, x, B)[0].to(F32).to(DEV) if g.kidsum_rows > 0 else None
    gots = [("pulled", S._one_launch(g, lambda: ops.gcn_layer_cls_fold_fwd(g, B, xg, fold, True, pg)))]
    if kin is not None:
        gots.append(("handed in", S._one_launch(g, lambda: ops.gcn_layer_cls_fold_fwd(g, B, xg, fold, True, pg, kidsum_in=kin))))
    assert float((gots[0][1] - full).abs().max()) > 1e-3               # the matrix left out carries weight
    rep = _rule(f"{which} {handle} B={B}", gots, E.topo_edges(*handle), B, x, fold, packed)
    assert not rep.failed(), rep.failed()


FEW = [((16, 3, False, False, False, False, False), 1), ((16, 3, False, False, False, False, False), 2),
       ((64, 6, False, False, False, False, False), 1), ((64, 6, False, False, False, True, True), 1)]


@pytest.mark.parametrize("handle,B", FEW, ids=str)
def test_few_tiles_per_workgroup(handle, B):
    """As many workgroups as tiles (or 256 of them): every workgroup gets 0, 1 or 2 tiles, so the meetings run in the prologue
    alone, or once more.  The float64 rule; a second launch gives the same bits; each frame of a batch equals that frame alone."""
    g = S._graph(handle)
    Bx = max(B, 2)
    topo, x, fold, packed, pg = _case(handle, Bx)
    n = topo.num_nodes
    xg = x.to(DEV)[:B * n].contiguous()
    got = S._one_launch(g, lambda: ops.gcn_layer_cls_fold_fwd(g, B, xg, fold, True, pg))
    assert torch.equal(ops.gcn_layer_cls_fold_fwd(g, B, xg, fold, True, pg), got)
    rep = _rule(f"few tiles {handle} B={B}", [("pulled", got)], E.topo_edges(*handle), B, x[:B * n], fold, packed)
    assert not rep.failed(), rep.failed()
    rows = got.shape[0] // B
    for f in range(B):
        alone = ops.gcn_layer_cls_fold_fwd(g, 1, xg[f * n:(f + 1) * n].contiguous(), fold, True, pg)
        assert torch.equal(got[f * rows:(f + 1) * rows], alone), f
    if B == 1:                                                          # ... and as the second frame of a batch of two
        x2 = torch.cat([x.to(DEV)[n:2 * n], xg]).contiguous()
        both = ops.gcn_layer_cls_fold_fwd(g, 2, x2, fold, True, pg)
        assert torch.equal(both[rows:], got)


def test_chained_pair_in_steady_state_eager_and_captured():
    """(64, 6), B = 8: about 1 200 tiles, four to five per workgroup.  The plain split layer with kidsum_out, then the folded launch
    with kidsum_in, 100 times: no element differs from the first pair (counted on the device); the same pair captured in a graph
    and replayed three times gives the eager bits."""
    handle, B = S.SHAPES[2]
    g = S._graph(handle)
    n = g.num_nodes
    x = torch.randn(B * n, C, device=DEV, generator=torch.Generator(DEV).manual_seed(6))
    w, sc, sh = (t.to(DEV) for t in E.layer_params(51))
    pg = {k: v.to(DEV) for k, v in E.uniform_heads(7).items()}
    fold = fold_last_into_heads(w, sc, sh, pg["w1"], pg["s1"], pg["t1"], True)
    fold = fold + (ops.fold_lo_table(fold[0], fold[1]),)
    ka = ops.new_kidsum(g, B)
    h = torch.empty_like(x)

    def pair():
        ops.gcn_layer_fwd(g, B, x, w, sc, sh, x, relu=True, out=h, kidsum_out=ka)
        return ops.gcn_layer_cls_fold_fwd(g, B, h, fold, True, pg, kidsum_in=ka)

    first = pair().clone()
    differ = torch.zeros((), dtype=torch.int64, device=DEV)
    for _ in range(99):
        differ += (pair() != first).sum()
    assert int(differ) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pair()                                                           # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pair()
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, first)


def test_both_bodies_inside_the_rule_one_launch_each():
    handle, B = S.SHAPES[3]
    g, g_fp32 = S._graph(handle), S._graph(handle, "0")
    topo, x, fold, packed, pg = _case(handle, B)
    xg = x.to(DEV)
    gots = [(body, S._one_launch(gg, lambda: ops.gcn_layer_cls_fold_fwd(gg, B, xg, fold, True, pg))) for body, gg in (("split", g), ("fp32", g_fp32))]
    assert not torch.equal(gots[0][1], gots[1][1])                      # (two bodies: another summation order)
    rep = _rule(f"both bodies {handle} B={B}", gots, E.topo_edges(*handle), B, x, fold, packed)
    assert not rep.failed(), rep.failed()
