"""-m gpu: the plain eval layer of the producer / consumer kernel on its split route -- both operands of the matrix product cut
exactly into three bf16 pieces, six piece products per 16-k step on the bf16 matrix path (csrc/tile.h mfma_rowblock_bf16x6) --
against a float64 evaluation on the CPU that contains no HIP kernel (test 1; test 3 takes the product's operand from the fp32
route's W = I output, whose aggregation test 1 checks) and against the fp32 route (EG_LAYER_SPLIT=0, read when the
handle is created) on the same inputs: error against float64 within the bound of tests/test_gpu_jk.py and within twice the fp32
route's own, W = I bit for bit, |err| / sum |a||w| <= 1e-6 over six orders of magnitude (a route that left out any second-order
product sits at 1.8e-5), 200 identical launches at the full grid, and batch invariance."""
import contextlib
import functools
import itertools
import os

import numpy as np
import pytest
import torch

from gpu_util import DEV, rand_rows
from echoglad_amd import ops
from echoglad_amd.topology import HierTopology, TopologySpec

pytestmark = pytest.mark.gpu

# (frame, naux, main_only, coordinate nodes)
HANDLES = [(16, 3, False, False),          # levels smaller than a tile
           (17, 3, False, False),          # ragged patches: absent segments, short segments
           (30, 3, False, False),
           (16, 2, True, False),           # a single level: no child sums
           (20, 0, True, False),           # ... with ragged patches
           (16, 3, False, True)]           # the 4-row coordinate tile


@contextlib.contextmanager
def _env(value):
    old = os.environ.get("EG_LAYER_SPLIT")
    if value is None:
        os.environ.pop("EG_LAYER_SPLIT", None)
    else:
        os.environ["EG_LAYER_SPLIT"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("EG_LAYER_SPLIT", None)
        else:
            os.environ["EG_LAYER_SPLIT"] = old


def _graphs(*handle):
    """(handle on the default = split route, handle on the fp32 route): the variable is read when a handle is created."""
    with _env(None):
        g_split = ops.Graph.topo(*handle)
    with _env("0"):
        g_fp32 = ops.Graph.topo(*handle)
    return g_split, g_fp32


def _one_launch(g, fn):
    before = g.ps_launches
    got = fn()
    assert g.ps_launches == before + 1                      # the producer / consumer kernel, once
    return got


def _glorot(seed):
    rs = np.random.RandomState(seed)
    b = float(np.sqrt(6.0 / 256.0))
    return torch.from_numpy(rs.uniform(-b, b, (128, 128)).astype(np.float32)).to(DEV)


# ---- the float64 reference: CPU only, no kernel of the library in it -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edges(frame, naux, main_only, coord):
    topo = HierTopology(TopologySpec(frame, naux, main_only, coord))
    e = torch.from_numpy(np.ascontiguousarray(topo.edge_index())).long()
    n = topo.num_nodes
    deg = torch.ones(n, dtype=torch.float64)
    deg.index_add_(0, e[1], torch.ones(e.shape[1], dtype=torch.float64))
    dis = deg.pow(-0.5)
    return n, e[0], e[1], dis[e[0]] * dis[e[1]], dis * dis


def _ahat64(handle, x, B):
    n, src, dst, w_edge, w_self = _edges(*handle)
    xv = x.detach().cpu().double().view(B, n, 128)
    out = xv * w_self[None, :, None]
    out.index_add_(1, dst, xv[:, src, :] * w_edge[None, :, None])
    return out.reshape(B * n, 128)


def _kidsum64(handle, out64, B):
    """Child sums of finished rows, float64: row p of a frame's side buffer = sum over the children c of aux node p of
    (deg_c + 1)^-1/2 out[c].  The children of a node are its neighbours on the next level down (node ids grow with the level)."""
    topo = HierTopology(TopologySpec(*handle))
    n, src, dst, _, w_self = _edges(*handle)
    bases = torch.tensor([lv.base for lv in topo.aux_levels] + [topo.main.base, topo.coord_base], dtype=torch.long)
    level = lambda ids: torch.bucketize(ids, bases, right=True)
    down = (level(src) > level(dst)) & (src < topo.coord_base) & (dst < topo.main.base)
    rows = topo.main.base                                     # aux nodes per frame (no connection nodes in these handles)
    ov = out64.view(B, n, 128)
    kid = torch.zeros(B, rows, 128, dtype=torch.float64)
    kid.index_add_(1, dst[down], ov[:, src[down], :] * w_self[src[down]].sqrt()[None, :, None])
    return kid.reshape(B * rows, 128)


def _layer64(xw, x, sc, sh, residual, relu):
    h = xw
    if sc is not None:
        h = h * sc.cpu().double()
    if sh is not None:
        h = h + sh.cpu().double()
    if relu:
        h = torch.relu(h)
    if residual:
        h = h + x.cpu().double()
    return h


# ---- 1. against float64, beside the fp32 route ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("frame,naux,main_only,coord", HANDLES)
def test_split_route_vs_float64_and_the_fp32_route(frame, naux, main_only, coord, B):
    """Every ReLU / residual / scale-shift combination with the child sums pulled, handed in and handed out.  Bound: the one of
    tests/test_gpu_jk.py, 2e-5 max(1, max |want|).  The split route's worst error / bound may be at most twice the fp32 route's
    of the same run (the rounding patterns differ; a CPU simulation of both gives 0.85 - 1.0)."""
    handle = (frame, naux, main_only, coord)
    g_s, g_f = _graphs(*handle)
    n = g_s.num_nodes
    assert n == _edges(*handle)[0]
    w = rand_rows(128, seed=21).to(DEV) * 0.08
    sc = rand_rows(1, seed=30).to(DEV).reshape(128) * 0.1 + 1.0
    sh = rand_rows(1, seed=31).to(DEV).reshape(128) * 0.1
    forms = ("pulled", "handed in", "handed out", "handed in and out") if g_s.kidsum_rows > 0 else ("pulled",)
    worst_s, worst_f = 0.0, 0.0
    for form in forms:
        x, ka = rand_rows(B * n, seed=9).to(DEV), None
        if "in" in form.split():                            # the output of a layer together with the child sums it left behind
            ka = ops.new_kidsum(g_f, B)
            x = _one_launch(g_f, lambda: ops.gcn_layer_fwd(g_f, B, x, w, sc, sh, x, relu=True, kidsum_out=ka))
        x_keep = x.clone()
        xw = _ahat64(handle, x, B) @ w.cpu().double().T
        for relu, residual, affine in itertools.product((True, False), repeat=3):
            scale, shift = (sc, sh) if affine else (None, None)
            want = _layer64(xw, x, scale, shift, residual, relu)
            bound = 2e-5 * max(1.0, float(want.abs().max()))
            what = (form, relu, residual, affine)
            outs, kouts = [], []
            for g in (g_s, g_f):
                kb = ops.new_kidsum(g, B) if "out" in form.split() else None
                outs.append(_one_launch(g, lambda: ops.gcn_layer_fwd(g, B, x, w, scale, shift, x if residual else None, relu,
                                                                     kidsum_in=ka, kidsum_out=kb)))
                kouts.append(kb)
            err_s = float((outs[0].cpu().double() - want).abs().max())
            err_f = float((outs[1].cpu().double() - want).abs().max())
            worst_s, worst_f = max(worst_s, err_s / bound), max(worst_f, err_f / bound)
            assert err_s < bound and err_f < bound, (what, err_s, err_f, bound)
            assert torch.equal(x, x_keep), what
            if kouts[0] is not None:                        # the child sums of the output, from the same finished tile
                assert float((kouts[0] - kouts[1]).abs().max()) < bound, what
                kid64 = _kidsum64(handle, want, B)
                assert kouts[0].shape == kid64.shape, (kouts[0].shape, kid64.shape)
                err_k = [float((k.cpu().double() - kid64).abs().max()) for k in kouts]
                assert err_k[0] < bound and err_k[1] < bound, (what, err_k, bound)
    print(f"{frame}/{naux}{' main-only' if main_only else ''}{' coord' if coord else ''} B={B}: worst |err| / bound: "
          f"split {worst_s:.4f}, fp32 {worst_f:.4f}, ratio {worst_s / worst_f:.2f}")
    assert worst_s <= 2.0 * worst_f, (worst_s, worst_f)


# ---- 2. W = I ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame,naux,main_only,coord,B", [(17, 3, False, False, 3), (20, 0, True, False, 2), (64, 6, False, False, 4),
                                                          (224, 7, False, False, 8)])
def test_identity_weight_returns_the_fp32_routes_bits(frame, naux, main_only, coord, B):
    """With W = I and nothing else the output IS the aggregated row as the matrix unit saw it: hi + mid + lo on the split route,
    the row itself on the fp32 route.  A dropped, stale or misplaced piece is a mismatch.
    (224, 7), batch 8 -- every workgroup slot busy for many tiles, producers and consumers side by side on every SIMD -- is where
    packed fp32 instructions beside the bf16 MFMAs returned rows with zeroed channels in 56 of 60 launches (DESIGN_NOTES 9.8;
    smaller grids: 0 of 60): five launches of each form there."""
    g_s, g_f = _graphs(frame, naux, main_only, coord)
    eye = torch.eye(128, device=DEV)
    full = frame == 224
    gen = torch.Generator(device=DEV).manual_seed(5)
    for scale in (1.0,) if full else (1.0, 1e-3, 1e4):
        x = (torch.randn(B * g_s.num_nodes, 128, device=DEV, generator=gen) if full else rand_rows(B * g_s.num_nodes, seed=5).to(DEV)) * scale
        for chained in (False, True) if g_s.kidsum_rows > 0 else (False,):
            xin, ka = x, None
            if chained:                                     # a layer's output together with the child sums it left behind
                ka = ops.new_kidsum(g_f, B)
                xin = ops.gcn_layer_fwd(g_f, B, x, eye, None, None, x, kidsum_out=ka)
            want = _one_launch(g_f, lambda: ops.gcn_layer_fwd(g_f, B, xin, eye, kidsum_in=ka))
            for launch in range(5 if full else 1):
                got = _one_launch(g_s, lambda: ops.gcn_layer_fwd(g_s, B, xin, eye, kidsum_in=ka))
                assert torch.equal(got, want), (scale, chained, launch, float((got - want).abs().max()))


# ---- 3. magnitudes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame,naux,main_only", [(30, 3, False), (20, 0, True)])
def test_error_per_term_over_six_orders_of_magnitude(frame, naux, main_only):
    """|err| / sum_k |a_k||w_k| <= 1e-6 per output element, a = the aggregated row the product starts from (the fp32 route's
    W = I output: exact, test 2), the reference a W^T in float64.  fp32 and six piece products reach 2e-7, three reach 1.8e-5:
    a route that leaves out a second-order product fails.  Frames scaled 1e-3, 1, 30, 1e4 and one mixing them per element."""
    g_s, g_f = _graphs(frame, naux, main_only, False)
    n, B = g_s.num_nodes, 5
    x = rand_rows(B * n, seed=13).view(B, n, 128)
    mags = torch.tensor([1e-3, 1.0, 30.0, 1e4])
    for b in range(4):
        x[b] *= mags[b]
    x[4] *= mags[torch.from_numpy(np.random.RandomState(2).randint(0, 4, (n, 128)))]
    x = x.reshape(B * n, 128).contiguous().to(DEV)
    w = _glorot(7)
    a = ops.gcn_layer_fwd(g_f, B, x, torch.eye(128, device=DEV)).cpu().double()
    want = a @ w.cpu().double().T
    denom = a.abs() @ w.cpu().double().abs().T
    assert float(denom.min()) > 0.0
    worst = {}
    for name, g in (("split", g_s), ("fp32", g_f)):
        out = _one_launch(g, lambda: ops.gcn_layer_fwd(g, B, x, w))
        ratio = ((out.cpu().double() - want).abs() / denom).view(B, n, 128)
        worst[name] = [float(ratio[b].max()) for b in range(B)]
    print(f"{frame}/{naux}: worst |err| / sum|a||w| per frame (1e-3, 1, 30, 1e4, mixed): split {worst['split']}, fp32 {worst['fp32']}")
    assert max(worst["split"]) <= 1e-6 and max(worst["fp32"]) <= 1e-6, worst


# ---- 4. determinism and batch invariance -------------------------------------------------------------------------------------------
def test_two_hundred_launches_at_the_full_grid_are_bit_identical():
    """(224, 7), batch 8, chained form: every workgroup slot busy, producers stalled on memory -- the conditions under which a
    piece register rewritten while an MFMA still reads it shows (DESIGN_NOTES 5.14), as a launch that differs from the first."""
    g = ops.Graph.topo(224, 7)
    B = 8
    gen = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(B * g.num_nodes, 128, device=DEV, generator=gen)
    w = _glorot(11)
    sc, sh = torch.rand(128, device=DEV, generator=gen) + 0.5, torch.randn(128, device=DEV, generator=gen) * 0.1
    ka, kb, kc = ops.new_kidsum(g, B), ops.new_kidsum(g, B), ops.new_kidsum(g, B)
    h = ops.gcn_layer_fwd(g, B, x, w, sc, sh, x, relu=True, kidsum_out=ka)
    first = _one_launch(g, lambda: ops.gcn_layer_fwd(g, B, h, w, sc, sh, h, relu=True, kidsum_in=ka, kidsum_out=kb))
    out = torch.empty_like(first)
    same = torch.ones(2, dtype=torch.bool, device=DEV)
    for _ in range(200):
        ops.gcn_layer_fwd(g, B, h, w, sc, sh, h, relu=True, out=out, kidsum_in=ka, kidsum_out=kc)
        same[0] &= (out == first).all()
        same[1] &= (kc == kb).all()
    assert bool(torch.isfinite(first).all())
    assert same.tolist() == [True, True], f"(rows, child sums) identical over 200 launches: {same.tolist()}"


@pytest.mark.parametrize("frame,naux,main_only,coord", [(17, 3, False, False), (30, 3, False, False), (20, 0, True, False)])
def test_a_frame_does_not_depend_on_its_neighbours(frame, naux, main_only, coord):
    g = ops.Graph.topo(frame, naux, main_only, coord)
    n, B = g.num_nodes, 3
    x, w = rand_rows(B * n, seed=17).to(DEV), _glorot(3)
    for chained in (False, True) if g.kidsum_rows > 0 else (False,):
        xin, ka = x, None
        if chained:
            ka = ops.new_kidsum(g, B)
            xin = ops.gcn_layer_fwd(g, B, x, w, None, None, x, relu=True, kidsum_out=ka)
        f1 = lambda t: None if t is None else t.view(B, -1, 128)[1].contiguous()
        kb, kb1 = (ops.new_kidsum(g, B), ops.new_kidsum(g, 1)) if chained else (None, None)
        out = _one_launch(g, lambda: ops.gcn_layer_fwd(g, B, xin, w, None, None, xin, relu=True, kidsum_in=ka, kidsum_out=kb))
        alone = _one_launch(g, lambda: ops.gcn_layer_fwd(g, 1, f1(xin), w, None, None, f1(xin), relu=True, kidsum_in=f1(ka), kidsum_out=kb1))
        assert torch.equal(out.view(B, n, 128)[1], alone), chained
        if chained:
            assert torch.equal(kb.view(B, -1, 128)[1], kb1)


# ---- 5. the switch ----------------------------------------------------------------------------------------------------------------
def test_the_fp32_route_still_runs_and_differs_by_rounding_only():
    g_s, g_f = _graphs(64, 6, False, False)
    n, B = g_s.num_nodes, 2
    x, w = rand_rows(B * n, seed=23).to(DEV), _glorot(5)
    ka_s, ka_f = ops.new_kidsum(g_s, B), ops.new_kidsum(g_f, B)
    out_s = _one_launch(g_s, lambda: ops.gcn_layer_fwd(g_s, B, x, w, None, None, x, relu=True, kidsum_out=ka_s))
    out_f = _one_launch(g_f, lambda: ops.gcn_layer_fwd(g_f, B, x, w, None, None, x, relu=True, kidsum_out=ka_f))
    want = _layer64(_ahat64((64, 6, False, False), x, B) @ w.cpu().double().T, x, None, None, True, True)
    bound = 2e-5 * max(1.0, float(want.abs().max()))
    assert float((out_s.cpu().double() - want).abs().max()) < bound and float((out_f.cpu().double() - want).abs().max()) < bound
    diff = float((out_s - out_f).abs().max())
    assert 0.0 < diff < bound, diff                         # two routes (not one kernel twice), apart by rounding
    assert float((ka_s - ka_f).abs().max()) < bound
