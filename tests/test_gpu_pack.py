"""-m gpu: node-feature packing (csrc/pack.hip) against the reference's op sequence."""
import numpy as np
import pytest
import torch

import pool_reference as R
from coord_reference import FACTOR, ULP, Report
from gpu_util import DEV, model_pair
from fixtures_util import initial_coords, synthetic_frames
from pool_reference import pack_rows as _reference_pack
from echoglad_amd import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sides,batch,extra_front,extra_back", [
    ([2, 4, 8, 16], 3, 0, 0), ([2, 4, 30], 2, 4, 4), ([17], 2, 0, 0), ([2, 4, 8, 16, 32, 64, 128, 224], 2, 0, 0), ([1, 3, 65], 1, 2, 0)])
def test_pack_levels_is_the_reference_permute_cat(sides, batch, extra_front, extra_back):
    rs = np.random.RandomState(sum(sides))
    maps = [torch.from_numpy(rs.standard_normal((batch, 128, s, s)).astype(np.float32)).to(DEV).requires_grad_(True) for s in sides]
    n_rows = extra_front + sum(s * s for s in sides) + extra_back
    got = ops.pack_levels(maps, batch, n_rows, extra_front)
    want = _reference_pack(maps, batch, n_rows, extra_front)
    assert torch.equal(got, want)                                   # a copy: bit-exact
    g = torch.from_numpy(rs.standard_normal(tuple(got.shape)).astype(np.float32)).to(DEV)
    got_g = torch.autograd.grad(got, maps, g)
    want_g = torch.autograd.grad(want, maps, g)
    for a, b in zip(got_g, want_g):
        assert torch.equal(a, b)


def test_pack_rejects_bad_maps():
    with pytest.raises(RuntimeError):
        ops.pack_levels([torch.zeros(1, 128, 4, 4)], 1, 16)                       # CPU tensor
    with pytest.raises(RuntimeError):
        ops.pack_levels([torch.zeros(1, 64, 4, 4, device=DEV)], 1, 16)            # wrong channel count
    with pytest.raises(RuntimeError):
        ops.pack_levels([torch.zeros(1, 128, 8, 8, device=DEV)], 1, 16)           # does not fit the frame's rows


@pytest.mark.parametrize("frame,naux,coord,main_only", [(16, 3, False, False), (32, 4, True, False), (16, 2, False, True),
                                                        (64, 2, False, False), (224, 7, False, False)])
def test_create_node_pixels_matches_oracle(frame, naux, coord, main_only):
    hip, ref = model_pair(frame, naux, 1, coord=coord, main_only=main_only)
    B = 2
    frames = synthetic_frames(B, 128, frame, seed=3)
    coords = initial_coords(B, frame) if coord else None
    with torch.no_grad():
        want = ref.create_node_pixels(frames, B, None if coords is None else coords.view(B, 4, 2))
        got = hip.create_node_pixels(frames.to(DEV), B, None if coords is None else coords.to(DEV)).cpu()
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 2e-6 * max(1.0, float(want.abs().max()))


# the small cases whose seed meets the ReLU condition of test_gpu_pool_pack_fp64.py (float32 mask == float64 mask on the references,
# min|s64| >= 64 max|s32 - s64|): their gradients fall under the float64 rule too.  With 10^5 .. 10^7 pre-activations no seed does
# (none of 400 tried on the CPU for the other two): some |s| is always within rounding of the kink, so there the gradients keep the
# bound they had against torch's float32, next to the rule on the values.
CONV_RULE_SEED = {((17,), (1,), 2, 0, 0): 2}


def _decoder_shape_on_the_device(sides, chans, batch, n_rows, front, capsys):
    """The UNet variant's decoder (17 M node features): the float64 rule evaluated with torch float64 on the device."""
    gen = torch.Generator(device=DEV).manual_seed(sum(sides) + sum(chans))
    mk = lambda *shape, s=1.0: (torch.randn(*shape, device=DEV, generator=gen) * s).requires_grad_(True)
    feats = [mk(batch, c, sd, sd) for sd, c in zip(sides, chans)]
    ws = [mk(128, c, s=c ** -0.5) for c in chans]
    bs = [mk(128, s=0.5) for _ in chans]
    got = ops.conv1x1_relu_pack_levels(feats, ws, bs, batch, n_rows, front)
    conv = lambda f, w, b, dt: torch.einsum("oc,bcij->boij", w.detach().to(dt), f.detach().to(dt)) + b.detach().to(dt).view(1, 128, 1, 1)
    with torch.no_grad():
        ref64 = _reference_pack([torch.relu(conv(f, w, b, torch.float64)) for f, w, b in zip(feats, ws, bs)], batch, n_rows, front)
        scale = _reference_pack([conv(f.abs(), w.abs(), b.abs(), torch.float64) for f, w, b in zip(feats, ws, bs)], batch, n_rows, front)
    maps = [torch.relu(torch.nn.functional.conv2d(f, w.view(128, -1, 1, 1), b)) for f, w, b in zip(feats, ws, bs)]
    want = _reference_pack(maps, batch, n_rows, front)
    ref_err = float((want.detach().double() - ref64).abs().max())
    err = (got.detach().double() - ref64).abs()
    tol = FACTOR * ref_err + 8 * ULP * scale
    old = 1e-5 * max(1.0, float(want.detach().abs().max()))
    with capsys.disabled():
        print(f"\n  conv-pack decoder shape: max|kernel - fp64| {float(err.max()):.3e}, max|torch32 - fp64| {ref_err:.3e}, worst err / tol "
              f"{float((err / tol).max()):.3f}; largest tolerance of the rule {float(tol.max()):.3e}, the bound it replaces {old:.3e}")
    assert bool((err <= tol).all())
    return feats, ws, bs, got, maps, want


@pytest.mark.parametrize("sides,chans,batch,extra_front,extra_back", [
    ([2, 4, 8, 16, 32, 64, 128, 224], [512, 256, 128, 64, 32, 16, 8, 4], 2, 0, 0),      # the UNet variant's decoder (models.py:678-683)
    ([2, 4, 30], [40, 7, 3], 2, 4, 4), ([17], [1], 2, 0, 0), ([1, 3, 65], [33, 64, 5], 1, 2, 0)])
def test_conv1x1_relu_fused_into_the_packing(sides, chans, batch, extra_front, extra_back, capsys):
    """eg_conv1x1_relu_pack_levels == F.relu(Conv2d(C_l, 128, 1)(features[l])) + the reference's permute / cat
    (models.py:707-710, :726-756).  Values: every element against float64 under the rule of coord_reference.Report.check with
    scale = |W||x| + |b| (ReLU is 1-Lipschitz: no margin, no element left out, a differing zero pattern is an error like any other).
    Gradients (features, weights, biases): under the same rule where the case's seed keeps every pre-activation away from the
    kink (CONV_RULE_SEED), and within 2e-4 of torch's float32 everywhere."""
    n_rows = extra_front + sum(s * s for s in sides) + extra_back
    case = (tuple(sides), tuple(chans), batch, extra_front, extra_back)
    if sides[-1] == 224:
        feats, ws, bs, got, maps, want = _decoder_shape_on_the_device(sides, chans, batch, n_rows, extra_front, capsys)
        g = torch.randn(tuple(got.shape), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        params = feats + ws + bs
        for a, b in zip(torch.autograd.grad(got, params, g), torch.autograd.grad(want, params, g)):
            assert float((a - b).abs().max()) <= 2e-4 * max(1.0, float(b.abs().max()))
        # the model-level tail: the same through HierarchicalPatchModel.pack_node_features_linear on the default shape
        convs = [torch.nn.Conv2d(c, 128, kernel_size=1).to(DEV) for c in chans]
        with torch.no_grad():
            for m, w, b in zip(convs, ws, bs):
                m.weight.copy_(w.view_as(m.weight))
                m.bias.copy_(b)
        hip, _ = model_pair(224, 7, 1)
        with torch.no_grad():
            a = hip.pack_node_features_linear([f.detach() for f in feats], convs, batch)
            b = hip.pack_node_features([m.detach() for m in maps], batch)
        assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max()))
        return
    fx = R.conv_fixture(*case, "all", CONV_RULE_SEED.get(case, sum(sides) + sum(chans)))
    r64 = R.conv_pack64(fx["feats"], fx["weights"], fx["biases"], batch, n_rows, extra_front, dnodes=fx["dnodes"])
    r32 = R.conv_torch32(fx)
    same, ratio = R.relu_margin(r64["s"], r32["s"])
    if case in CONV_RULE_SEED:
        assert same and ratio >= R.MARGIN, (same, ratio)              # on the references alone, before the kernel runs
    dev = lambda t: t.to(DEV).requires_grad_(True)
    feats, ws, bs = [dev(t) for t in fx["feats"]], [dev(t) for t in fx["weights"]], [dev(t) for t in fx["biases"]]
    got = ops.conv1x1_relu_pack_levels(feats, ws, bs, batch, n_rows, extra_front)
    got_g = torch.autograd.grad(got, feats + ws + bs, fx["dnodes"].to(DEV))
    rep = Report()
    rep.check("node rows", got, r64["out"], r32["out"], r64["scale"])
    n = len(sides)
    want_g = r32["dfeat"] + r32["dw"] + r32["db"]
    for a, b in zip(got_g, want_g):
        assert float((a.cpu() - b).abs().max()) <= 2e-4 * max(1.0, float(b.abs().max()))
    if case in CONV_RULE_SEED:
        for key, lo in (("dfeat", 0), ("dw", n), ("db", 2 * n)):
            for l in range(n):
                rep.check(key, got_g[lo + l], r64[key][l], r32[key][l], r64[key + "_scale"][l])
    tol = FACTOR * rep.rows["node rows"][2] + 8 * ULP * float(r64["scale"].max())
    with capsys.disabled():
        print(rep.table(f"conv-pack {case} (min|s64| / max|s32 - s64| = {ratio:.1f}, masks equal: {same})"))
        print(f"    largest tolerance of the rule on the values {tol:.3e}, the bound it replaces {1e-5 * max(1.0, float(r32['out'].abs().max())):.3e}")
    assert not rep.failed(), rep.failed()


def test_conv_pack_rejects_bad_arguments():
    f = torch.zeros(1, 8, 4, 4, device=DEV)
    w = torch.zeros(128, 8, device=DEV)
    with pytest.raises(RuntimeError):
        ops.conv1x1_relu_pack_levels([f.cpu()], [w], [None], 1, 16)                 # CPU features
    with pytest.raises(RuntimeError):
        ops.conv1x1_relu_pack_levels([f], [torch.zeros(64, 8, device=DEV)], [None], 1, 16)     # not 128 output channels
    with pytest.raises(RuntimeError):
        ops.conv1x1_relu_pack_levels([torch.zeros(1, 8, 8, 8, device=DEV)], [w], [None], 1, 16)     # does not fit the frame's rows


@pytest.mark.parametrize("frame,naux,coord", [(32, 4, False), (64, 5, True), (224, 7, True)])
def test_unet_variant_example_end_to_end(frame, naux, coord):
    """INTEGRATION.md route A for the reference's UNet variant (echoglad_amd/examples.py): the subclass's create_node_pixels
    (stock torch front-end + ONE fused launch for the 1x1 convolutions, ReLU and the node-major packing) gives the reference
    tail's node features, and forward() runs frame -> logits on the HIP path (eval and one train step)."""
    from echoglad_amd.examples import UNetNodeFeatureModel, reference_tail
    from echoglad_amd.topology import HierTopology, TopologySpec
    from fixtures_util import initial_coords
    B = 2
    widths = [2 ** g for g in range(naux, 0, -1)]
    dims = [8 * 2 ** i for i in range(naux)]
    torch.manual_seed(3)
    model = UNetNodeFeatureModel(encoder_embedding_widths=widths, encoder_embedding_dims=dims, frame_size=frame, num_aux_graphs=naux,
                                 node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32, num_gnn_layers=3,
                                 output_activation="logit", use_coordinate_graph=coord, gnn_dropout_p=0.0,
                                 classifier_dropout_p=0.0).to(DEV).eval()
    topo = HierTopology(TopologySpec(frame, naux, False, coord))
    ei = torch.from_numpy(topo.batched_edge_index(B)).to(DEV)
    frames = torch.randn(B, dims[0] // 2, frame, frame, device=DEV)
    c0 = initial_coords(B, frame).to(DEV) if coord else None
    with torch.no_grad():
        maps = model.decoder_maps(frames)
        got = model.create_node_pixels(frames, B, None if c0 is None else c0.view(B, 4, 2))
        want = reference_tail(model, maps, B).view(B, -1, 128)
        n_grid = want.shape[1]
        assert float((got.view(B, topo.num_nodes, 128)[:, :n_grid] - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))
        logits, coords = model(x=frames, node_coords=c0, edge_index=ei, node_type=None, batch_idx=None)
        again, _ = model.forward_nodes(got, ei, B, None if c0 is None else c0.clone())
    assert logits.shape == (B * topo.num_valid_nodes, 4) and torch.isfinite(logits).all()
    # (not bit-equal: the second forward re-runs the torch front-end, and MIOpen may pick another convolution algorithm on a later call)
    assert float((logits - again).abs().max()) < 1e-4 * max(1.0, float(again.abs().max()))
    if frame > 64:
        return
    model.train()
    logits, coords = model(x=frames, node_coords=None if c0 is None else c0.clone(), edge_index=ei, node_type=None, batch_idx=None)
    ((logits ** 2).mean() + (0 if coords is None else (coords ** 2).mean() * 1e-3)).backward()
    missing = [k for k, p in model.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not missing, missing
    assert float(model.linears[0].weight.grad.abs().max()) > 0 and float(model.down_convs[0].conv1.weight.grad.abs().max()) > 0


@pytest.mark.parametrize("frame,sides,batch,chans", [(224, [2, 4, 8, 16, 32, 64, 128], 2, 128), (64, [2, 4, 8, 16, 32, 64], 2, 128),
                                                      (30, [2, 4, 8], 3, 128), (31, [2, 4, 8, 16], 2, 8), (448, [2, 4, 8, 16, 32, 64, 128, 256], 1, 4),
                                                      (16, [3, 5, 16], 2, 16), (256, [2, 4, 8, 16, 32, 64, 128], 1, 16), (8, [2], 1, 128)])
def test_avg_pool_pyramid_is_adaptive_avg_pool2d_for_every_level(frame, sides, batch, chans, capsys):
    """models.py:511-521: F.adaptive_avg_pool2d(frame, (2^g, 2^g)) for every aux level -- all levels in one launch
    (eg_avg_pool_pyramid_fwd: exact block means of a coarser level taken as the mean of 2 x 2 finer ones, everything else summed
    window by window) against torch's own op on the CPU in float64, and the gradient (a gather, no atomics) against torch's
    autograd; odd frames, sides that do not divide the frame, a side equal to the frame."""
    rs = np.random.RandomState(frame + len(sides))
    x_cpu = torch.from_numpy(rs.standard_normal((batch, chans, frame, frame))).requires_grad_(True)          # float64
    want = [torch.nn.functional.adaptive_avg_pool2d(x_cpu, (p, p)) for p in sides]
    x = x_cpu.detach().float().to(DEV).requires_grad_(True)
    got = ops.avg_pool_pyramid(x, sides)
    # ... and under the float64 rule of coord_reference.Report.check (yardstick: torch's op on the CPU in float32, scale: the sum of
    # the summands' magnitudes); the absolute thresholds stay next to it where the rule is not the tighter bound
    x32 = x_cpu.detach().float().requires_grad_(True)
    want32 = [torch.nn.functional.adaptive_avg_pool2d(x32, (p, p)) for p in sides]
    rep, tols = Report(), []
    for g, w, w32, sc, p in zip(got, want, want32, R.pool_fwd_scale(x_cpu, sides), sides):
        assert g.shape == w.shape
        assert float((g.detach().cpu().double() - w.detach()).abs().max()) < 2e-6, p
        assert rep.check("pool forward", g, w, w32, sc), p
        tols.append(FACTOR * float((w32.detach().double() - w.detach()).abs().max()) + 8 * ULP * float(sc.max()))
    ws = [torch.from_numpy(rs.standard_normal(tuple(w.shape))) for w in want]
    sum((w * k).sum() for w, k in zip(want, ws)).backward()
    sum((g * k.float().to(DEV)).sum() for g, k in zip(got, ws)).backward()
    assert float((x.grad.cpu().double() - x_cpu.grad).abs().max()) < 1e-5
    sum((w * k.float()).sum() for w, k in zip(want32, ws)).backward()
    dscale = R.pool_bwd_scale(ws, None, sides, x_cpu.shape)
    assert rep.check("pool x.grad", x.grad, x_cpu.grad, x32.grad, dscale)
    with capsys.disabled():
        print(rep.table(f"avg_pool_pyramid F {frame}, sides {sides}"))
        print(f"    largest tolerance of the rule: forward {max(tols):.3e} (threshold 2e-6), x.grad "
              f"{FACTOR * rep.rows['pool x.grad'][2] + 8 * ULP * float(dscale.max()):.3e} (threshold 1e-5)")
    # bit-reproducible (torch's CUDA backward adds with float atomics)
    x2 = x.detach().clone().requires_grad_(True)
    sum((g * k.float().to(DEV)).sum() for g, k in zip(ops.avg_pool_pyramid(x2, sides), ws)).backward()
    assert torch.equal(x2.grad, x.grad)
    # a level without a gradient
    x3 = x.detach().clone().requires_grad_(True)
    ops.avg_pool_pyramid(x3, sides)[0].sum().backward()
    x_cpu.grad = None
    torch.nn.functional.adaptive_avg_pool2d(x_cpu, (sides[0], sides[0])).sum().backward()
    assert float((x3.grad.cpu().double() - x_cpu.grad).abs().max()) < 1e-5


@pytest.mark.parametrize("frame,naux,coord,conn,batch", [(224, 7, True, False, 2), (64, 6, False, True, 2), (30, 3, False, False, 3), (32, 4, True, True, 2)])
def test_create_node_pixels_with_the_fused_pyramid_equals_the_torch_pools(monkeypatch, frame, naux, coord, conn, batch):
    """create_node_pixels (models.py:498-537) through eg_avg_pool_pyramid_* + eg_pack_levels as one autograd node against the
    route with torch's adaptive_avg_pool2d per level (EG_POOL_PYRAMID=0): node features to 2e-6, the gradient w.r.t. the frames to
    1e-5 of its largest entry."""
    hip, _ = model_pair(frame, naux, 2, coord=coord, seed=3, use_connection_nodes=conn)
    frames = synthetic_frames(batch, 128, frame, 9).to(DEV)
    coords = initial_coords(batch, frame).to(DEV).reshape(batch, 4, 2) if coord else None
    w = synthetic_frames(1, 1, 64, 3).reshape(-1)[:128].to(DEV)
    res = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("EG_POOL_PYRAMID", knob)
        x = frames.clone().requires_grad_(True)
        feats = hip.create_node_pixels(x, batch, coords)
        (feats * w).sum().backward()
        res[knob] = (feats.detach().clone(), x.grad.clone())
    assert res["1"][0].shape == res["0"][0].shape
    assert float((res["1"][0] - res["0"][0]).abs().max()) < 2e-6
    assert float((res["1"][1] - res["0"][1]).abs().max()) < 1e-5 * float(res["0"][1].abs().max())
