"""-m gpu: the train-mode layer (eg_gcn_layer_train_fwd / _bwd*), the stacked heads (eg_classifier_train_fwd / _bwd*), the
BatchNorm-backward sums the two hand on, and the pieces under them, per quantity against tests/train_reference.py in float64 under
coord_reference.Report's rule: |kernel - fp64| <= 4 max|ref32 - fp64| + 8 ulp x (the sum of the summands' magnitudes).  Inputs come
from the tables of train_reference.py: every ReLU decision is at least the margin away from its kink on the float64 reference alone,
so no element of any compared array is left out."""
import itertools

import numpy as np
import pytest
import torch

import coord_reference as CR
import eval_reference as EV
import train_reference as T
from echoglad_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C = 128
F64, F32 = torch.float64, torch.float32


@pytest.fixture(autouse=True)
def _epoch_zero():
    """The masks hash with seed + epoch: hash_mask writes them out at epoch 0."""
    e0 = ops.dropout_epoch()
    ops.dropout_epoch_set(0)
    yield
    ops.dropout_epoch_set(e0)


def _finish(rep, title, capsys):
    with capsys.disabled():
        print(rep.table(title))
    assert not rep.failed(), rep.failed()


def _both(fn):
    return fn(F64), fn(F32)


def _dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


# ---------------------------------------------------------------------------
# a. the layer
# ---------------------------------------------------------------------------
def _graph(case):
    """(handle, the batch its launches take) of a layer case."""
    E, B, rows = T.layer_edges(case)
    if case[0] == "topo":
        g = ops.Graph.topo(case[1], case[2], case[3], case[4], use_connection_nodes=case[5])
    elif case[0] == "diag":
        g = ops.Graph.topo(case[1], case[2], case[3], case[4], use_connection_nodes=case[5], diag_main=case[6], diag_aux=case[7])
        assert g.structured and g.hybrid
    else:
        g = ops.Graph.csr(torch.from_numpy(T.case_edge_index(case)).to(DEV), rows)
        assert not g.structured and g.kidsum_rows == 0
    assert g.num_nodes * B == rows and g.num_nodes == E[0]
    assert (g.bwd is not g) == (case[0] == "directed")
    return g, B


def _check_layer_forward(rep, tag, got, rm, rv, r64, r32):
    out, z, agg, bn = got
    big = lambda k: float(r64[k].abs().max())
    rep.check("agg", agg, r64["agg"], r32["agg"], r64["agg_scale"])
    rep.check("z", z, r64["z"], r32["z"], r64["z_scale"])
    rep.check("bn mean", bn[0], r64["mean"], r32["mean"], r64["mean_scale"])
    rep.check("bn invstd", bn[1], r64["invstd"], r32["invstd"], big("invstd"))
    rep.check("bn scale", bn[2], r64["scale"], r32["scale"], big("scale"))
    rep.check("bn shift", bn[3], r64["shift"], r32["shift"], r64["shift_scale"])
    rep.check("running_mean", rm, r64["running_mean"], r32["running_mean"], r64["running_mean_scale"])
    rep.check("running_var", rv, r64["running_var"], r32["running_var"], r64["running_var_scale"])
    rep.check("out" + tag, out, r64["out"], r32["out"], big("out"))


def _check_layer_backward(rep, tag, got, r64, r32, need_dx=True, need_dw=True):
    dx, dw, db, dgamma, dbeta = got[:5]
    assert (dx is not None) == need_dx and (dw is not None) == need_dw
    assert float(db.abs().max()) == 0.0                         # a bias in front of a train-mode BatchNorm
    if need_dx:
        rep.check("dx" + tag, dx, r64["dx"], r32["dx"], r64["dx_scale"])
    if need_dw:
        rep.check("dw" + tag, dw, r64["dw"], r32["dw"], r64["dw_scale"])
    rep.check("dgamma" + tag, dgamma, r64["dgamma"], r32["dgamma"], r64["dgamma_scale"])
    rep.check("dbeta" + tag, dbeta, r64["dbeta"], r32["dbeta"], r64["dbeta_scale"])


def _check_child_sums(rep, tag, topo, B, ka, out, r64, r32):
    """kidsum_out of a train forward under the rule, twice: against eval_reference.kidsum of the reference's out (float64, and float32
    as the yardstick; the scale: the same sums over the scale `out` itself is judged with, its largest magnitude), and against
    kidsum of the kernel's OWN out (the kernel sums its own rows: float64 sums of them, float32 sums as the yardstick, the sums of
    their magnitudes as the scale).  Rows of the side buffer that have no children -- connection rows, aux nodes outside the crop, the
    parents of a level that runs node by node -- have scale 0 and are exactly zero."""
    k64, k_scale = EV.kidsum(topo, r64["out"], B, out_scale=torch.full_like(r64["out"], float(r64["out"].abs().max())))
    k32 = EV.kidsum(topo, r32["out"], B, F32)[0]
    assert ka.shape == k64.shape
    rep.check("child sums" + tag, ka, k64, k32, k_scale)
    own64, own_scale = EV.kidsum(topo, out, B)
    own32 = EV.kidsum(topo, out, B, F32)[0]
    rep.check("child sums of its own out" + tag, ka, own64, own32, own_scale)
    never = (k_scale == 0).all(1)
    assert not never.any() or float(ka.cpu()[never].abs().max()) == 0.0


@pytest.mark.parametrize("case", T.LAYER_CASES, ids=str)
def test_train_layer_against_fp64(case, capsys):
    """relu x residual x p in {0, 0.5} on one handle (residual on / off: the producer / consumer and the symmetric dX kernel), every
    need_dx / need_dw form, equal bits on a second call, the child sums every form leaves behind, and once over child sums left by
    a previous launch.  On 'grid-diagonal' handles the train forward and the residual dX are launches of the producer / consumer
    kernel (its {mode 1 / 2, diag} forms), counted on the handle."""
    T.assert_input_condition(T.layer_condition(case))           # on the reference alone, before a kernel is looked at
    g, B = _graph(case)
    E = T.layer_edges(case)[0]
    I = T.layer_inputs(case)
    D = _dev(I)
    rep = CR.Report()
    chained_from = None
    topo = EV.topology(*case[1:-1]) if g.kidsum_rows > 0 else None
    ps = case[0] == "diag" and ops.lower_sums_supported(g.bwd)          # (EG_TRAIN_PS=0: the symmetric kernel throughout)
    for relu, residual, p in itertools.product((False, True), (False, True), (0.0, 0.5)):
        ref = lambda dt, x=I["x"], relu=relu, residual=residual, p=p: T.layer64(
            E, B, x, I["weight"], I["bias"], I["gamma"], I["beta"], I["rmean"], I["rvar"], relu=relu, p=p, seed=T.SEED_L,
            residual=residual, dy=I["dy"], dtype=dt)
        r64, r32 = _both(ref)
        tag = f" relu {int(relu)} res {int(residual)} p {p:g}"

        def fwd(x=D["x"], relu=relu, residual=residual, p=p, **kw):
            rm, rv = D["rmean"].clone(), D["rvar"].clone()
            return ops.gcn_layer_train_fwd(g, B, x, D["weight"], D["bias"], D["gamma"], D["beta"], rm, rv, T.MOMENTUM, T.EPS, relu, p,
                                           T.SEED_L, residual, **kw), rm, rv
        launches = g.ps_launches
        got, rm, rv = fwd()
        assert not ps or g.ps_launches == launches + 1
        _check_layer_forward(rep, tag, got, rm, rv, r64, r32)
        again, rm2, rv2 = fwd()
        assert all(torch.equal(a, b) for a, b in zip(got + (rm, rv), again + (rm2, rv2)))
        out, z, agg, bn = got
        first = None
        for need_dx, need_dw in ((True, True), (True, False), (False, True)):
            bwd = lambda: ops.gcn_layer_bwd(g.bwd, B, D["dy"], z, agg, D["weight"], D["gamma"], D["beta"], bn, relu, p, T.SEED_L, residual,
                                            need_dx, need_dw)
            launches = g.ps_launches
            res = bwd()
            assert not ps or g.ps_launches == launches + (1 if need_dx and residual else 0)
            _check_layer_backward(rep, tag, res, r64, r32, need_dx, need_dw)
            if first is None:
                first = res
                assert all(torch.equal(a, b) for a, b in zip(res, bwd()))
        if g.kidsum_rows > 0:
            # the same launch leaving the child sums of its output behind: the same out under the same bounds, and the sums ...
            ka = ops.new_kidsum(g, B)
            got_k, rm, rv = fwd(kidsum_out=ka)
            _check_layer_forward(rep, tag, got_k, rm, rv, r64, r32)
            _check_child_sums(rep, tag, topo, B, ka, got_k[0], r64, r32)
        if g.kidsum_rows > 0 and relu and residual and p > 0:
            chained_from = (got_k[0], ka)
    if chained_from is not None:
        # ... and a layer on top of it that reads one child-sum row in place of four child rows (no ReLU: no kink, whatever its input)
        x2, ka = chained_from
        r64, r32 = _both(lambda dt: T.layer64(E, B, x2.cpu(), I["weight"], I["bias"], I["gamma"], I["beta"], I["rmean"], I["rvar"], relu=False,
                                              p=0.5, seed=T.SEED_L + 1, residual=True, dy=I["dy"], dtype=dt))
        rm, rv = D["rmean"].clone(), D["rvar"].clone()
        launches = g.ps_launches
        got = ops.gcn_layer_train_fwd(g, B, x2, D["weight"], D["bias"], D["gamma"], D["beta"], rm, rv, T.MOMENTUM, T.EPS, False, 0.5,
                                      T.SEED_L + 1, True, kidsum_in=ka)
        assert not ps or g.ps_launches == launches + 1
        _check_layer_forward(rep, " over child sums", got, rm, rv, r64, r32)
        out, z, agg, bn = got
        res = ops.gcn_layer_bwd(g.bwd, B, D["dy"], z, agg, D["weight"], D["gamma"], D["beta"], bn, False, 0.5, T.SEED_L + 1, True, True, True)
        _check_layer_backward(rep, " over child sums", res, r64, r32)
    else:
        assert g.kidsum_rows == 0
    _finish(rep, f"train layer {case}", capsys)


# ---------------------------------------------------------------------------
# b. the heads
# ---------------------------------------------------------------------------
def _heads_params(P, p):
    """(the eg_cls_train_params dictionary on the device, its running statistics before a step)."""
    G = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in P.items()}
    G.update(p1=p, p2=p, seed1=T.SEED1, seed2=T.SEED2)
    return G, {k: P[k].clone() for k in ("running_mean1", "running_var1", "running_mean2", "running_var2")}


def _heads_forward(G, running, h, B, n, row_lo, n_valid, sigmoid):
    for k, v in running.items():
        G[k] = v.clone().to(DEV)
    return ops.classifier_train_fwd(h, B, n, row_lo, n_valid, G, sigmoid)


def _check_heads_forward(rep, tag, got, G, r64, r32):
    logits, z1, z2, bn = got
    rep.check("logits" + tag, logits, r64["logits"], r32["logits"], r64["logits_scale"])
    rep.check("z1", z1, r64["z1"], r32["z1"], r64["z1_scale"])
    rep.check("z2" + tag, z2, r64["z2"], r32["z2"], r64["z2_scale"])
    at = 0
    for width in (T.H1, T.H2):
        for name in ("mean", "invstd", "scale", "shift"):
            sl = slice(at, at + width)
            at += width
            rep.check(f"bn{1 + (width == T.H2)} {name}", bn[sl], r64["bn"][sl], r32["bn"][sl], r64["bn_scale"][sl])
    assert at == bn.numel() == 768
    for k in ("running_mean1", "running_var1", "running_mean2", "running_var2"):
        rep.check(k, G[k], r64[k], r32[k], r64[k + "_scale"])


def _check_heads_backward(rep, tag, dh, grads, need_dh, B, n, row_lo, n_valid, r64, r32):
    assert (dh is not None) == need_dh
    if need_dh:
        rep.check("dh" + tag, dh, r64["dh"], r32["dh"], r64["dh_scale"])
        drop = ~T.frame_rows(B, n, row_lo, row_lo + n_valid)
        assert not drop.any() or float(dh.cpu()[drop].abs().max()) == 0.0           # exact zeros outside the filter
    grads, at = grads.cpu(), 0
    biggest = float(r64["grads"].abs().max())
    for name, size in T.GRAD_SLICES:
        sl = slice(at, at + size)
        at += size
        if name in ("b1", "b2"):                                 # a bias in front of a train-mode BatchNorm: exactly zero from the kernel
            assert float(grads[sl].abs().max()) == 0.0 and float(r64["grads"][sl].abs().max()) <= 1e-9 * biggest, name
            continue
        rep.check(f"d {name}{tag}", grads[sl], r64["grads"][sl], r32["grads"][sl], r64["grads_scale"][sl])
    assert at == ops.CLS_GRADS_FLOATS == grads.numel()


@pytest.mark.parametrize("case", T.HEADS_CASES, ids=str)
def test_train_heads_against_fp64(case, capsys):
    T.assert_input_condition(T.heads_condition(case))
    n, row_lo, n_valid, B, need_dh = T.heads_shape(case)
    h, dl = T.heads_inputs(case)
    hg, dlg = h.to(DEV), dl.to(DEV)
    rep = CR.Report()
    for p, act in itertools.product((0.0, 0.5), ("logit", "sigmoid")):
        sig = act == "sigmoid"
        P = T.stack_heads(T.oracle_heads(5, act))
        r64, r32 = _both(lambda dt: T.heads64(P, h, B, n, row_lo, n_valid, p, T.SEED1, T.SEED2, sig, dl, dtype=dt))
        G, running = _heads_params(P, p)
        tag = f" p {p:g} {act}"
        got = _heads_forward(G, running, hg, B, n, row_lo, n_valid, sig)
        _check_heads_forward(rep, tag, got, G, r64, r32)
        kept = {k: G[k].clone() for k in running}
        again = _heads_forward(G, running, hg, B, n, row_lo, n_valid, sig)
        assert all(torch.equal(a, b) for a, b in zip(got, again)) and all(torch.equal(kept[k], G[k]) for k in running)
        logits, z1, z2, bn = got
        # (the kernels take the gradient in front of the sigmoid: its slope is the caller's, nn/_train.py heads_bwd)
        dpre = dlg * logits * (1.0 - logits) if sig else dlg
        dh, grads = ops.classifier_bwd(dpre, hg, B, n, row_lo, n_valid, G, z1, z2, bn, need_dh)
        _check_heads_backward(rep, tag, dh, grads, need_dh, B, n, row_lo, n_valid, r64, r32)
        dh2, grads2 = ops.classifier_bwd(dpre, hg, B, n, row_lo, n_valid, G, z1, z2, bn, need_dh)
        assert torch.equal(grads, grads2) and (not need_dh or torch.equal(dh, dh2))
    _finish(rep, f"train heads (n, row_lo, n_valid, B, need_dh) {case}", capsys)


# ---------------------------------------------------------------------------
# c. the BatchNorm-backward sums handed on
# ---------------------------------------------------------------------------
def _kept_layer(rows, seed, shift_mean=0.5):
    """What a train forward keeps of a layer, made up: z with no BatchNorm output near 0 (|z - centre| >= 0.75 in every channel), agg, the
    parameters, and bn [4,128] = mean, invstd from ops.bn_stats, scale, shift.  Float32, CPU; bn on the device."""
    rg = np.random.default_rng(seed)
    f32 = np.float32
    normal = lambda *shape: rg.standard_normal(shape, dtype=f32)
    side = np.where(rg.random((rows, C), dtype=f32) < 0.5, f32(-1), f32(1))
    z = torch.from_numpy(f32(shift_mean) * normal(C) + side * (f32(0.75) + np.abs(normal(rows, C))))
    L = dict(z=z, agg=torch.from_numpy(normal(rows, C)), weight=torch.from_numpy(rg.uniform(-0.15, 0.15, (C, C)).astype(f32)),
             gamma=torch.from_numpy(rg.uniform(0.7, 1.3, C).astype(f32)), beta=torch.from_numpy(rg.uniform(-0.05, 0.05, C).astype(f32)))
    mean, var = ops.bn_stats(z.to(DEV))
    invstd = torch.rsqrt(var + T.EPS)
    scale = L["gamma"].to(DEV) * invstd
    L["bn"] = torch.stack([mean, invstd, scale, L["beta"].to(DEV) - mean * scale]).contiguous()
    y = (z.double() - mean.cpu().double()) * invstd.cpu().double() * L["gamma"].double() + L["beta"].double()
    assert float(y.abs().min()) >= 1e-2 and 0.25 <= float((y > 0).double().mean()) <= 0.75           # the input condition, by construction
    return L


def _check_fed_back(rep, tag, E, B, g, dy, L, relu, p, seed, dy_sums, mask):
    """gcn_layer_bwd of the layer the sums belong to, given them, against the written-out backward on the same tensors."""
    bn = L["bn"].cpu()
    r64, r32 = _both(lambda dt: T.layer_bwd64(E, B, dy.cpu(), L["z"], L["agg"], L["weight"], L["gamma"], L["beta"], bn[0], bn[1], relu, mask,
                                              True, dtype=dt))
    res = ops.gcn_layer_bwd(g.bwd, B, dy, L["z"].to(DEV), L["agg"].to(DEV), L["weight"].to(DEV), L["gamma"].to(DEV), L["beta"].to(DEV),
                            L["bn"], relu, p, seed, True, True, True, dy_sums=dy_sums)
    _check_layer_backward(rep, tag, res, r64, r32)
    own = ops.gcn_layer_bwd(g.bwd, B, dy, L["z"].to(DEV), L["agg"].to(DEV), L["weight"].to(DEV), L["gamma"].to(DEV), L["beta"].to(DEV),
                            L["bn"], relu, p, seed, True, True, True)
    _check_layer_backward(rep, tag + " (own sums)", own, r64, r32)


@pytest.mark.parametrize("case", [(72, 4, 64, 2, True), (340, 0, 340, 2, True)], ids=str)
def test_layer_sums_taken_in_the_heads_backward_against_fp64(case, capsys):
    n, row_lo, n_valid, B, _ = T.heads_shape(case)
    T.assert_input_condition(T.heads_condition(case))
    h, dl = T.heads_inputs(case)
    hg, dlg = h.to(DEV), dl.to(DEV)
    P = T.stack_heads(T.oracle_heads())
    p, relu = 0.5, True
    L = _kept_layer(B * n, seed=n)
    mask = CR.hash_mask(B * n, C, p, T.SEED_L)
    rows = T.frame_rows(B, n, row_lo, row_lo + n_valid)
    bn = L["bn"].cpu()

    def ref(dt):
        r = T.heads64(P, h, B, n, row_lo, n_valid, p, T.SEED1, T.SEED2, False, dl, dtype=dt)
        r["sums"] = T.layer_sums64(r["dh"], L["z"], bn, L["gamma"], L["beta"], relu, mask, rows, dtype=dt)
        return r
    r64, r32 = _both(ref)
    sums_scale = T.layer_sums64(r64["dh_scale"], L["z"], bn, L["gamma"], L["beta"], relu, mask, rows, absolute=True)
    G, running = _heads_params(P, p)
    logits, z1, z2, cbn = _heads_forward(G, running, hg, B, n, row_lo, n_valid, False)
    layer = (L["z"].to(DEV), L["bn"], L["gamma"].to(DEV), L["beta"].to(DEV), relu, p, T.SEED_L)
    assert ops.classifier_layer_sums_supported(B, n, n_valid)
    dh, grads, sums = ops.classifier_bwd(dlg, hg, B, n, row_lo, n_valid, G, z1, z2, cbn, True, layer=layer)
    rep = CR.Report()
    assert sums is not None and sums.dtype == F64
    rep.check("sum g", sums[:C], r64["sums"][:C], r32["sums"][:C], sums_scale[:C])
    rep.check("sum g xhat", sums[C:], r64["sums"][C:], r32["sums"][C:], sums_scale[C:])
    _check_heads_backward(rep, "", dh, grads, True, B, n, row_lo, n_valid, r64, r32)
    dh0, grads0 = ops.classifier_bwd(dlg, hg, B, n, row_lo, n_valid, G, z1, z2, cbn, True)
    assert torch.equal(dh, dh0) and torch.equal(grads, grads0)
    if case[:3] == (340, 0, 340):
        # fed back into the backward of the layer they belong to: the (16, 3) topology has 340 nodes
        g = ops.Graph.topo(16, 3)
        assert g.num_nodes == n
        _check_fed_back(rep, " given the heads' sums", T.topo_edges(16, 3), B, g, dh, L, relu, p, T.SEED_L, (sums, B, row_lo, n_valid), mask)
    _finish(rep, f"layer sums from the heads' backward {case}", capsys)


def test_no_layer_sums_from_the_heads_backward_below_one_tile():
    n, row_lo, n_valid, B, _ = case = (67, 4, 63, 2, True)
    h, dl = T.heads_inputs(case)
    G, running = _heads_params(T.stack_heads(T.oracle_heads()), 0.5)
    logits, z1, z2, cbn = _heads_forward(G, running, h.to(DEV), B, n, row_lo, n_valid, False)
    L = _kept_layer(B * n, seed=n)
    layer = (L["z"].to(DEV), L["bn"], L["gamma"].to(DEV), L["beta"].to(DEV), True, 0.5, T.SEED_L)
    assert not ops.classifier_layer_sums_supported(B, n, n_valid)
    dh, grads, sums = ops.classifier_bwd(dl.to(DEV), h.to(DEV), B, n, row_lo, n_valid, G, z1, z2, cbn, True, layer=layer)
    assert sums is None
    dh0, grads0 = ops.classifier_bwd(dl.to(DEV), h.to(DEV), B, n, row_lo, n_valid, G, z1, z2, cbn, True)
    assert torch.equal(dh, dh0) and torch.equal(grads, grads0)


@pytest.mark.parametrize("handle,B,cut", T.LOWER_SUMS_CASES, ids=str)
def test_layer_sums_handed_down_by_the_dx_launch_against_fp64(handle, B, cut, capsys):
    """`lsums` of gcn_layer_bwd(lower=) against layer_sums64 on the kernel's own dx, on both sides of TILE_SUMS_SMALL (train.hip: one
    launch up to 4096 tiles, two stages above), on handles with coordinate rows, connection nodes (their rows are rows of the frame
    like any other: inside [0, row_hi)) and 'grid-diagonal' levels (the {mode 3, diag} form), over all rows of a frame and with the
    last four left out, for a lower layer with ReLU and dropout, with neither, and with ReLU alone; at the small sizes also fed back
    into the lower layer's backward."""
    frame, naux, main_only, coord, conn, dm, da = handle
    g = ops.Graph.topo(frame, naux, main_only, coord, use_connection_nodes=conn, diag_main=dm, diag_aux=da)
    if not ops.lower_sums_supported(g.bwd):
        pytest.skip("EG_TRAIN_PS=0: the dX launch is the symmetric kernel's, which hands no sums down")
    n = g.num_nodes
    small = g.num_tiles * B <= 4096
    assert small == (frame != 224) and g.hybrid == (dm or da or conn)
    rows = B * n
    E = T.topo_edges(*handle)
    assert E[0] == n
    up, low = _kept_layer(rows, seed=frame), _kept_layer(rows, seed=frame + 1)
    dy = torch.from_numpy(np.random.default_rng(frame + 2).standard_normal((rows, C), dtype=np.float32)).to(DEV)
    seed_l = T.SEED_L + 7
    z_low, bn = low["z"].to(DEV), low["bn"].cpu()
    upper = lambda **kw: ops.gcn_layer_bwd(g.bwd, B, dy, up["z"].to(DEV), up["agg"].to(DEV), up["weight"].to(DEV), up["gamma"].to(DEV),
                                           up["beta"].to(DEV), up["bn"], True, 0.5, T.SEED_L, True, True, True, **kw)
    launches = g.ps_launches
    plain = upper()
    assert g.ps_launches == launches + 1                        # the dX launch is the producer / consumer kernel's
    dxc = plain[0].cpu()
    rep = CR.Report()
    for row_hi, (relu_l, p_l) in itertools.product(cut, ((True, 0.5), (False, 0.0), (True, 0.0))):
        tag = f" row_hi {'n' if row_hi == 0 else f'n - {-row_hi}'} relu {int(relu_l)} p {p_l:g}"
        row_hi += n
        launches = g.ps_launches
        res = upper(lower=(z_low, low["bn"], relu_l, p_l, seed_l, row_hi))
        assert g.ps_launches == launches + 1
        dx, lsums = res[0], res[5]
        assert all(torch.equal(a, b) for a, b in zip(res[:5], plain))       # the by-product changes nothing else
        mask = CR.hash_mask(rows, C, p_l, seed_l) if p_l > 0 else None
        sel = T.frame_rows(B, n, 0, row_hi)
        s64, s32 = _both(lambda dt: T.layer_sums64(dxc, low["z"], bn, None, None, relu_l, mask, sel, dtype=dt))
        scale = T.layer_sums64(dxc.abs(), low["z"], bn, None, None, relu_l, mask, sel, absolute=True)
        assert lsums.dtype == F64 and lsums.numel() == 2 * C
        rep.check("sum g" + tag, lsums[:C], s64[:C], s32[:C], scale[:C])
        rep.check("sum g xhat" + tag, lsums[C:], s64[C:], s32[C:], scale[C:])
        if small:
            _check_fed_back(rep, " given the dX launch's sums," + tag, E, B, g, dx, low, relu_l, p_l, seed_l, (lsums, B, 0, row_hi), mask)
    _finish(rep, f"layer sums from the dX launch, handle {handle} B {B}: {g.num_tiles * B} tiles", capsys)


# ---------------------------------------------------------------------------
# d. the pieces
# ---------------------------------------------------------------------------
def _rows(rows, seed, scale=1.0, offset=0.0):
    rs = np.random.RandomState(seed)
    return torch.from_numpy((rs.standard_normal((rows, C)) * scale + offset).astype(np.float32))


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000])
def test_column_reductions_against_fp64(rows, capsys):
    x, gr = _rows(rows, rows, 2.0, 0.5), _rows(rows, rows + 1)
    xg = x.to(DEV)
    rep = CR.Report()
    xa = x.double().abs()
    rep.check("colsum128", ops.colsum128(xg), x.double().sum(0), x.sum(0), xa.sum(0))
    mean, var = ops.bn_stats(xg)
    m64, m32 = x.double().mean(0), x.mean(0)
    rep.check("bn_stats mean", mean, m64, m32, xa.mean(0))
    rep.check("bn_stats var", var, ((x.double() - m64) ** 2).mean(0), ((x - m32) ** 2).mean(0), ((xa + m64.abs()) ** 2).mean(0))
    rep.check("dweight128", ops.dweight128(gr.to(DEV), xg), gr.double().t() @ x.double(), gr.t() @ x, gr.double().abs().t() @ xa)
    a, b = ops.bn_stats(xg)
    assert torch.equal(a, mean) and torch.equal(b, var)
    _finish(rep, f"column reductions, {rows} rows", capsys)


@pytest.mark.parametrize("rows", [65, 1000])
def test_bn_act_forward_backward_against_fp64(rows, capsys):
    """eg_bn_act_fwd / _bwd with the residual, ReLU and p = 0.5 on the kept tensors of a made-up layer."""
    L = _kept_layer(rows, seed=rows)
    res, dy = _rows(rows, 5), _rows(rows, 6)
    bn = L["bn"].cpu()
    p, seed = 0.5, T.SEED_L + 3
    mask = CR.hash_mask(rows, C, p, seed)
    E = T.edges_of(np.zeros((2, 0), dtype=np.int64), rows)       # no edges: A_hat = I

    def ref(dt):
        y = (L["z"].to(dt) * bn[2].to(dt) + bn[3].to(dt)) * mask.to(dt)
        r = T.layer_bwd64(E, 1, dy, L["z"], L["agg"], L["weight"], L["gamma"], L["beta"], bn[0], bn[1], True, mask, False, dtype=dt)
        r["out"] = torch.relu(y) + res.to(dt)
        return r
    r64, r32 = _both(ref)
    rep = CR.Report()
    out = ops.bn_act_fwd(L["z"].to(DEV), L["bn"][2], L["bn"][3], res.to(DEV), True, p, seed)
    rep.check("out", out, r64["out"], r32["out"], float(r64["out"].abs().max()))
    dz, dgamma, dbeta = ops.bn_act_bwd(dy.to(DEV), L["z"].to(DEV), L["bn"][0], L["bn"][1], L["gamma"].to(DEV), L["beta"].to(DEV), True, p, seed)
    rep.check("dgamma", dgamma, r64["dgamma"], r32["dgamma"], r64["dgamma_scale"])
    rep.check("dbeta", dbeta, r64["dbeta"], r32["dbeta"], r64["dbeta_scale"])
    # dz = gamma invstd (g - sum g / R - xhat sum g xhat / R): the same on magnitudes
    xhat = ((L["z"].double() - bn[0].double()) * bn[1].double()).abs()
    dz_scale = (L["gamma"].double() * bn[1].double()).abs() * (r64["g"].abs() + r64["dbeta_scale"] / rows + xhat * r64["dgamma_scale"] / rows)
    rep.check("dz", dz, r64["dz"], r32["dz"], dz_scale)
    _finish(rep, f"bn_act forward / backward, {rows} rows", capsys)


@pytest.mark.parametrize("rows,width", [(204, 128), (204, 64), (63, 128), (63, 64), (1020, 128)])
def test_the_written_out_mask_is_the_kernels(rows, width):
    for seed in (T.SEED_L, T.SEED1, T.SEED2):
        m = CR.hash_mask(rows, width, 0.5, seed)
        assert torch.equal(CR.kernel_mask(rows, width, 0.5, seed), m)
        assert 0.45 <= float((m > 0).float().mean()) <= 0.55
