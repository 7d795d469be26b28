"""The coordinate-graph kernels (coord.hip, coord_common.h, coord_mlp.hip) against the fp64 reference of tests/coord_reference.py,
at the positions where a resampling goes wrong (collisions, integers, borders, outside the frame) and at the batch sizes where the
kernels change path (4 frames per workgroup of k_bilinear4_bwd; 64 rows = batch 16 between the single-tile and the general landmark
kernels).  Tolerances are measured, not chosen: coord_reference.Report.check, with the same reference in float32 as the yardstick.
The worst ratio per quantity is printed (pytest -s / the log of the GPU run)."""
import copy

import numpy as np
import pytest
import torch

import coord_reference as R
from echoglad_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C = 128
F32 = torch.float32


@pytest.fixture(autouse=True)
def _epoch_zero():
    """The masks hash with seed + epoch: the inputs of the general case were checked on the CPU at epoch 0."""
    e0 = ops.dropout_epoch()
    ops.dropout_epoch_set(0)
    yield
    ops.dropout_epoch_set(e0)


def _rows(rows, seed, width=C):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((rows, width)).astype(np.float32))


def _layout(F, before, extra=0):
    """(n, coord_base, main_base): a guard row in front, the 4 coordinate rows after the main grid (the model's order) or before it
    with a gap row between, two guard rows (+ extra) at the end."""
    if before:
        return 1 + 4 + 1 + F * F + 2 + extra, 1, 6
    return 1 + F * F + 4 + 2 + extra, 1 + F * F, 1


def _finish(rep, title, capsys):
    with capsys.disabled():
        print(rep.table(title))
    assert not rep.failed(), rep.failed()


def _both(fn):
    """The same reference in float64 and in float32."""
    return fn(torch.float64), fn(F32)


# ---------------------------------------------------------------------------
# resampling
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,points,before", [(1, 1, 4, False), (3, 2, 1, True), (4, 5, 4, False), (5, 16, 4, True), (9, 17, 4, False),
                                               (16, 5, 3, True), (17, 16, 5, False), (5, 17, 8, True), (9, 2, 4, True), (17, 5, 4, False),
                                               (1, 16, 8, False), (4, 17, 3, True), (3, 5, 1, False)])
def test_resampling_against_fp64(B, F, points, before, capsys):
    """eg_bilinear4_fwd / _bwd, packed and in rows, points == 4 (every load up front, read-modify-writes forwarded in registers) and
    the walk of any other count."""
    n, cb, mb = _layout(F, before)
    rep = R.Report()
    h = _rows(B * n, 7)
    hg = h.to(DEV)
    inplace = points == 4                       # the model's form: samples into / gradients out of the coordinate rows of the same array
    n_side, row0 = (n, cb) if inplace else (1 + max(points, 4) + 2, 1)
    for k, c in enumerate(R.position_rounds(F, points, B, seed=100 * F + points)):
        cg = torch.from_numpy(c).reshape(B * points, 2).to(DEV)
        dout = _rows(B * points, 50 + k)
        pre = _rows(B * n, 60 + k)             # dh is accumulated into
        if inplace:                             # ... and holds the samples' gradient in its coordinate rows
            pre.view(B, n, C)[:, cb:cb + 4] = dout.view(B, 4, C)
        r64, r32 = _both(lambda dt: R.sample64(h, c, B, n, mb, F, points, dout=dout, dtype=dt))
        # ---- forward
        out = ops.bilinear4_fwd(hg, cg, B, n, mb, F, points=points)
        rep.check("samples", out, r64["out"], r32["out"], float(r64["out"].abs().max()))
        side0 = h if inplace else _rows(B * n_side, 70 + k)
        side = side0.to(DEV)
        assert ops.bilinear4_fwd(side if inplace else hg, cg, B, n, mb, F, points=points, out_rows=(side, n_side, row0)) is None
        sv, s0 = side.cpu().view(B, n_side, C), side0.view(B, n_side, C)
        assert torch.equal(sv[:, row0:row0 + points].reshape(B * points, C), out.cpu())           # the same samples in rows
        assert torch.equal(sv[:, :row0], s0[:, :row0]) and torch.equal(sv[:, row0 + points:], s0[:, row0 + points:])
        assert torch.equal(hg.cpu(), h)
        # ---- backward, packed: dh prefilled
        dh = pre.to(DEV)
        dc = ops.bilinear4_bwd(dout.to(DEV), hg, cg, B, n, mb, F, dh=dh, points=points)
        want64, want32 = pre.double() + r64["dh"], pre + r32["dh"]
        rep.check("d h", dh, want64, want32, float(want64.abs().max()))
        rep.check("d coords", dc, r64["dcoords"], r32["dcoords"], r64["dcoords_scale"])
        untouched = r64["dh"].abs().sum(1) == 0                 # outside the main grid, other frames' rows, pixels no tap reaches
        assert bool(untouched.view(B, n)[:, :mb].all()) and bool(untouched.view(B, n)[:, mb + F * F:].all())
        assert torch.equal(dh.cpu()[untouched], pre[untouched])
        # ---- dh = None; want_dcoords = False
        assert torch.equal(ops.bilinear4_bwd(dout.to(DEV), hg, cg, B, n, mb, F, dh=None, points=points), dc)
        dh2 = pre.to(DEV)
        assert ops.bilinear4_bwd(dout.to(DEV), hg, cg, B, n, mb, F, dh=dh2, want_dcoords=False, points=points) is None
        assert torch.equal(dh2, dh)
        # ---- backward, the gradient read from rows
        dh3 = pre.to(DEV)
        if inplace:
            src = dh3
        else:
            src0 = _rows(B * n_side, 80 + k)
            src0.view(B, n_side, C)[:, row0:row0 + points] = dout.view(B, points, C)
            src = src0.to(DEV)
        dc3 = ops.bilinear4_bwd(None, hg, cg, B, n, mb, F, dh=dh3, points=points, dout_rows=(src, n_side, row0))
        assert torch.equal(dc3, dc) and torch.equal(dh3, dh)
        if not inplace:
            assert torch.equal(src.cpu(), src0)
    _finish(rep, f"resampling B {B} F {F} points {points} coordinate rows {'before' if before else 'after'}", capsys)


def _lower_inputs(B, n, relu, p, seed):
    """(z, bn, keep) of a layer below: mean, inverse deviation, scale and shift that are NOT consistent with each other (gate and
    normalisation are told apart), no gate input within 1e-4 of its kink."""
    rs = np.random.RandomState(seed)
    z = rs.standard_normal((B * n, C)).astype(np.float32)
    mean, invstd = z.mean(0), 1.0 / z.std(0)
    scale = (rs.uniform(0.3, 1.5, C) * rs.choice([-1.0, 1.0], C)).astype(np.float32)
    shift = (0.3 * rs.standard_normal(C)).astype(np.float32)
    near = np.abs(z.astype(np.float64) * scale + shift) < 1e-4
    z[near] += np.float32(0.5)
    assert float(np.abs(z.astype(np.float64) * scale + shift).min()) >= 1e-5
    bn = torch.from_numpy(np.concatenate([mean, invstd, scale, shift]).astype(np.float32))
    keep = R.kernel_mask(B * n, C, p, 999) if p > 0 else torch.ones(B * n, C)
    if p > 0:
        assert set(keep.unique().tolist()) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
    return torch.from_numpy(z), bn, keep


def _taps_refs(r64, r32, z, bn, relu, keep, B, n, mb, F):
    sl = slice(mb, mb + F * F)
    b = bn.view(4, C)
    args = (z.view(B, n, C)[:, sl], b[0], b[1], b[2], b[3], relu, keep.view(B, n, C)[:, sl])
    return (R.tap_sums64(r64["dh"].view(B, n, C)[:, sl], *args), R.tap_sums64(r32["dh"].view(B, n, C)[:, sl], *args, dtype=F32),
            R.tap_sums64(r64["add_abs"], *args, absolute=True))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("B,F,points,before", [(1, 16, 4, False), (5, 5, 4, True), (9, 17, 4, False), (5, 16, 5, False), (9, 5, 3, True)])
def test_tap_sums_of_the_resampling_backward_against_fp64(B, F, points, before, p, relu, capsys):
    """eg_bilinear4_bwd_rows_sums: what the taps add to the BatchNorm-backward sums of the layer below, per frame."""
    n, cb, mb = _layout(F, before)
    rep = R.Report()
    h = _rows(B * n, 7)
    hg = h.to(DEV)
    z, bn, keep = _lower_inputs(B, n, relu, p, 25)
    lower = (z.to(DEV), bn.to(DEV), relu, p, 999)
    inplace = points == 4
    n_side, row0 = (n, cb) if inplace else (1 + max(points, 4) + 2, 1)
    for k, c in enumerate(R.position_rounds(F, points, B, seed=100 * F + points + 1)):
        cg = torch.from_numpy(c).reshape(B * points, 2).to(DEV)
        dout = _rows(B * points, 50 + k)
        pre = _rows(B * n, 60 + k)
        src0 = pre if inplace else _rows(B * n_side, 80 + k)
        src0.view(B, n_side, C)[:, row0:row0 + points] = dout.view(B, points, C)
        r64, r32 = _both(lambda dt: R.sample64(h, c, B, n, mb, F, points, dout=dout, dtype=dt))
        t64, t32, tscale = _taps_refs(r64, r32, z, bn, relu, keep, B, n, mb, F)
        dh = pre.to(DEV)
        src = dh if inplace else src0.to(DEV)
        dc, taps = ops.bilinear4_bwd(None, hg, cg, B, n, mb, F, dh=dh, points=points, dout_rows=(src, n_side, row0), lower=lower)
        rep.check("tap sums", taps, t64, t32, tscale)
        want64 = pre.double() + r64["dh"]
        rep.check("d h", dh, want64, pre + r32["dh"], float(want64.abs().max()))
        rep.check("d coords", dc, r64["dcoords"], r32["dcoords"], r64["dcoords_scale"])
    _finish(rep, f"tap sums B {B} F {F} points {points} relu {relu} p {p}", capsys)


# ---------------------------------------------------------------------------
# the landmark update
# ---------------------------------------------------------------------------
def _params(mlp, p):
    """The eg_cls_train_params dictionary of the 136-32-16-2 head `mlp` (an oracle module on the CPU) and its running statistics."""
    P = {k: t.detach().to(F32).contiguous().to(DEV) for k, t in zip(R.PARAM_NAMES, R.mlp_params(mlp))}
    P.update(eps1=mlp[1].eps, eps2=mlp[5].eps, p1=p, p2=p, momentum1=mlp[1].momentum, momentum2=mlp[5].momentum, seed1=R.SEED1, seed2=R.SEED2)
    running = {"running_mean1": mlp[1].running_mean, "running_var1": mlp[1].running_var,
               "running_mean2": mlp[5].running_mean, "running_var2": mlp[5].running_var}
    return P, {k: v.detach().to(F32).clone() for k, v in running.items()}


def _reset_running(P, running):
    for k, v in running.items():
        P[k] = v.clone().to(DEV)


def _masks(B, p):
    if p <= 0:
        return None, None
    m1, m2 = R.kernel_mask(4 * B, 32, p, R.SEED1), R.kernel_mask(4 * B, 16, p, R.SEED2)
    assert torch.equal(m1, R.hash_mask(4 * B, 32, p, R.SEED1)) and torch.equal(m2, R.hash_mask(4 * B, 16, p, R.SEED2))
    return m1, m2


def _check_forward_state(rep, fw64, fw32, mlp, saved, P, check_stats=True):
    """pre, both BatchNorm inputs and the running statistics of a kernel forward against mlp64's record."""
    z1, z2, _, pre = saved
    w1, b1, w2, b2 = (t.detach().double().abs() for t in (mlp[0].weight, mlp[0].bias, mlp[4].weight, mlp[4].bias))
    rep.check("pre", pre, fw64["pre"], fw32["pre"], float(fw64["pre"].detach().abs().max()))
    rep.check("z1", z1, fw64["z1"], fw32["z1"], fw64["x"].detach().abs() @ w1.t() + b1)
    rep.check("z2", z2, fw64["z2"], fw32["z2"], fw64["h1"].detach().abs() @ w2.t() + b2)
    if check_stats:
        (v64, s64), (v32, _) = R.running_stats(fw64), R.running_stats(fw32)
        for name, a, b, s in zip(("running_mean1", "running_var1", "running_mean2", "running_var2"), v64, v32, s64):
            rep.check(name, P[name], a, b, s)


def _check_grads(rep, grads, g64, g32, scale):
    """The 5042 packed gradients, parameter by parameter; a bias in front of a train-mode BatchNorm: exactly zero from the kernel."""
    grads, at = grads.cpu(), 0
    biggest = float(g64.abs().max())
    for name, size in zip(R.PARAM_NAMES, (32 * 136, 32, 32, 32, 16 * 32, 16, 16, 16, 2 * 16, 2)):
        sl = slice(at, at + size)
        at += size
        if name in ("b1", "b2"):
            assert float(grads[sl].abs().max()) == 0 and float(g64[sl].abs().max()) <= 1e-9 * max(biggest, 1e-30), name
            continue
        rep.check("d " + name, grads[sl], g64[sl], g32[sl], scale[sl])
    assert at == ops.COORD_MLP_GRADS_FLOATS == grads.numel()


UPDATE_CASES = [(B, F, p) for B in (1, 4, 16, 17) for F in (5, 16) for p in (0.0, 0.5)]


def _update_rounds(rep, mlp, B, F, p, n, cb, mb, coords_rounds, h, identity):
    """coord_update_fwd / _bwd on every array of coordinates against update64: dnew given and None, lower given and None."""
    P, running = _params(mlp, p)
    m1, m2 = _masks(B, p)
    hg0 = h.to(DEV)
    for k, c in enumerate(coords_rounds):
        c = torch.as_tensor(c).reshape(4 * B, 2)
        cg = c.to(DEV)
        f64, f32 = _both(lambda dt: R.update64(mlp, h, c, B, n, cb, mb, F, m1, m2, dtype=dt))
        if not identity:
            R.assert_input_condition(f64["fw"])                 # on the reference alone, before the kernel is looked at
        # ---- forward
        hg = hg0.clone()
        _reset_running(P, running)
        (new, again), lm, saved = ops.coord_update_fwd(hg, cg, B, n, cb, mb, P, True, F, True)
        assert torch.equal(new, again) and new.data_ptr() != again.data_ptr()
        assert torch.equal(lm.cpu(), h.view(B, n, C)[:, cb:cb + 4].reshape(4 * B, C))
        rep.check("new", new, f64["new"], f32["new"], float(F - 1))
        _check_forward_state(rep, f64["fw"], f32["fw"], mlp, saved, P)
        if identity:                                            # w3 = b3 = 0: the positions reach the resampling unchanged
            assert torch.equal(saved[3].cpu(), c) and torch.equal(new.cpu(), c.clamp(0, F - 1))
        # the coordinate rows: the main grid sampled at the KERNEL's own new positions, every other row as it was
        s64, s32 = _both(lambda dt: R.sample64(h, new.cpu(), B, n, mb, F, 4, dtype=dt))
        hv = hg.cpu().view(B, n, C)
        rep.check("coordinate rows", hv[:, cb:cb + 4].reshape(4 * B, C), s64["out"], s32["out"], float(s64["out"].abs().max()))
        keep_rows = torch.ones(n, dtype=torch.bool)
        keep_rows[cb:cb + 4] = False
        assert torch.equal(hv[:, keep_rows], h.view(B, n, C)[:, keep_rows])
        # ---- backward from the kernel's forward state
        dx0 = _rows(B * n, 23 + k)
        dnew = _rows(4 * B, 29 + k, 2)
        sl = slice(mb, mb + F * F)
        other = keep_rows.clone()
        other[sl] = False
        for dn, configs in ((dnew, ((True, 0.3), (False, 0.0), None)), (None, ((False, 0.3), (True, 0.0), None))):
            r64, r32 = _both(lambda dt: R.update64(mlp, h, c, B, n, cb, mb, F, m1, m2, dx=dx0, dnew=dn, dtype=dt))
            tag = " (dnew)" if dn is not None else " (no dnew)"
            for cfg in configs:
                lower = None
                if cfg is not None:
                    relu, pl = cfg
                    z, bn, keep = _lower_inputs(B, n, relu, pl, 25 + k)
                    lower = (z.to(DEV), bn.to(DEV), relu, pl, 999)
                dx = dx0.to(DEV)
                dc, grads, taps = ops.coord_update_bwd(dx, None if dn is None else dn.to(DEV), hg, new, lm, cg, B, n, cb, mb, P, F, saved,
                                                       True, lower=lower)
                dxv, d64, d32 = dx.cpu().view(B, n, C), r64["dx"].view(B, n, C), r32["dx"].view(B, n, C)
                rep.check("dx main grid" + tag, dxv[:, sl], d64[:, sl], d32[:, sl], float(d64[:, sl].abs().max()))
                rep.check("d lm" + tag, dxv[:, cb:cb + 4], d64[:, cb:cb + 4], d32[:, cb:cb + 4], float(d64[:, cb:cb + 4].abs().max()))
                assert torch.equal(dxv[:, other], dx0.view(B, n, C)[:, other])
                rep.check("d coords" + tag, dc, r64["dcoords"], r32["dcoords"], r64["dcoords_scale"])
                _check_grads(rep, grads, r64["grads"], r32["grads"], r64["grads_scale"])
                if cfg is None:
                    assert taps is None
                    continue
                b4 = bn.view(4, C)
                args = (z.view(B, n, C)[:, sl], b4[0], b4[1], b4[2], b4[3], relu, keep.view(B, n, C)[:, sl])
                rep.check(f"tap sums relu {int(relu)} p {pl}", taps, R.tap_sums64(r64["add"], *args), R.tap_sums64(r32["add"], *args, dtype=F32),
                          R.tap_sums64(r64["add_abs"], *args, absolute=True))
    return P, running, m1, m2


@pytest.mark.parametrize("B,F,p", UPDATE_CASES)
def test_landmark_update_with_an_identity_head_against_fp64(B, F, p, capsys):
    """w3 = 0, b3 = 0: pre == coords exactly and new == clamp(coords), so every hand-placed position reaches the fused resampling and
    its backward unchanged: the coordinate rows, the taps and their sums, d coords through the inclusive clamp, dW3 and db3."""
    mlp = copy.deepcopy(R.oracle_mlp(3 + B))
    with torch.no_grad():
        mlp[8].weight.zero_()
        mlp[8].bias.zero_()
    n, cb, mb = _layout(F, before=(F == 5))
    rep = R.Report()
    _update_rounds(rep, mlp, B, F, p, n, cb, mb, R.position_rounds(F, 4, B, seed=7 * F + B), _rows(B * n, 21), identity=True)
    _finish(rep, f"landmark update, identity head, B {B} F {F} p {p}", capsys)


@pytest.mark.parametrize("B,F,p", R.GENERAL_CASES)
def test_landmark_update_with_trained_like_weights_against_fp64(B, F, p, capsys):
    """Every one of the 5042 gradients, d lm, d coords and the running statistics of eg_coord_update_fwd / _bwd, and of
    eg_coord_mlp_fwd / _bwd packed and in rows, with inputs that keep every ReLU and clamp decision away from its kink."""
    mlp = R.oracle_mlp(3 + B)
    n, cb, mb = _layout(F, before=(F == 16))
    rep = R.Report()
    lm0, c = R.general_inputs(B, F, p)
    h = _rows(B * n, 21)
    h.view(B, n, C)[:, cb:cb + 4] = lm0.view(B, 4, C)
    P, running, m1, m2 = _update_rounds(rep, mlp, B, F, p, n, cb, mb, [c], h, identity=False)
    # ---- the MLP alone: packed, and on the rows of the node array
    f64, f32 = _both(lambda dt: R.mlp64(mlp, lm0, c, B, F, m1, m2, dtype=dt))
    dnew = _rows(4 * B, 31, 2)
    b64, b32 = R.mlp_backward(f64, dnew), R.mlp_backward(f32, dnew)
    cg, lmg, hg = c.to(DEV), lm0.to(DEV), h.to(DEV)
    _reset_running(P, running)
    new, saved = ops.coord_mlp_fwd(lmg, cg, B, P, True, F, True)
    rep.check("new (mlp)", new, f64["new"], f32["new"], float(F - 1))
    _check_forward_state(rep, f64, f32, mlp, saved, P)
    _reset_running(P, running)
    lm_out = torch.empty(4 * B, C, device=DEV)
    new_r, saved_r = ops.coord_mlp_fwd(lm_out, cg, B, P, True, F, True, in_rows=(hg, n, cb))
    assert torch.equal(new_r, new) and torch.equal(lm_out, lmg) and all(torch.equal(a, b) for a, b in zip(saved_r, saved))
    assert torch.equal(hg.cpu(), h)
    dlm, dc, grads = ops.coord_mlp_bwd(dnew.to(DEV), lmg, cg, B, P, F, saved, True, True)
    rep.check("d lm (mlp)", dlm, b64["dlm"], b32["dlm"], float(b64["dlm"].abs().max()))
    rep.check("d coords (mlp)", dc, b64["dcoords"], b32["dcoords"], b64["dcoords_scale"])
    _check_grads(rep, grads, b64["grads"], b32["grads"], b64["grads_scale"])
    none_lm, none_dc, grads2 = ops.coord_mlp_bwd(dnew.to(DEV), lmg, cg, B, P, F, saved, False, False)
    assert none_lm is None and none_dc is None and torch.equal(grads2, grads)
    for accumulate in (False, True):
        dx0 = _rows(B * n, 33)
        dx = dx0.to(DEV)
        _, dc_r, grads_r = ops.coord_mlp_bwd(dnew.to(DEV), lmg, cg, B, P, F, saved, True, True, out_rows=(dx, n, cb), accumulate=accumulate)
        want = dx0.to(DEV)
        rows = want.view(B, n, C)[:, cb:cb + 4]
        want.view(B, n, C)[:, cb:cb + 4] = (rows + dlm.view(B, 4, C)) if accumulate else dlm.view(B, 4, C)
        assert torch.equal(dx, want) and torch.equal(dc_r, dc) and torch.equal(grads_r, grads)
    _finish(rep, f"landmark update, trained-like weights, B {B} F {F} p {p}", capsys)


# ---------------------------------------------------------------------------
# operands that are not 16-byte aligned
# ---------------------------------------------------------------------------
def _off4(t):
    """A contiguous copy of t that starts 4 bytes into a larger buffer."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("B", [4, 17])
def test_landmark_mlp_scalar_fallbacks_for_unaligned_operands_fill_the_same_tiles(B):
    """stage_inputs and load_weights branch on the alignment of lm and of w1 | w2 and fill the same LDS tile either way: the results
    are the aligned run's, bit for bit.  (Both kernels read lm, w1 and w2 through these two functions only; every other operand stays
    aligned -- the resampling kernels and the dW1 store use unguarded 8- and 16-byte accesses.)"""
    F, p = 16, 0.5
    mlp = R.oracle_mlp(3 + B)
    P, running = _params(mlp, p)
    lm0, c = R.general_inputs(B, F, p)
    lmg, cg, dnew = lm0.to(DEV), c.to(DEV), _rows(4 * B, 31, 2).to(DEV)
    assert lmg.data_ptr() % 16 == 0 and P["w1"].data_ptr() % 16 == 0 and P["w2"].data_ptr() % 16 == 0

    def run(lm, Q):
        _reset_running(Q, running)
        new, saved = ops.coord_mlp_fwd(lm, cg, B, Q, True, F, True)
        dlm, dc, grads = ops.coord_mlp_bwd(dnew, lm, cg, B, Q, F, saved, True, True)
        return [new, *saved, dlm, dc, grads] + [Q[k] for k in sorted(running)]

    base = run(lmg, P)
    for got in (run(_off4(lmg), P), run(lmg, dict(P, w1=_off4(P["w1"]), w2=_off4(P["w2"])))):
        assert len(got) == len(base) and all(torch.equal(a, b) for a, b in zip(got, base))
