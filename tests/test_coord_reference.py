"""The fp64 reference of the coordinate-graph kernels (tests/coord_reference.py), checked by independent formulations on the CPU:
the dense hat-weight formula against a four-tap gather / scatter written from floor(), the tap sums against autograd through
keep * relu(BatchNorm), the fused update's hand-composed backward against autograd through its forward as one expression; and
the inputs of the GPU tests' general case against the condition that keeps every ReLU and clamp decision away from its kink."""
import copy

import numpy as np
import pytest
import torch

import coord_reference as R
from oracle import gnn_oracle as O

C = 128
F64 = torch.float64


def _rows(rows, seed):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((rows, C)).astype(np.float32))


def _four_tap(h, coords, B, n, main_base, F, points, dout):
    """(out, dh, dcoords) in double from floor(): taps i0 = floor(c), i0 + 1 with weight 1 - |c - i| where 0 <= i < F and the weight is
    positive; derivative -sign(c - i) of such a tap, so 0 at c == i, 0 for a tap of weight exactly 0 and 0 outside the frame."""
    h, c, dout = h.double(), torch.as_tensor(coords).double().reshape(B * points, 2), dout.double()
    out, dh, dc = torch.zeros(B * points, C, dtype=F64), torch.zeros_like(h), torch.zeros(B * points, 2, dtype=F64)

    def taps(x):
        res = []
        for k in range(2):
            i = int(np.floor(x)) + k
            d = x - i
            w = 1.0 - abs(d)
            if 0 <= i < F and w > 0.0:
                res.append((i, w, -float(np.sign(d))))
        return res

    for p in range(B * points):
        base = (p // points) * n + main_base
        for i, wi, dwi in taps(float(c[p, 0])):
            for j, wj, dwj in taps(float(c[p, 1])):
                row = base + i * F + j
                out[p] += wi * wj * h[row]
                dh[row] += wi * wj * dout[p]
                dot = float(dout[p] @ h[row])
                dc[p, 0] += dwi * wj * dot
                dc[p, 1] += wi * dwj * dot
    return out, dh, dc


def _close(a, b, rel=1e-12):
    return float((a - b).abs().max()) <= rel * max(float(b.abs().max()), 1e-300) or float((a - b).abs().max()) == 0.0


@pytest.mark.parametrize("F", [1, 2, 5, 16, 17])
@pytest.mark.parametrize("points,B", [(4, 5), (1, 9), (3, 4)])
def test_dense_formula_equals_the_four_tap_form_at_every_hand_placed_position(F, points, B):
    n, mb = 4 + F * F + 3, 4
    h = _rows(B * n, 7)
    rounds = R.position_rounds(F, points, B, seed=3)
    placed = {tuple(np.float32(q)) for g in R.hand_positions(F) for q in g}
    seen = {tuple(q) for c in rounds for q in c.reshape(-1, 2)}
    assert placed <= seen                                   # every hand-placed position is in some round
    for k, c in enumerate(rounds):
        dout = _rows(B * points, 11 + k)
        s = R.sample64(h, c, B, n, mb, F, points, dout=dout)
        out, dh, dc = _four_tap(h, c, B, n, mb, F, points, dout)
        assert _close(s["out"], out) and _close(s["dh"], dh) and _close(s["dcoords"], dc), (F, points, k)
        assert bool((s["dcoords_scale"] >= s["dcoords"].abs() * (1 - 1e-12)).all())
        assert float(s["dh"].view(B, n, C)[:, :mb].abs().max()) == 0 and float(s["dh"].view(B, n, C)[:, mb + F * F:].abs().max()) == 0


def test_kink_conventions_of_the_dense_formula():
    F, n, mb = 5, 4 + 25, 4
    h = _rows(n, 1)
    c = np.array([[2.0, 3.0], [-1.0, 2.5], [2.5, 5.0], [1.0, 2.5]], dtype=np.float32)
    s = R.sample64(h, c, 1, n, mb, F, 4, dout=_rows(4, 2))
    assert torch.equal(s["out"][0], h[mb + 2 * F + 3].double())              # an integer position is the pixel itself
    assert float(s["dcoords"][0].abs().max()) == 0                           # 0 at c == i, 0 for the taps of weight exactly 0
    assert float(s["out"][1].abs().max()) == 0 and float(s["dcoords"][1].abs().max()) == 0       # -1: the only tap has weight 0
    assert float(s["out"][2].abs().max()) == 0 and float(s["dcoords"][2].abs().max()) == 0       # F: outside
    assert float(s["dcoords"][3, 0]) == 0 and float(s["dcoords"][3, 1]) != 0                     # the kink along h only


@pytest.mark.parametrize("relu", [False, True])
def test_tap_sums_equal_autograd_through_the_layers_activation(relu):
    B, rows = 3, 25
    rs = np.random.RandomState(5)
    add, z = (torch.from_numpy(rs.standard_normal((B, rows, C))) for _ in range(2))
    keep = torch.from_numpy((rs.uniform(size=(B, rows, C)) > 0.3) / 0.7)
    mean, gamma, beta = (torch.from_numpy(rs.standard_normal(C)) for _ in range(3))
    invstd = torch.from_numpy(rs.uniform(0.5, 2.0, C))
    scale, shift = gamma * invstd, beta - mean * gamma * invstd
    got = R.tap_sums64(add, z, mean, invstd, scale, shift, relu, keep)
    assert got.shape == (B, 2, C)
    for b in range(B):
        g, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        y = g * (z[b] - mean) * invstd + be
        f = keep[b] * (torch.relu(y) if relu else y)
        dg, db = torch.autograd.grad(f, (g, be), add[b])
        assert _close(got[b, 0], db) and _close(got[b, 1], dg)
    big = R.tap_sums64(add.abs(), z, mean, invstd, scale, shift, relu, keep, absolute=True)
    assert bool((big >= got.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("coord_base,main_base", [(25, 0), (1, 6)])
@pytest.mark.parametrize("with_dnew", [False, True])
def test_update_backward_equals_autograd_through_its_forward(coord_base, main_base, with_dnew):
    B, F = 3, 5
    n = 4 + F * F + 3
    rs = np.random.RandomState(9)
    mlp = R.oracle_mlp(4)
    h = _rows(B * n, 3)
    c = torch.from_numpy(rs.uniform(-0.5, F - 0.5, (4 * B, 2)).astype(np.float32))
    m1 = torch.from_numpy(((rs.uniform(size=(4 * B, 32)) > 0.5) * 2.0))
    m2 = torch.from_numpy(((rs.uniform(size=(4 * B, 16)) > 0.5) * 2.0))
    dx = _rows(B * n, 4)
    dnew = torch.from_numpy(rs.standard_normal((4 * B, 2))) if with_dnew else None
    got = R.update64(mlp, h, c, B, n, coord_base, main_base, F, m1, m2, dx=dx, dnew=dnew)
    z, keep = _rows(B * n, 5), torch.from_numpy((rs.uniform(size=(B * n, C)) > 0.3) / 0.7)
    bn = torch.from_numpy(rs.uniform(0.5, 1.5, (4, C)))
    low = R.update64(mlp, h, c, B, n, coord_base, main_base, F, m1, m2, dx=dx, dnew=dnew, lower=(z, bn, True, keep))
    sl = slice(main_base, main_base + F * F)
    gained = (got["dx"] - dx.double()).view(B, n, C)[:, sl]
    assert _close(got["add"], gained, 1e-9) and torch.equal(low["dx"], got["dx"])
    assert _close(low["taps"], R.tap_sums64(got["add"], z.view(B, n, C)[:, sl], bn[0], bn[1], bn[2], bn[3], True, keep.view(B, n, C)[:, sl]))
    assert bool((low["taps_scale"] >= low["taps"].abs() * (1 - 1e-12)).all())
    # the forward as ONE differentiable expression
    m = copy.deepcopy(mlp).double().train()
    hl, cl = h.double().requires_grad_(True), c.double().requires_grad_(True)
    rows = hl.view(B, n, C)[:, coord_base:coord_base + 4].reshape(4 * B, C)
    cc = cl.view(B, 4, 2)
    x = torch.cat((rows, (cc.unsqueeze(1) - cc.unsqueeze(2)).reshape(4 * B, 8)), 1)
    a = torch.relu(m[1](m[0](x))) * m1
    b = torch.relu(m[5](m[4](a))) * m2
    new = torch.clamp(cc + m[8](b).view(B, 4, 2), min=0, max=F - 1)
    main = hl.view(B, n, C)[:, main_base:main_base + F * F].permute(0, 2, 1).reshape(B, C, F, F)
    samples = torch.cat([O.bilinear_interpolation_dense(new[k], main[k]) for k in range(B)])
    after = hl.view(B, n, C).clone()
    after[:, coord_base:coord_base + 4] = samples.view(B, 4, C)
    loss = (after.reshape(B * n, C) * dx.double()).sum()
    if with_dnew:
        loss = loss + (new.reshape(4 * B, 2) * dnew).sum()
    g = torch.autograd.grad(loss, [hl, cl] + R.mlp_params(m))
    assert _close(got["h"], after.detach().reshape(B * n, C)) and _close(got["new"], new.detach().reshape(4 * B, 2))
    assert 0 < int(((new == 0) | (new == F - 1)).sum()) < new.numel()
    assert _close(got["dx"], g[0]) and _close(got["dcoords"], g[1])
    packed = torch.cat([t.reshape(-1) for t in g[2:]])
    assert packed.numel() == 5042
    assert float((got["grads"] - packed).abs().max()) <= 1e-12 * float(packed.abs().max())
    assert bool((got["grads_scale"] >= 0).all()) and bool((got["dcoords_scale"] >= got["dcoords"].abs() * (1 - 1e-9)).all())


def test_hash_mask_is_a_mask_with_the_asked_keep_rate():
    m = R.hash_mask(64, 32, 0.5, R.SEED1)
    assert set(m.unique().tolist()) == {0.0, 2.0} and 0.45 < float((m > 0).float().mean()) < 0.55
    assert not torch.equal(m, R.hash_mask(64, 32, 0.5, R.SEED2)) and torch.equal(R.hash_mask(3, 16, 0.0, 1), torch.ones(3, 16))


@pytest.mark.parametrize("B,F,p", R.GENERAL_CASES)
def test_general_case_inputs_keep_every_decision_away_from_its_kink(B, F, p):
    """The condition the GPU tests of the landmark update assert before they look at the kernel, evaluated here for every case."""
    lm, c = R.general_inputs(B, F, p)
    m1 = R.hash_mask(4 * B, 32, p, R.SEED1) if p > 0 else None
    m2 = R.hash_mask(4 * B, 16, p, R.SEED2) if p > 0 else None
    R.assert_input_condition(R.mlp64(R.oracle_mlp(3 + B), lm, c, B, F, m1, m2))
