"""The fp64 reference of the heat-map losses, decode and evaluator record (tests/heatmap_reference.py), checked without a GPU:
against oracle/loss_oracle.py run in float64 and the reference project's recorded fp32 values on the two golden fixtures, the tie
rule on hand-made maps, and every input builder of tests/test_gpu_heatmap_edges.py against the condition it was built for -- a
case that misses its condition fails here, not silently on the GPU."""
import os

import numpy as np
import pytest
import torch

import heatmap_reference as H
from oracle import loss_oracle as LO

F64 = torch.float64
FIXTURES = ["decode_f16_a3.npz", "decode_f30_a3.npz"]


def _rel(a, b):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("name", FIXTURES)
def test_losses_agree_with_the_oracle_in_float64_and_with_the_recorded_values(golden_dir, name):
    d = np.load(os.path.join(golden_dir, name))
    B, F, naux = int(d["batch"]), int(d["frame"]), int(d["naux"])
    levels = LO.level_grids(F, naux)
    n = d["logits"].shape[0] // B
    assert H.n_rows_of(levels) == n
    lg = torch.from_numpy(d["logits"]).double().requires_grad_(True)
    y, v = torch.from_numpy(d["labels"]).double(), torch.from_numpy(d["valid"]).double()
    o_bce = LO.weighted_bce_with_logits(lg.view(B, n, 4), y.view(B, n, 4), v, ones_weight=9000, loss_weight=1)
    og_bce, = torch.autograd.grad(o_bce, lg)
    o_elm = LO.expected_landmark_mse(lg, y, v, B, F, naux, loss_weight=10)
    og_elm, = torch.autograd.grad(o_elm, lg)

    r = H.criteria(d["logits"], d["labels"], d["valid"], B, levels, 9000, 1.0, 10.0)
    g_bce, = torch.autograd.grad(r["bce"], r["x"], retain_graph=True)
    g_elm, = torch.autograd.grad(r["elm"], r["x"], retain_graph=True)
    g_tot, = torch.autograd.grad(r["total"], r["x"])
    assert _rel(r["bce"].detach(), o_bce.detach()) < 1e-13 and _rel(r["elm"].detach(), o_elm.detach()) < 1e-12
    assert _rel(g_bce.reshape(-1, 4), og_bce) < 1e-13 and _rel(g_elm.reshape(-1, 4), og_elm) < 1e-11
    assert _rel(g_tot, g_bce + g_elm) < 1e-15
    # the reference project's own fp32 numbers, to the fixtures' existing tolerances (tests/test_oracle.py)
    assert abs(float(r["bce"].detach()) - float(d["bce"])) <= 1e-5 * abs(float(d["bce"]))
    assert abs(float(r["elm"].detach()) - float(d["elm"])) <= 1e-5 * abs(float(d["elm"]))
    assert np.allclose(g_elm.reshape(-1, 4).numpy(), d["grad_elm"], rtol=1e-4, atol=1e-8)
    # d bce / d x = w v (sigmoid(x) - y) / sum(v): where y = 1 and sigmoid(x) is close to 1 the RECORDED fp32 value carries the
    # cancellation error 2^-24 (sigmoid + y) of its own subtraction (x = 7.87: 6e-5 of the entry), which no fp64 value can follow.  So:
    # the same code in float32 meets the fixtures' tolerance as it stands, and the fp64 run meets it plus one ulp of the entry's scale.
    e = np.abs(g_bce.reshape(-1, 4).numpy() - d["grad_bce"])
    assert (e <= 1e-9 + 1e-5 * np.abs(d["grad_bce"]) + H.ULP * r["gs_bce"].reshape(-1, 4).numpy()).all()
    assert (e <= 1e-9 + 1e-5 * np.abs(d["grad_bce"]))[np.asarray(d["labels"]).reshape(-1, 4) != 1].all()
    # the scales bound the values they belong to
    assert r["s_bce"] >= float(r["bce"].detach()) > 0 and r["s_elm"] >= float(r["elm"].detach()) > 0
    assert (r["gs_bce"].reshape(-1) * (1 + 1e-12) >= g_bce.reshape(-1).abs()).all()
    assert (r["gs_elm"].reshape(-1) * (1 + 1e-9) >= g_elm.reshape(-1).abs()).all()
    # the same code in float32 is close to itself in float64
    r32 = H.criteria(d["logits"], d["labels"], d["valid"], B, levels, 9000, 1.0, 10.0, dtype=torch.float32)
    assert r32["total"].dtype == torch.float32 and _rel(r32["total"].detach(), r["total"].detach()) < 1e-5
    g32, = torch.autograd.grad(r32["bce"], r32["x"])
    assert np.allclose(g32.reshape(-1, 4).numpy(), d["grad_bce"], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("name", FIXTURES)
def test_decode_and_record_agree_with_the_oracle_in_float64_and_with_the_recorded_values(golden_dir, name):
    d = np.load(os.path.join(golden_dir, name))
    B, F = int(d["batch"]), int(d["frame"])
    n = d["logits"].shape[0] // B
    want = LO.evaluate_landmarks(torch.from_numpy(d["logits"]).double(), torch.from_numpy(d["labels"]).double(),
                                 torch.from_numpy(d["pix2mm_x"]).double(), torch.from_numpy(d["pix2mm_y"]).double(),
                                 torch.from_numpy(d["valid"]).double(), B, F)
    dec = H.decode(d["logits"], B, [(n - F * F, F)], d["labels"], d["valid"])
    assert np.array_equal(dec["argmax"][:, 0].numpy(), d["argmax_main"])
    assert np.array_equal(dec["gt"][:, 0].numpy(), d["gt_coords"]) and np.array_equal(dec["gt"][:, 0].numpy(), want["gt_coords"].numpy())
    assert _rel(dec["expect"][:, 0], want["pred_coords"]) < 1e-13
    assert np.allclose(dec["expect"][:, 0].numpy(), d["pred_coords"], rtol=1e-6, atol=1e-5)
    rec = H.record(dec["expect"][:, 0], dec["gt"][:, 0], dec["vmean"][:, 0], d["pix2mm_x"], d["pix2mm_y"])
    h = rec["history"]
    got = {"lvid_top": h[0], "lvid_bot": h[1], "lvpw": h[2], "ivs": h[3], "ivs_w": h[8], "lvid_w": h[9], "lvpw_w": h[10],
           "ivs_mpe": h[11], "lvid_mpe": h[12], "lvpw_mpe": h[13]}
    for k, val in got.items():
        assert abs(float(val) - want[k]) <= 1e-12 * max(1.0, abs(want[k])), k
    assert [bool(f) for f in h[4:8]] == want["present"] and float(h[14]) == 0 and float(h[15]) == 0
    for k, w in zip(d["last_keys"], d["last_vals"]):
        assert abs(float(got[str(k)]) - float(w)) <= 1e-5 * max(1.0, abs(float(w))), k
    det = rec["detail"]
    assert torch.equal(det[:, 0:8].reshape(B, 4, 2), dec["expect"][:, 0]) and torch.equal(det[:, 8:16].reshape(B, 4, 2), dec["gt"][:, 0].double())
    for j, k in enumerate(("pred_ivs_mm", "pred_lvid_mm", "pred_lvpw_mm", "gt_ivs_mm", "gt_lvid_mm", "gt_lvpw_mm")):
        assert _rel(det[:, 16 + j], want["widths"][k]) < 1e-13, k
    for k, w in zip(d["width_keys"], d["width_vals"]):
        j = ("pred_ivs_mm", "pred_lvid_mm", "pred_lvpw_mm", "gt_ivs_mm", "gt_lvid_mm", "gt_lvpw_mm").index(str(k))
        assert np.allclose(det[:, 16 + j].numpy(), w, rtol=1e-5, atol=1e-5), k
    assert (rec["history_scale"][[0, 1, 2, 3, 8, 9, 10]] * (1 + 1e-12) >= h[[0, 1, 2, 3, 8, 9, 10]].abs()).all()


def test_the_tie_rule_on_hand_made_label_maps():
    S = 7
    y = np.zeros((5, S, S, 4), np.float32)
    y[0, 1, 5, :] = 1
    y[0, 4, 2, :] = 1                     # two separated maxima: (1, 5) and (4, 2) -> (1, 2), which holds no maximum
    # frame 1: all zeros -> (0, 0)
    y[2, 3, :, :] = 0.5                   # a whole row equal -> (3, 0)
    y[3, :, 6, :] = 0.5                   # a whole column equal -> (0, 6)
    y[4, 2, 2, 0], y[4, 2, 4, 0], y[4, 5, 1, 0] = 0.25, 0.75, 0.75       # (2, 4) and (5, 1) -> (2, 1)
    got = H.label_coords(y)
    assert got[0].tolist() == [[1, 2]] * 4 and y[0, 1, 2, 0] == 0
    assert got[1].tolist() == [[0, 0]] * 4
    assert got[2].tolist() == [[3, 0]] * 4
    assert got[3].tolist() == [[0, 6]] * 4
    assert got[4, 0].tolist() == [2, 1]
    # the same through decode, and the oracle's restatement agrees
    flat = torch.from_numpy(y.reshape(5 * S * S, 4))
    d = H.decode(torch.zeros(5 * S * S, 4), 5, [(0, S)], flat, torch.ones(5 * S * S, 4))
    assert np.array_equal(d["gt"][:, 0].numpy(), got) and np.array_equal(LO.gt_coords(torch.from_numpy(y)).numpy(), got)
    # constant logits: arg max 0 and the expectation exactly the centre
    assert d["argmax"].eq(0).all() and d["expect"].eq((S - 1) / 2).all() and d["vmean"].eq(1).all()
    # first arg max among equal maxima
    x = np.zeros((S * S, 4), np.float32)
    x[[30, 9, 41], 1] = 2.5
    assert H.decode(x, 1, [(0, S)])["argmax"][0, 0].tolist() == [0, 9, 0, 0]


@pytest.mark.parametrize("name", list(H.GEOMETRY) + ["cfg5"])
def test_geometry_builders_meet_their_conditions(name):
    levels, n_rows, batch = H.geometry_case(name)
    assert all(s + side * side <= n_rows for s, side in levels)
    if name == "cfg5":
        from echoglad_amd import losses
        assert levels == losses.level_grids(448, 8) and n_rows == levels[-1][0] + 448 * 448


TIE_CASES = [(lv, ks) for lv, side in H.TIE_LEVELS.items() for ks in H.tie_sets(side)]


def test_every_tie_kind_is_placed_where_the_level_has_room_for_it():
    for lv, side in H.TIE_LEVELS.items():
        have = {k for l, ks in TIE_CASES if l == lv for k in ks}
        want = set(H.TIE_KINDS) - ({"round", "higher"} if H.n_chunks(side) <= H.WAVE else set())
        assert have == want, (lv, have)


@pytest.mark.parametrize("what", ["logits", "labels"])
@pytest.mark.parametrize("level,kinds", TIE_CASES)
def test_tie_builders_meet_their_conditions(level, kinds, what):
    levels, n_rows, batch, x, y, v, li, frame, expected = H.tie_case(level, kinds, what)
    d = H.decode(x, batch, levels, y, v)
    side = levels[li][1]
    for c, kind in enumerate(kinds):
        if what == "logits":
            assert int(d["argmax"][frame, li, c]) == expected[c], (kind, c)
            if kind == "all":
                # (torch's fp64 softmax is within rounding of the centre; the kernel's sums are exact, tests/test_gpu_heatmap_edges.py)
                assert (d["expect"][frame, li, c] - (side - 1) / 2).abs().max() < 1e-10
        else:
            assert tuple(d["gt"][frame, li, c].tolist()) == expected[c], (kind, c)
    assert torch.isfinite(d["expect"]).all()


@pytest.mark.parametrize("kind", H.RANGE_KINDS)
@pytest.mark.parametrize("level", list(H.RANGE_LEVELS))
def test_range_builders_meet_their_conditions(level, kind):
    levels, n_rows, batch, x, rows = H.range_case(level, kind)
    g = np.random.RandomState(1).standard_normal((batch, 1, 4, 2)).astype(np.float32)
    d, dx, scale = H.expect_backward(x, batch, levels, g)
    assert torch.isfinite(d["expect"]).all() and torch.isfinite(dx).all() and torch.isfinite(scale).all()
    assert (scale * (1 + 1e-9) >= dx.abs()).all()
    dx = dx.view(batch, n_rows, 4)
    for c in range(4):
        if kind == "neginf":
            assert dx[:, rows[c], c].eq(0).all()
        if kind == "peak30":
            r = rows[c][0]
            side = levels[0][1]
            assert (d["expect"][:, 0, c].detach() - torch.tensor([r // side, r % side], dtype=F64)).abs().max() < 0.2


CRIT = H.criteria_cases()


def test_criteria_cases_cover_what_they_are_there_for():
    assert {c[0] for c in CRIT} == set(H.CRIT_BATCHES) and {c[1] for c in CRIT} == set(H.CRIT_FORMS)
    nine = {(c[1], c[2], c[3]) for c in CRIT if c[0] == 9 and not c[4]}
    assert len(nine) == 2 * 3 * 3 and sum(1 for c in CRIT if c[4]) == 2
    for B in H.CRIT_BATCHES:
        assert {c[1] for c in CRIT if c[0] == B} == set(H.CRIT_FORMS)


@pytest.mark.parametrize("B,form,valid_form,ow,gaps", [c for c in CRIT if c[0] <= 17])
def test_criteria_builders_meet_their_conditions(B, form, valid_form, ow, gaps):
    levels, n_rows, x, y, v, cp, cy = H.criteria_case(B, form, valid_form, gaps)
    r = H.criteria(x, y, v, B, levels, ow, 1.0, 10.0, cp, cy, 0.5, probs=form[0] == "probs", l1=form[1] == "mae")
    gx, gc = torch.autograd.grad(r["total"], [r["x"], r["c"]])
    assert all(torch.isfinite(r[k]).all() for k in ("total", "bce", "elm", "coord")) and torch.isfinite(gx).all()
    if valid_form == "channel2_invalid":
        # the slot contributes nothing: no gradient reaches channel 2, and the loss does not move with its logits
        assert gx[:, :, 2].eq(0).all() and r["d"]["vmean"][:, :, 2].eq(0).all()
    if form[1] == "mae":
        assert gc[1].eq(0).all()                               # sign(0) = 0


@pytest.mark.parametrize("B", [224, 225])
def test_criteria_builders_of_the_large_batches_meet_their_conditions(B):
    H.criteria_case(B, H.CRIT_FORMS[0], "binary", False)


@pytest.mark.parametrize("probs", [False, True])
@pytest.mark.parametrize("n", H.BCE_SIZES)
def test_bce_builders_meet_their_conditions(n, probs):
    x, y, v = H.bce_case(n, probs)
    if n > 100000:
        return                                                 # (the builder's own assertions; the fp64 value is taken on the GPU box)
    xt = H.t(x).requires_grad_(True)
    loss, scale, gscale = H.bce(xt, y, v, 9000.0, probs)
    g, = torch.autograd.grad(loss, xt)
    assert torch.isfinite(loss) and torch.isfinite(g).all() and scale >= float(loss.detach()) >= 0
    assert (gscale * (1 + 1e-9) >= g.abs()).all()
    if probs and n >= 3:
        # torch's clamps on the exact 0 / 1 probabilities: p = 0, y = 1 costs 100 and has the gradient -1e12 * w / sum(valid)
        sv = float(n if v is None else v.sum())
        assert abs(float(g[2]) + 1e12 * 9000.0 / sv) <= 1e-7 * 1e12 * 9000.0 / sv          # (the floor is the FLOAT nearest 1e-12)


@pytest.mark.parametrize("B", H.RECORD_BATCHES)
def test_record_builders_meet_their_conditions(B):
    pred, gt, px, py = H.record_coord_case(B)
    r = H.record(pred, gt, None, px, py)
    h = r["history"]
    assert torch.isfinite(h[:11]).all() and h[4:8].eq(1).all() and torch.isfinite(h[[11, 13]]).all()
    assert torch.isnan(h[12]) if B % 2 == 0 else torch.isposinf(h[12])
    r32 = H.record(pred, gt, None, px, py, dtype=torch.float32)
    assert H.same_nonfinite(r32["history"], h)


def test_record_heat_map_builder_meets_its_conditions():
    x, y, v, px, py, n_rows = H.record_hm_case()
    B, F = 257, 4
    d = H.decode(x, B, [(n_rows - F * F, F)], y, v)
    r = H.record(d["expect"][:, 0], d["gt"][:, 0], d["vmean"][:, 0], px, py)
    h = r["history"]
    assert h[4:8].tolist() == [1, 1, 0, 1] and float(h[2]) == 0 and float(h[10]) == 0          # landmark 2: no valid row anywhere
    assert torch.isposinf(h[12]) and torch.isfinite(h[[0, 1, 3, 8, 9, 11]]).all()
