"""-m gpu: the heat-map pass, its backward, both weighted BCEs, the fused criteria node and the evaluator record (csrc/heatmap.hip)
against the fp64 reference of tests/heatmap_reference.py at the sizes and values where these kernels take another path: more than 64
chunks per level, exact ties across every merge boundary, chunk maxima 60 to 120 apart and a chunk of -inf, the eights / 8 x 128 /
2,048-workgroup / 256-frame loop boundaries, and the values the arithmetic treats specially.  Every floating-point comparison goes
through coord_reference.Report.check (tolerance = FACTOR x the float32 reference's own error + 8 ulp x scale; the scales are
explained in heatmap_reference.py); integer outputs are compared exactly, documented bit-reproducibility bit for bit.

Worst |kernel - fp64| / tolerance per group on an MI355X (every test prints its own table; the file takes 7 s): level geometry 0.06,
config 5 through the public classes 0.04, ties 0.04, range 0.02, criteria 0.16 (d total / d logits), stand-alone BCE 0.12 (d loss / d x
on logits), record 0.15.  Each of these one-line changes to heatmap.hip fails tests here: `oi < bidx` -> `oi > bidx` in hm_final_wave
(ties in the logits), no tie merge in its lane loop (ties in the labels, chunks k / k + 64: the later chunk brings the smaller w; its
h alone can never matter, rows ascend with the chunks), f = 1 for exp(q[0] - M) (30 tests), no remainder loop over the batch in
criteria_final_body (every batch that is no multiple of 8), `i += stride` in k_bce_partial (n = 4,095 and 6,292,659 and the criteria's
rows-outside-the-levels route), a single round in lm_record_body (batch 257 and 600)."""
import numpy as np
import pytest
import torch

import heatmap_reference as H
from gpu_util import DEV
from echoglad_amd import evaluators, losses, ops

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def dev(a):
    return None if a is None else torch.as_tensor(a).to(DEV)


def _finish(rep, title, capsys):
    with capsys.disabled():
        print(rep.table(title))
    assert not rep.failed(), rep.failed()


def _check_forward(rep, r, d64, d32, levels, labels=True):
    """Every output of ops.heatmap_expect_fwd: expect by the rule, arg max and label coordinates exactly, vmean by the rule."""
    rep.check("expect", r["expect"], d64["expect"].detach(), d32["expect"].detach(), H.expect_scale(d64, levels))
    assert torch.equal(r["argmax"].cpu(), d64["argmax"]), "arg max"
    if labels:
        assert torch.equal(r["gt"].cpu(), d64["gt"].to(F32)), "label coordinates"
        rep.check("vmean", r["vmean"], d64["vmean"], d32["vmean"], d64["vmean"].abs())


def _check_backward(rep, x, r, B, levels, n_rows, seed=77):
    """ops.heatmap_expect_bwd under a random upstream gradient; rows in no level get exactly zero."""
    g = np.random.RandomState(seed).standard_normal((B, len(levels), 4, 2)).astype(np.float32)
    got = ops.heatmap_expect_bwd(dev(x), r["expect"], r["stats"], dev(g), B, levels)
    _, g64, scale = H.expect_backward(x, B, levels, g)
    _, g32, _ = H.expect_backward(x, B, levels, g, dtype=F32)
    rep.check("d logits", got, g64, g32, scale)
    covered = torch.zeros(n_rows, dtype=torch.bool)
    for s, side in levels:
        covered[s:s + side * side] = True
    assert got.cpu().view(B, n_rows, 4)[:, ~covered, :].eq(0).all(), "rows in no level"
    return g, got


# ---------------------------------------------------------------------------
# level geometry
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(H.GEOMETRY) + ["cfg5"])
def test_level_geometry_forward_and_backward_against_fp64(name, capsys):
    levels, n_rows, B = H.geometry_case(name)
    x, y, v = H.random_inputs(B, n_rows, seed=len(name) + n_rows % 91)
    r = ops.heatmap_expect_fwd(dev(x), B, levels, dev(y), dev(v), want_argmax=True)
    d64, d32 = H.decode(x, B, levels, y, v), H.decode(x, B, levels, y, v, dtype=F32)
    rep = H.Report()
    _check_forward(rep, r, d64, d32, levels)
    g, got = _check_backward(rep, x, r, B, levels, n_rows)
    # the autograd wrapper runs the same two entry points: the same bits
    xt = dev(x).requires_grad_(True)
    e, gt, vm = ops.heatmap_expect(xt, B, tuple(levels), dev(y), dev(v))
    e.backward(dev(g))
    assert torch.equal(e.detach(), r["expect"]) and torch.equal(gt, r["gt"]) and torch.equal(vm, r["vmean"]) and torch.equal(xt.grad, got)
    _finish(rep, f"level geometry {name}", capsys)


def test_config5_table_through_the_public_classes_against_fp64(capsys):
    """BASELINE config 5 (448 x 448, 8 aux levels: 196 + 64 + ... chunks) through ExpectedLandmarkMSE, WeightedBCEWithLogitsLoss,
    decode_landmarks and one device-mode LandmarkExpectedCoordiantesEvaluator.update."""
    levels, n_rows, B = H.geometry_case("cfg5")
    F, W_ELM, OW = 448, 10.0, 9000.0
    x, y, v = H.random_inputs(B, n_rows, seed=448)
    for c in range(4):
        y[n_rows - 1000 - 37 * c, c] = 1.0                     # exact ones (the weight's `== 1`), four different label positions
    rep = H.Report()
    r64 = H.criteria(x, y, v, B, levels, OW, 1.0, W_ELM)
    r32 = H.criteria(x, y, v, B, levels, OW, 1.0, W_ELM, dtype=F32)
    xd, yd, vd = dev(x), dev(y), dev(v)

    def grads(r):
        ge, = torch.autograd.grad(r["elm"], r["x"], retain_graph=True)
        gb, = torch.autograd.grad(r["bce"], r["x"], retain_graph=True)
        return ge.reshape(-1, 4), gb.reshape(-1, 4)
    (ge64, gb64), (ge32, gb32) = grads(r64), grads(r32)
    xt = xd.clone().requires_grad_(True)
    elm = losses.ExpectedLandmarkMSE(W_ELM, B, F, 8).compute(xt.view(B, n_rows, 4), yd.view(B, n_rows, 4), vd)
    g, = torch.autograd.grad(elm, xt)
    rep.check("ExpectedLandmarkMSE", elm.detach().reshape(()), r64["elm"].detach(), r32["elm"].detach(), r64["s_elm"])
    rep.check("d ELM / d logits", g, ge64, ge32, r64["gs_elm"])
    xt = xd.clone().requires_grad_(True)
    bce = losses.WeightedBCEWithLogitsLoss("none", OW, 1).compute(xt.view(B, n_rows, 4), yd.view(B, n_rows, 4), vd)
    g, = torch.autograd.grad(bce, xt)
    rep.check("WeightedBCEWithLogits", bce.detach().reshape(()), r64["bce"].detach(), r32["bce"].detach(), r64["s_bce"])
    rep.check("d BCE / d logits", g, gb64, gb32, r64["gs_bce"])
    # decode of the main grid and the evaluator's record
    main = [levels[-1]]
    d64, d32 = H.decode(x, B, main, y, v), H.decode(x, B, main, y, v, dtype=F32)
    dl = evaluators.decode_landmarks(xd, B, F, yd, vd)
    _check_forward(rep, {k: (None if t is None else t.unsqueeze(1)) for k, t in dl.items()}, d64, d32, main)
    px, py = np.array([0.31], np.float32), np.array([0.47], np.float32)
    ev = evaluators.LandmarkExpectedCoordiantesEvaluator(None, B, F, False, max_updates=2)
    ev.update(xd, yd, torch.from_numpy(px), torch.from_numpy(py), vd)
    last = ev.get_last()
    keys = ("lvid_top", "lvid_bot", "lvpw", "ivs", "ivs_w", "lvid_w", "lvpw_w", "ivs_mpe", "lvid_mpe", "lvpw_mpe")
    idx = [0, 1, 2, 3, 8, 9, 10, 11, 12, 13]
    rec64 = H.record(d64["expect"][:, 0], d64["gt"][:, 0], d64["vmean"][:, 0], px, py)
    rec32 = H.record(d32["expect"][:, 0], d32["gt"][:, 0], d32["vmean"][:, 0], px, py, dtype=F32)
    assert torch.isfinite(rec64["history"]).all()
    rep.check("evaluator record", torch.tensor([float(last[k]) for k in keys], dtype=F64), rec64["history"][idx], rec32["history"][idx],
              rec64["history_scale"][idx])
    assert [ev.valid_errors[k][0] for k in evaluators.NAMES] == [bool(f) for f in rec64["history"][4:8]]
    _finish(rep, "config 5 (448, 8 aux levels) through the public classes", capsys)


# ---------------------------------------------------------------------------
# exact ties across every merge boundary
# ---------------------------------------------------------------------------
TIE_CASES = [(lv, ks) for lv, side in H.TIE_LEVELS.items() for ks in H.tie_sets(side)]


@pytest.mark.parametrize("what", ["logits", "labels"])
@pytest.mark.parametrize("level,kinds", TIE_CASES)
def test_exact_ties_across_every_merge_boundary(level, kinds, what, capsys):
    levels, n_rows, B, x, y, v, li, frame, expected = H.tie_case(level, kinds, what)
    side = levels[li][1]
    r = ops.heatmap_expect_fwd(dev(x), B, levels, dev(y), dev(v), want_argmax=True)
    am, gt, ex = r["argmax"].cpu(), r["gt"].cpu(), r["expect"].cpu()
    for c, kind in enumerate(kinds):                           # the placed ties first: by name
        if what == "logits":
            assert int(am[frame, li, c]) == expected[c], (kind, H.TIE_KINDS[kind], int(am[frame, li, c]), expected[c])
            if kind == "all":                                  # every exp is 1, every sum exact: the centre, exactly
                assert ex[frame, li, c].tolist() == [(side - 1) / 2] * 2, (kind, ex[frame, li, c].tolist())
        else:
            assert tuple(int(q) for q in gt[frame, li, c]) == expected[c], (kind, H.TIE_KINDS[kind], gt[frame, li, c].tolist(), expected[c])
    d64, d32 = H.decode(x, B, levels, y, v), H.decode(x, B, levels, y, v, dtype=F32)
    rep = H.Report()
    _check_forward(rep, r, d64, d32, levels)
    if level != "cfg5":
        _check_backward(rep, x, r, B, levels, n_rows)
    dl = evaluators.decode_landmarks(dev(x), B, side, dev(y), dev(v))          # the evaluator's decode of the same main grid
    assert torch.equal(dl["argmax"], r["argmax"][:, li]) and torch.equal(dl["gt"], r["gt"][:, li]) and torch.equal(dl["expect"], r["expect"][:, li])
    _finish(rep, f"ties in the {what}, {level}, channels {kinds}", capsys)


# ---------------------------------------------------------------------------
# dynamic range across the chunks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", H.RANGE_KINDS)
@pytest.mark.parametrize("level", list(H.RANGE_LEVELS))
def test_dynamic_range_across_chunks_against_fp64(level, kind, capsys):
    """kind "neginf": a whole chunk of -inf next to finite chunks has the finite fp64 answer with zero mass (torch.softmax's), and a
    zero gradient on those rows -- decode and heat-map backward only, no BCE (whose value at -inf is infinite)."""
    levels, n_rows, B, x, rows = H.range_case(level, kind)
    r = ops.heatmap_expect_fwd(dev(x), B, levels, want_argmax=True)
    d64, d32 = H.decode(x, B, levels), H.decode(x, B, levels, dtype=F32)
    rep = H.Report()
    assert torch.isfinite(r["expect"]).all(), r["expect"].cpu()
    _check_forward(rep, r, d64, d32, levels, labels=False)
    _, got = _check_backward(rep, x, r, B, levels, n_rows)
    if kind == "neginf":
        got = got.cpu().view(B, n_rows, 4)
        assert torch.isfinite(got).all() and all(got[:, rows[c], c].eq(0).all() for c in range(4))
    _finish(rep, f"range {kind}, {level}", capsys)


# ---------------------------------------------------------------------------
# the criteria node
# ---------------------------------------------------------------------------
W_BCE, W_ELM, W_COORD = 1.5, 10.0, 0.5


@pytest.mark.parametrize("k,B,form,valid_form,ow,gaps", [(k,) + c for k, c in enumerate(H.criteria_cases())])
def test_criteria_node_against_fp64(k, B, form, valid_form, ow, gaps, capsys):
    levels, n_rows, x, y, v, cp, cy = H.criteria_case(B, form, valid_form, gaps)
    probs, l1 = form[0] == "probs", form[1] == "mae"
    inv_side = dev(np.array([1.0 / s for _, s in levels], np.float32))
    xt, ct = dev(x).requires_grad_(True), dev(cp).requires_grad_(True)
    total, vb, ve, vc = ops.landmark_criteria(xt, dev(y), dev(v), B, tuple(levels), inv_side, ow, W_BCE, W_ELM, ct, dev(cy), W_COORD,
                                              bce_on_probs=probs, coord_l1=l1)
    r64 = H.criteria(x, y, v, B, levels, ow, W_BCE, W_ELM, cp, cy, W_COORD, probs=probs, l1=l1)
    r32 = H.criteria(x, y, v, B, levels, ow, W_BCE, W_ELM, cp, cy, W_COORD, probs=probs, l1=l1, dtype=F32)
    rep = H.Report()
    for name, got, s in (("total", total, "s_total"), ("bce", vb, "s_bce"), ("elm", ve, "s_elm"), ("coord", vc, "s_coord")):
        rep.check(name, got.detach().reshape(()), r64[name].detach(), r32[name].detach(), r64[s])
    # .backward() of the total, and of one component alone
    gx, gc = torch.autograd.grad(total, [xt, ct], retain_graph=True)
    (gx64, gc64), (gx32, gc32) = (torch.autograd.grad(r["total"], [r["x"], r["c"]], retain_graph=True) for r in (r64, r32))
    rep.check("d total / d logits", gx, gx64.reshape(-1, 4), gx32.reshape(-1, 4), r64["gs_bce"] + r64["gs_elm"])
    rep.check("d total / d coord", gc, gc64, gc32, r64["gs_coord"])
    one, which, scale = (ve, "elm", "gs_elm") if k % 2 == 0 else (vb, "bce", "gs_bce")
    g1, = torch.autograd.grad(one, xt, retain_graph=True)
    g64, g32 = (torch.autograd.grad(r[which], r["x"], retain_graph=True)[0].reshape(-1, 4) for r in (r64, r32))
    rep.check(f"d {which} / d logits", g1, g64, g32, r64[scale])
    g1, = torch.autograd.grad(vc, ct)
    rep.check("d coord / d coord", g1, gc64, gc32, r64["gs_coord"])
    if valid_form == "channel2_invalid":
        # nv == 0 -> 1: the slot adds nothing to any loss and its gradient rows are exactly zero
        assert gx.view(B, n_rows, 4)[:, :, 2].eq(0).all() and gx64.reshape(B, n_rows, 4)[:, :, 2].eq(0).all()
    if l1:
        assert gc[1].eq(0).all()                               # sign(0) = 0
    _finish(rep, f"criteria B {B} {form[0]} + {form[1]}, valid {valid_form}, ones_weight {ow:g}{', rows outside the levels' if gaps else ''}",
            capsys)


# ---------------------------------------------------------------------------
# the stand-alone BCE
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("probs", [False, True], ids=["logits", "probs"])
@pytest.mark.parametrize("n", H.BCE_SIZES)
def test_stand_alone_bce_against_fp64_and_reproducible(n, probs, capsys):
    x, y, v = H.bce_case(n, probs)
    OW = 9000.0
    fn = ops.bce_probs if probs else ops.bce_logits
    runs = []
    for _ in range(2):
        xt = dev(x).requires_grad_(True)
        loss = fn(xt, dev(y), dev(v), OW)
        g, = torch.autograd.grad(loss, xt)
        runs.append((loss.detach().cpu(), g.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])      # the same bits on every run
    res = []
    for dtype in (F64, F32):
        xr = H.t(x, dtype).requires_grad_(True)
        loss, scale, gscale = H.bce(xr, y, v, OW, probs, dtype)
        g, = torch.autograd.grad(loss, xr)
        res.append((loss.detach(), g, scale, gscale))
    rep = H.Report()
    rep.check("loss", runs[0][0].reshape(()), res[0][0], res[1][0], res[0][2])
    rep.check("d loss / d x", runs[0][1], res[0][1], res[1][1], res[0][3])
    _finish(rep, f"stand-alone BCE on {'probabilities' if probs else 'logits'}, n {n}", capsys)


# ---------------------------------------------------------------------------
# the evaluator record
# ---------------------------------------------------------------------------
SENTINEL = -7.0
IDX = [0, 1, 2, 3, 8, 9, 10, 11, 12, 13]


def _buffers(B, capacity=2):
    """history / detail of `capacity` records inside buffers one record longer, filled with a sentinel."""
    hist = torch.full((capacity + 1, ops.LANDMARK_RECORD_FLOATS), SENTINEL, device=DEV)
    det = torch.full((capacity + 1, B, ops.LANDMARK_DETAIL_FLOATS), SENTINEL, device=DEV)
    return hist, det, torch.zeros(1, dtype=torch.int64, device=DEV)


def _check_record(rep, hist, det, r64, r32):
    ok, ref = H.split_finite(r64["history"])
    zero = torch.zeros_like(ref)
    rep.check("history", torch.where(ok, hist.cpu().to(F64), zero), ref, torch.where(ok, r32["history"].to(F64), zero),
              torch.where(ok, r64["history_scale"], zero))
    assert H.same_nonfinite(hist, r64["history"]), (hist.cpu(), r64["history"])             # inf / NaN as the host arithmetic gives
    assert torch.equal(hist.cpu()[4:8].to(F64), r64["history"][4:8]) and hist.cpu()[14:].eq(0).all()       # flags: exactly
    assert torch.isfinite(r64["detail"]).all()
    rep.check("detail", det, r64["detail"], r32["detail"], r64["detail_scale"])


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))      # (NaN entries compare as their bits)


def _three_updates(update, hist, det, counter, capacity=2):
    """`capacity` updates fill the history (the same bits each), one more writes nothing and still advances the counter."""
    for _ in range(capacity):
        update()
    assert int(counter.item()) == capacity
    assert _same_bits(hist[0], hist[1]) and _same_bits(det[0], det[1])                      # bit-reproducible
    before = (hist.clone(), det.clone())
    update()
    assert int(counter.item()) == capacity + 1
    assert _same_bits(hist, before[0]) and _same_bits(det, before[1])
    assert hist[capacity].eq(SENTINEL).all() and det[capacity].eq(SENTINEL).all()             # nothing past capacity


@pytest.mark.parametrize("B", H.RECORD_BATCHES)
def test_record_from_coordinates_against_fp64(B, capsys):
    pred, gt, px, py = H.record_coord_case(B)
    hist, det, counter = _buffers(B)
    args = (dev(pred.reshape(-1, 2)), dev(gt.reshape(-1, 2)), B, dev(px), dev(py), hist[:2], det[:2], counter)
    _three_updates(lambda: ops.landmark_record_coord(*args), hist, det, counter)
    r64, r32 = H.record(pred, gt, None, px, py), H.record(pred, gt, None, px, py, dtype=F32)
    rep = H.Report()
    _check_record(rep, hist[0], det[0], r64, r32)
    assert torch.equal(det[0, :, :8].cpu(), torch.from_numpy(pred.reshape(B, 8))) and torch.equal(det[0, :, 8:16].cpu(), torch.from_numpy(gt.reshape(B, 8)))
    _finish(rep, f"record from coordinates, batch {B}", capsys)


def test_record_from_heat_maps_against_fp64(capsys):
    B, F = 257, 4
    x, y, v, px, py, n_rows = H.record_hm_case(B, F)
    hist, det, counter = _buffers(B)
    ws = torch.empty(ops.landmark_record_workspace_bytes(B, F), dtype=torch.uint8, device=DEV)
    args = (dev(x), dev(y), dev(v), B, F, dev(px), dev(py), hist[:2], det[:2], counter, ws)
    _three_updates(lambda: ops.landmark_record_hm(*args), hist, det, counter)
    main = [(n_rows - F * F, F)]
    recs = []
    for dtype in (F64, F32):
        d = H.decode(x, B, main, y, v, dtype=dtype)
        recs.append(H.record(d["expect"][:, 0], d["gt"][:, 0], d["vmean"][:, 0], px, py, dtype=dtype))
    rep = H.Report()
    _check_record(rep, hist[0], det[0], *recs)
    assert hist[0].cpu()[4:8].tolist() == [1, 1, 0, 1]                                       # landmark 2: no valid row in any frame
    _finish(rep, f"record from heat maps, frame {F}, batch {B}", capsys)
