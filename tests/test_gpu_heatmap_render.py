"""-m gpu: eg_heatmap_render (csrc/heatmap_render.hip) through ops.heatmap_render and the landmark evaluator's get_softmaxed_heatmap /
get_overlays / get_heatmaps, against the restatement of tests/heatmap_render_reference.py.

Shapes: the smallest at which each mechanism can fail -- side 1 (a single pixel), 2 (fewer pixels than one packed group of 4), 3 and 5
(odd: 27 / 75 bytes per frame, so frames after the first start misaligned and take the byte stores), 33 (1089 rows: two chunks of the
stats kernel and a one-pixel tail), 64 (4096 rows, four workgroups per frame) -- each with count in {1, 3}, first in {0, 2} of a batch
of 5, level_start in {0, 21}, 0 and 4 rows behind the level and an image stride of side^2 and 4 side^2 (8 combinations in which every
pair of values occurs), every output alone and all together; and F = 224 with the real 224 / 7 rows at batch 2 through the evaluator.

Comparisons: `base` and `gt` involve no transcendental and equal the float32 restatement byte for byte; `heat` meets
coord_reference.Report's rule against float64 with the softmax weight's scale p (1 + |x - M| / 16); a `pred` byte equals the float64
byte unless a candidate 255 col e_c lies within its tolerance of an integer in 1..255 -- then it may differ by exactly 1 (an excused
byte), and at most 1 % of a case's bytes may be excused; the case of exact values allows none.

On an MI355X (every test prints its own table; the file takes 4 s): worst |kernel - fp64| / tolerance of `heat` 0.076 over the 48 cases,
0.037 on the exact values, 5e-5 at F = 224; no pred byte differs from the float64 byte in any case (0 excused)."""
import numpy as np
import pytest
import torch

import heatmap_render_reference as R
from gpu_util import DEV
from echoglad_amd import evaluators, ops

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def dev(a):
    return None if a is None else torch.as_tensor(a).to(DEV)


def _check_images(rep, got, r64, r32, exact=False):
    """Every output in `got` against the restatement -> (excused, compared) bytes of the pred image."""
    if "heat" in got:
        assert got["heat"].dtype == F32 and got["heat"].shape == r64["heat"].shape
        rep.check("heat", got["heat"], r64["heat"], r32["heat"], R.heat_scale(r64))
        assert torch.isfinite(got["heat"]).all()
    for name in ("base", "gt"):
        if name in got:
            assert got[name].dtype == torch.uint8 and torch.equal(got[name].cpu(), r32[name]), name
    excused, total = 0, 0
    if "pred" in got:
        assert got["pred"].dtype == torch.uint8
        bad, excused, total = R.pred_bytes_rule(got["pred"], r64, r32)
        print(f"    pred bytes: {bad} outside the rule, {excused} excused of {total}")
        assert bad == 0 and excused <= R.CAP * total, (bad, excused, total)
        if exact:
            assert excused == 0 and torch.equal(got["pred"].cpu(), r64["pred"])
    return excused, total


def _finish(rep, title, capsys):
    with capsys.disabled():
        print(rep.table(title))
    assert not rep.failed(), rep.failed()


@pytest.mark.parametrize("key", R.CASES, ids=lambda k: "side{}-count{}-first{}-start{}-behind{}-ch{}".format(*k))
def test_render_against_the_restatement(key, capsys):
    side, count, first, start, behind, channels = key
    c = R.case(*key)
    lg, lb, img = dev(c["logits"]), dev(c["labels"]), dev(c["image"])
    rep = R.Report()
    with capsys.disabled():
        print(f"\n  {key}: {R.WHAT[side]}")
        every = ops.heatmap_render(lg, R.BATCH, c["level"], first, count, labels=lb, image=img)
        assert set(every) == set(ops.HEATMAP_RENDER_OUTPUTS)
        _check_images(rep, every, c["r64"], c["r32"])
    # every output alone (the others NULL): the same bits; and a second run of all of them: bit-identical
    for want in R.OUTPUT_SETS[:-1]:
        one = ops.heatmap_render(lg, R.BATCH, c["level"], first, count, labels=lb, image=img, want=want)
        assert list(one) == list(want) and torch.equal(one[want[0]], every[want[0]]), want
    again = ops.heatmap_render(lg, R.BATCH, c["level"], first, count, labels=lb, image=img)
    assert all(torch.equal(again[k], every[k]) for k in every)
    # without an image the frame is black: the base is 0, the labels' overlay is the restatement's on a black frame
    black = ops.heatmap_render(lg, R.BATCH, c["level"], first, count, labels=lb, want=("gt", "base"))
    r_black = R.render(c["logits"][c["sl"]], count, c["n_rows"], start, side, c["labels"][c["sl"]], None, dtype=F32)
    assert not black["base"].any() and torch.equal(black["gt"].cpu(), r_black["gt"])
    _finish(rep, f"render side {side}", capsys)


def test_exact_values_allow_no_excused_byte(capsys):
    c = R.exact_case()
    rep = R.Report()
    with capsys.disabled():
        got = ops.heatmap_render(dev(c["logits"]), c["count"], c["level"], 0, c["count"], labels=dev(c["labels"]), image=dev(c["image"]))
        _check_images(rep, got, c["r64"], c["r32"], exact=True)
    assert torch.equal(got["gt"].cpu(), c["r64"]["gt"]) and torch.equal(got["base"].cpu(), c["r64"]["base"])
    _finish(rep, "exact values", capsys)


def _evaluator(c, max_updates, coord=False):
    return evaluators.LandmarkExpectedCoordiantesEvaluator(None, c["batch"], c["level"][1], coord, max_updates=max_updates)


def test_full_size_through_the_evaluator(capsys):
    """F = 224, the real 224 / 7 row layout, batch 2: get_softmaxed_heatmap and get_overlays, host mode and device-history mode."""
    c = R.full_case()
    B, F = c["batch"], c["level"][1]
    lg, lb, img = dev(c["logits"]), dev(c["labels"]), dev(c["image"])
    host, device = _evaluator(c, None), _evaluator(c, 4)
    rep = R.Report()
    heat = host.get_softmaxed_heatmap(lg.view(B, -1, 4))
    assert heat.is_cuda and heat.shape == (B, F, F, 4) and torch.equal(heat, device.get_softmaxed_heatmap(lg))
    over = host.get_overlays(img, lg, lb, 0, B)
    assert set(over) == {"pred_img", "gt_img", "coord_img"} and all(v.is_cuda and v.shape == (B, F, F, 3) for v in over.values())
    with capsys.disabled():
        print("\n  F = 224, batch 2, through the evaluator")
        _check_images(rep, {"heat": heat, "pred": over["pred_img"], "gt": over["gt_img"], "base": over["coord_img"]}, c["r64"], c["r32"])
    # the softmax sums to 1 per (frame, channel) within the rule (the kernel's values added in float64)
    s64, s32 = c["r64"]["heat"].sum(dim=(1, 2)), c["r32"]["heat"].sum(dim=(1, 2))
    rep.check("sum over (h, w)", heat.cpu().to(F64).sum(dim=(1, 2)), s64, s32, R.heat_scale(c["r64"]).sum(dim=(1, 2)))
    assert (s64 - 1).abs().max() < 1e-12
    # coord_img is the base image; a later frame alone is that frame of the batch; both modes give identical images; so do two runs
    base = ops.heatmap_render(lg, B, c["level"], 0, B, image=img, want=("base",))["base"]
    assert torch.equal(over["coord_img"], base)
    second = host.get_overlays(img, lg, lb, first=1)
    other = device.get_overlays(img, lg, lb, 0, B)
    for k in over:
        assert second[k].shape == (1, F, F, 3) and torch.equal(second[k][0], over[k][1]), k
        assert torch.equal(other[k], over[k]), k
    again = host.get_overlays(img, lg, lb, 0, B)
    assert all(torch.equal(again[k], over[k]) for k in over) and torch.equal(host.get_softmaxed_heatmap(lg), heat)
    _finish(rep, "F = 224 through the evaluator", capsys)


@pytest.mark.parametrize("coord", [False, True], ids=["heatmap", "coord_graph"])
@pytest.mark.parametrize("max_updates", [None, 3], ids=["host", "device"])
def test_get_heatmaps_figure(coord, max_updates):
    """The figure of frame 0: 2 panels, 3 with use_coord_graph; the titles are formatted from get_predictions()."""
    pytest.importorskip("matplotlib")
    import matplotlib.pyplot as plt
    B, side = 2, 33
    c = R.case(side, 3, 0, 21, 4, 4)
    rows = slice(0, B * c["n_rows"])
    lg, lb, img = dev(c["logits"][rows]), dev(c["labels"][rows]), dev(c["image"][:B])
    valid = torch.ones_like(lg)
    px, py = dev(np.array([0.5, 0.25], np.float32)), dev(np.array([0.75, 1.5], np.float32))
    rs = np.random.RandomState(3)
    cp, cy = dev(rs.uniform(0, side - 1, (B * 4, 2)).astype(np.float32)), dev(np.floor(rs.uniform(0, side, (B * 4, 2))).astype(np.float32))
    ev = evaluators.LandmarkExpectedCoordiantesEvaluator(None, B, side, coord, max_updates=max_updates)
    if coord:
        ev.update(cp, cy, px, py, valid)
    else:
        ev.update(lg, lb, px, py, valid)
    fig = ev.get_heatmaps(img, lg, lb, cp if coord else None, px, py)
    try:
        groups = ("pred", "coord", "gt") if coord else ("pred", "gt")
        assert len(fig.axes) == len(groups)
        rec = ev.get_predictions()
        shown = ev.get_overlays(img, lg, lb)
        for ax, g in zip(fig.axes, groups):
            if g == "coord":                                     # the reference's own widths of the coordinate predictions: (h, w) order
                q, x0, y0 = cp.cpu()[:4], float(px[0]), float(py[0])
                three = [float(evaluators.pixel_length(q[i, 0], q[i, 1], q[j, 0], q[j, 1], x0, y0)) for i, j in ((3, 0), (0, 1), (1, 2))]
            else:
                three = [float(rec["widths"][f"{g}_{k}_mm"][0]) for k in ("ivs", "lvid", "lvpw")]
            want = "{}: [{:.1f}, {:.1f}, {:.1f}]".format(g, *three)
            assert ax.get_title() == want, (ax.get_title(), want)
            assert len(ax.images) == 1 and np.array_equal(np.asarray(ax.images[0].get_array()), shown[g + "_img"][0].cpu().numpy())
            assert len(ax.lines) == 4 + 3                        # a marker per landmark, two blue segments and the red one
        w = {k: v[0] for k, v in rec["widths"].items()}
        mae, mpe = ev.calculate_width_MAE(w), ev.calculate_width_MPE(w)
        assert fig._suptitle.get_text() == ("MAE [mm] | IVS: {:.1f} | LVID: {:.1f} | LVPW: {:.1f}\nMPE [%] | IVS: {:.1f} | LVID: {:.1f} | LVPW: {:.1f}"
                                            .format(*(float(v) for v in mae + mpe)))
    finally:
        plt.close(fig)
