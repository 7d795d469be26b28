"""CPU: the host side of the heat-map renderer -- the ABI of eg_heatmap_render (csrc/heatmap_render.hip), its refusals before any
launch, the binding's refusals, the evaluator methods' refusals of host tensors, and engine.prediction_table.  No GPU needed."""
import ctypes as ct
import re

import pytest
import torch

from echoglad_amd import _lib, engine, evaluators, ops

DECL = """
int eg_heatmap_render(const float* logits, const float* labels, const float* image, int64_t image_stride,
 const float* stats, int count, int64_t n_rows, int level_start, int side,
 float* heat, uint8_t* pred_rgb, uint8_t* gt_rgb, uint8_t* base_rgb, eg_stream_t stream);
"""
NAME = "eg_heatmap_render"


def _flat(text):
    return re.sub(r"\s+", " ", text).strip()


def test_header_and_binding_declare_abi_156():
    text = open(_lib.HEADER_PATH).read()
    header = _flat(re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    want = _lib.parse_header(DECL)
    assert list(want) == [NAME] and _flat(DECL) in header
    res, args, takes_stream = want[NAME]
    assert _lib.SIGNATURES[NAME] == (res, args) and takes_stream and NAME in _lib.TAKES_STREAM
    assert len(args) == 14 and args[10] is ct.c_void_p and args[3] is ct.c_int64 and args[5] is ct.c_int
    assert _lib.ABI_VERSION >= 156 and f"#define EG_ABI_VERSION {_lib.ABI_VERSION}" in text
    assert re.search(r"\* 156: eg_heatmap_render", _flat(text))                            # the ABI history line
    assert "156: eg_heatmap_render" in open(_lib.__file__).read()
    assert "SATURATES" in text and "heatmap_render" in ops.__dict__ and "HEATMAP_RENDER_OUTPUTS" in ops.__dict__


def test_library_exports_every_declared_symbol(built_lib):
    lib = _lib.load()
    assert lib.eg_version() == _lib.ABI_VERSION >= 156
    assert _lib.check_exports() == [] and hasattr(lib, NAME)


def test_bad_arguments_return_eg_err_arg_with_nothing_launched(built_lib):
    """NULL stream, pointers that are never dereferenced: every call below is refused before the launch (without a GPU a launch would
    come back as EG_ERR_HIP, so EG_ERR_ARG shows that the check came first)."""
    lib = _lib.load()
    mem = (ct.c_float * 256)()
    base = ct.addressof(mem) // 16 * 16 + 16
    p = [ct.c_void_p(base + 64 * i) for i in range(9)]
    odd = lambda q: ct.c_void_p(q.value + 4)

    def render(logits=p[0], labels=p[1], image=p[2], stride=4, stats=p[3], count=1, n_rows=6, start=2, side=2, heat=p[4], pred=p[5],
               gt=p[6], base=p[7]):
        return lib.eg_heatmap_render(logits, labels, image, stride, stats, count, n_rows, start, side, heat, pred, gt, base, None)

    rows = [(dict(logits=None), "NULL"), (dict(stats=None), "NULL"),
            (dict(heat=None, pred=None, gt=None, base=None), "no output"),
            (dict(labels=None), "gt_rgb needs labels"), (dict(labels=None, heat=None, pred=None, base=None), "gt_rgb needs labels"),
            (dict(logits=odd(p[0])), "16-byte"), (dict(labels=odd(p[1])), "16-byte"), (dict(heat=odd(p[4])), "16-byte"),
            (dict(labels=odd(p[1]), gt=None), "16-byte"),
            (dict(count=0), ">= 1"), (dict(count=-2), ">= 1"), (dict(side=0), ">= 1"), (dict(side=-3), ">= 1"), (dict(start=-1), ">= 1"),
            (dict(start=3), "outside the frame's rows"), (dict(side=3), "outside the frame's rows"), (dict(n_rows=5), "outside the frame's rows"),
            (dict(side=46341, n_rows=1 << 40, stride=1 << 40), "exceeds int32"), (dict(start=2147483647, n_rows=1 << 31), "outside the frame's rows"),
            (dict(stride=3), "image_stride"), (dict(stride=-4), "image_stride"),
            (dict(count=1 << 20, n_rows=1 << 12), "exceeds int32")]
    for kw, words in rows:
        assert render(**kw) == _lib.EG_ERR_ARG, kw
        assert words in _lib.last_error(), (kw, _lib.last_error())
    # what is optional passes the checks: the launch is what fails without a device
    if not torch.cuda.is_available():
        for kw in (dict(), dict(labels=None, gt=None), dict(image=None, stride=0), dict(heat=None, pred=None, gt=None),
                   dict(pred=odd(p[5]), gt=odd(p[6]), base=odd(p[7]))):
            assert render(**kw) == _lib.EG_ERR_HIP, kw


def test_binding_and_evaluator_refuse_host_tensors():
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.heatmap_render(torch.zeros(8, 4), 2, (0, 2))
    ev = evaluators.LandmarkExpectedCoordiantesEvaluator(None, 2, 2, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.get_softmaxed_heatmap(torch.zeros(2, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.get_overlays(torch.zeros(2, 1, 2, 2), torch.zeros(8, 4), torch.zeros(8, 4))
    assert not hasattr(ev, "create_overlay_image") and "create_overlay_image" in ev.get_overlays.__doc__
    assert ev.heatmap_panel_title("gt", {"gt_ivs_mm": torch.tensor(1.26), "gt_lvid_mm": 20.0, "gt_lvpw_mm": 3.04}) == "gt: [1.3, 20.0, 3.0]"


COLUMNS = ["pix2mm_x", "pix2mm_y", "pred_ivs", "pred_lvid_top", "pred_lvid_bot", "pred_lvpw", "gt_ivs", "gt_lvid_top", "gt_lvid_bot",
           "gt_lvpw", "pred_ivs_mm", "pred_lvid_mm", "pred_lvpw_mm", "gt_ivs_mm", "gt_lvid_mm", "gt_lvpw_mm"]


def test_prediction_table_columns_and_order():
    """engine.py:602-639: pix2mm first, then the coordinates, then the widths, each in get_predictions()'s order -- a hand-made one."""
    B = 3
    coords = {k: torch.arange(2 * B, dtype=torch.float32).reshape(B, 2) + i for i, k in enumerate(COLUMNS[2:10])}
    widths = {k: torch.arange(B, dtype=torch.float32) * 0.5 + i for i, k in enumerate(COLUMNS[10:])}

    class Hand:
        def get_predictions(self):
            return {"widths": widths, "coordinates": coords}                     # (the table orders the groups, not the dictionary)
    t = engine.prediction_table({"landmarkcoorderror": Hand()}, torch.tensor([0.5, 0.25, 0.125]), [0.75, 1.0, 2.0])
    assert list(t) == COLUMNS and all(isinstance(v, list) and len(v) == B for v in t.values())
    assert t["pix2mm_x"] == [0.5, 0.25, 0.125] and t["pix2mm_y"] == [0.75, 1.0, 2.0]
    assert t["gt_ivs"] == [[4.0, 5.0], [6.0, 7.0], [8.0, 9.0]] and t["pred_lvid_mm"] == [1.0, 1.5, 2.0]
    # the evaluator's own record has those columns in that order (host mode, after a hand-made detailed_performance)
    ev = evaluators.LandmarkExpectedCoordiantesEvaluator(None, B, 4, False)
    preds, gt = torch.rand(B, 4, 2) * 3, torch.floor(torch.rand(B, 4, 2) * 4)
    px, py = torch.full((B,), 0.5), torch.full((B,), 0.25)
    ev.detailed_performance = {"widths": ev.calculate_widths(preds, gt, px, py),
                               "coordinates": {f"{tag}_{k}": c[:, i] for tag, c in (("pred", preds), ("gt", gt))
                                               for k, i in (("ivs", 3), ("lvid_top", 0), ("lvid_bot", 1), ("lvpw", 2))}}
    assert list(engine.prediction_table({"landmarkcoorderror": ev}, px, py)) == COLUMNS
    with pytest.raises(RuntimeError, match="last update"):
        engine.prediction_table({"landmarkcoorderror": evaluators.LandmarkExpectedCoordiantesEvaluator(None, B, 4, False)}, px, py)
