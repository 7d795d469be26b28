"""A plain reference of the heat-map losses, the landmark decode and the evaluator record (csrc/heatmap.hip): torch / numpy on the
CPU, float64 by default, no kernels.  The kernels' fp32 inputs are converted to double (exactly), so every tie, every `== 1` and
every `== 0` decision is taken on the kernels' own numbers.  Every function takes ``dtype``: the same code in float32 is "what the
host classes would compute", the yardstick of the tolerance rule (coord_reference.Report, imported, not forked):

    |kernel - fp64| <= FACTOR * max|ref32 - fp64| + 8 * 2^-23 * scale.

The scale of a quantity is the value of its own formula with every subtraction replaced by the sum of the magnitudes (and every
sum taken over magnitudes): the rounding error of fp32 operands and of a sum taken in any order is bounded by a multiple of that
number, and a small result that comes from cancellation (expectation minus label, sigmoid minus label, predicted minus labelled
width) must not tighten the tolerance.  One more factor belongs to every softmax weight p = exp(x - M) / S: the kernels (and torch
in float32) form x - M in fp32, whose rounding error of up to 2^-24 |x - M| becomes a relative error of p, so p's scale is
p * (1 + |x - M| / 16)  (8 ulp * |x - M| / 16 = 2^-24 |x - M|).
Integer outputs (arg max, label coordinates, flags) are compared exactly, never through a tolerance.

The input builders of tests/test_gpu_heatmap_edges.py live here as well; each one ASSERTS the condition it was built for (the two
tied rows fall into the intended thread / wave / chunk / lane, the dim chunk is far enough below the maximum, the fp64 result is
finite), and tests/test_heatmap_reference.py runs every builder of every parametrised case without a GPU."""
import numpy as np
import torch

from coord_reference import FACTOR, ULP, Report          # noqa: F401  (the rule itself: one owner)

F64 = torch.float64
F32 = torch.float32

# the kernels' geometry (csrc/heatmap.hip): what the builders aim at
CHUNK = 1024            # rows of a level per workgroup of k_hm_partial
THREADS = 256           # threads of that workgroup: thread t holds rows t, t + 256, t + 512, t + 768 of its chunk
WAVE = 64               # lanes of a wave; hm_final_wave gives chunk k to lane k & 63
BATCH_UNROLL = 8        # criteria_final_body walks the batch in eights
BCE_UNROLL = 8 * 128    # ... and the BCE partials 8 x 128 at a time once there are more than 896
BCE_BLOCKS = 2048       # grid cap of k_bce_partial
RECORD_ROUND = 256      # frames per round of lm_record_body


def t(a, dtype=F64):
    return torch.as_tensor(a).detach().to(dtype)


def n_rows_of(levels, extra_behind=0):
    return max(s + side * side for s, side in levels) + extra_behind


def n_chunks(side):
    return (side * side + CHUNK - 1) // CHUNK


def place(r):
    """Where row r of a level (counted from the level's first row) is handled: its chunk, the thread / wave / lane of
    k_hm_partial and which of the thread's four rows it is, and the lane of hm_final_wave that owns the chunk."""
    chunk, idx = divmod(int(r), CHUNK)
    thread = idx % THREADS
    return dict(chunk=chunk, slot=idx // THREADS, thread=thread, wave=thread // WAVE, lane=thread % WAVE, final_lane=chunk % WAVE,
                final_round=chunk // WAVE)


# ---------------------------------------------------------------------------
# decode: softmax expectation, first arg max, label coordinates, mean of valid  (criterion.py:93-135, evaluators.py:291-340)
# ---------------------------------------------------------------------------
def label_coords(y_level):
    """[B, S, S, 4] -> int64 [B, 4, 2]: h = the first row whose maximum is the map's maximum, w = the first column whose maximum is
    (criterion.py:118-123) -- taken independently, so with two separated maxima the answer may hold no maximum."""
    y = np.asarray(y_level, dtype=np.float64)
    row_max = y.max(axis=2)                  # [B, S, 4] over w
    col_max = y.max(axis=1)                  # [B, S, 4] over h
    return np.stack([np.argmax(row_max, axis=1), np.argmax(col_max, axis=1)], axis=-1).astype(np.int64)


def decode(logits, batch, levels, labels=None, valid=None, dtype=F64, grad=False):
    """logits / labels / valid [batch * n_rows, 4] -> dict(expect [B,L,4,2] (on the autograd graph of "x" with grad=True), argmax
    [B,L,4] int64 (row inside the level), gt [B,L,4,2] int64, vmean [B,L,4], p = [per level [B, S*S, 4] softmax weights],
    xm = [per level |x - max|])."""
    x = t(logits, dtype).reshape(batch, -1, 4).clone().requires_grad_(grad)
    y = None if labels is None else np.asarray(t(labels, F64)).reshape(batch, -1, 4)
    v = None if valid is None else t(valid, dtype).reshape(batch, -1, 4)
    ex, am, gt, vm, ps, xms = [], [], [], [], [], []
    for start, side in levels:
        n = side * side
        xl = x[:, start:start + n, :]
        p = torch.softmax(xl, dim=1)
        hh = torch.arange(side, dtype=dtype).repeat_interleave(side).view(1, n, 1)
        ww = torch.arange(side, dtype=dtype).repeat(side).view(1, n, 1)
        ex.append(torch.stack(((p * hh).sum(1), (p * ww).sum(1)), dim=-1))                 # [B,4,2]
        am.append(torch.from_numpy(np.argmax(np.asarray(xl.detach().to(F64)), axis=1)))     # first occurrence: numpy's rule
        ps.append(p.detach())
        with torch.no_grad():
            xms.append((xl - xl.max(dim=1, keepdim=True).values).abs())
        if y is not None:
            gt.append(torch.from_numpy(label_coords(y[:, start:start + n, :].reshape(batch, side, side, 4))))
        if v is not None:
            vm.append(v[:, start:start + n, :].mean(dim=1))
    return dict(x=x, expect=torch.stack(ex, 1), argmax=torch.stack(am, 1), gt=torch.stack(gt, 1) if gt else None,
                vmean=torch.stack(vm, 1) if vm else None, p=ps, xm=xms)


def _hw(side, dtype=F64):
    return (torch.arange(side, dtype=dtype).repeat_interleave(side).view(1, -1, 1),
            torch.arange(side, dtype=dtype).repeat(side).view(1, -1, 1))


def expect_grad_scale(d, levels, g_abs, n_rows):
    """The scale of d logits = p ((h - E_h) g_h + (w - E_w) g_w) per element [B * n_rows, 4]: p (1 + |x - M| / 16) ((h + E_h) |g_h| +
    (w + E_w) |g_w|), 0 outside every level and where p is 0.  g_abs [B,L,4,2]: the magnitudes (or the scale) of the upstream gradient."""
    B = d["expect"].shape[0]
    out = torch.zeros(B, n_rows, 4, dtype=F64)
    E = d["expect"].detach().to(F64)
    for l, (start, side) in enumerate(levels):
        hh, ww = _hw(side)
        p, xm = d["p"][l].to(F64), d["xm"][l].to(F64)
        s = (hh + E[:, l, :, 0].unsqueeze(1)) * g_abs[:, l, :, 0].unsqueeze(1) + (ww + E[:, l, :, 1].unsqueeze(1)) * g_abs[:, l, :, 1].unsqueeze(1)
        s = p * (1 + torch.where(p > 0, xm, torch.zeros_like(xm)) / 16) * s
        out[:, start:start + side * side, :] = torch.where(p > 0, s, torch.zeros_like(s))
    return out.reshape(B * n_rows, 4)


def expect_scale(d, levels):
    """The scale of the expectations [B,L,4,2]: sum p (1 + |x - M| / 16) h (every summand is non-negative already)."""
    out = []
    for l, (start, side) in enumerate(levels):
        hh, ww = _hw(side)
        p, xm = d["p"][l].to(F64), d["xm"][l].to(F64)
        q = p * (1 + torch.where(p > 0, xm, torch.zeros_like(xm)) / 16)
        out.append(torch.stack(((q * hh).sum(1), (q * ww).sum(1)), dim=-1))
    return torch.stack(out, 1)


def expect_backward(logits, batch, levels, d_expect, dtype=F64):
    """-> (decode dict, d logits [B * n_rows, 4] by autograd in `dtype`, its per-element scale)."""
    d = decode(logits, batch, levels, dtype=dtype, grad=True)
    g, = torch.autograd.grad(d["expect"], d["x"], t(d_expect, dtype))
    n_rows = d["x"].shape[1]
    return d, g.reshape(-1, 4), expect_grad_scale(d, levels, t(d_expect).abs(), n_rows)


# ---------------------------------------------------------------------------
# the losses
# ---------------------------------------------------------------------------
def elm(d, levels, weight, dtype=F64):
    """ExpectedLandmarkMSE (criterion.py:133-151) over an arbitrary level table, on decode()'s expect / gt / vmean:
    w sum_{l,c,xy} [sum_b ((e - gt) / side)^2 vmean] / nv, nv = sum_b vmean (1 where that is 0) -> (loss, its scale: the same sum
    with ((|e| + |gt|) / side)^2, and G [B,L,4,2]: the scale of d loss / d expect = 2 w (|e| + |gt|) / side^2 vmean / nv)."""
    side = torch.tensor([s for _, s in levels], dtype=dtype).view(1, -1, 1, 1)
    e, gt, vm = d["expect"], d["gt"].to(dtype), d["vmean"].to(dtype).unsqueeze(-1)
    nv = vm.sum(dim=0, keepdim=True)
    nv = torch.where(nv == 0, torch.ones_like(nv), nv)
    loss = weight * ((((e - gt) / side) ** 2) * vm / nv).sum()
    with torch.no_grad():
        mag = (e.detach().abs() + gt.abs()) / side
        scale = float(weight * ((mag ** 2) * vm / nv).sum())
        G = (2 * weight * mag / side * vm / nv).to(F64)
    return loss, scale, G


def bce(x, y, valid, ones_weight, probs, dtype=F64):
    """WeightedBCE / WeightedBCEWithLogitsLoss (criterion.py:6-33): torch's element formula (on probabilities: the logs clamped at
    -100, and autograd's gradient floor 1e-12), x ones_weight where y == 1 and ones_weight > 1, sum(loss valid) / sum(valid).
    x on the autograd graph -> (loss, scale of the loss, scale of d loss / d x per element)."""
    y = t(y, dtype)
    v = torch.ones_like(y) if valid is None else t(valid, dtype).reshape(y.shape)
    fn = torch.nn.functional.binary_cross_entropy if probs else torch.nn.functional.binary_cross_entropy_with_logits
    el = fn(x, y, reduction="none")
    w = torch.where(y == 1, torch.full_like(y, float(ones_weight)), torch.ones_like(y)) if ones_weight > 1 else torch.ones_like(y)
    loss = (w * el * v).sum() / v.sum()
    with torch.no_grad():
        xd = x.detach()
        if probs:
            l1, l0 = torch.log(xd).clamp_min(-100).abs(), torch.log1p(-xd).clamp_min(-100).abs()
            mag = y.abs() * l1 + (1 - y).abs() * l0
            gmag = (xd.abs() + y.abs()) / ((1 - xd) * xd).clamp_min(float(np.float32(1e-12)))      # (torch's floor is the float constant)
        else:
            mag = xd.clamp_min(0) + (xd * y).abs() + torch.log1p(torch.exp(-xd.abs()))
            gmag = torch.sigmoid(xd) + y.abs()
        scale = float((w * mag * v.abs()).sum() / v.sum())
        gscale = (w * gmag * v.abs() / v.sum()).to(F64)
    return loss, scale, gscale


def coord_loss(pred, y, weight, l1, dtype=F64):
    """engine.MSE / engine.MAE on the landmark coordinates: weight * mean((pred - y)^2) or weight * mean|pred - y| -> (loss, scale of
    the loss, scale of its gradient per element); pred on the autograd graph."""
    y = t(y, dtype).reshape(pred.shape)
    d = pred - y
    loss = weight * (d.abs().mean() if l1 else (d ** 2).mean())
    with torch.no_grad():
        mag = pred.detach().abs() + y.abs()
        scale = float(weight * (mag.mean() if l1 else (mag ** 2).mean()))
        gscale = (torch.full_like(mag, weight / mag.numel()) if l1 else 2 * weight * mag / mag.numel()).to(F64)
    return loss, scale, gscale


def criteria(logits, labels, valid, batch, levels, ones_weight, w_bce, w_elm, coord_pred=None, coord_y=None, w_coord=1.0,
             probs=False, l1=False, dtype=F64):
    """The training step's criteria (engine.py:582-600) -> dict(total, bce, elm, coord (on the graph of "x" [B * n_rows, 4] and "c"),
    and the scales "s_total", "s_bce", "s_elm", "s_coord", "gs_bce", "gs_elm" [B * n_rows, 4], "gs_coord")."""
    d = decode(logits, batch, levels, labels, valid, dtype=dtype, grad=True)
    n_rows = d["x"].shape[1]
    v_elm, s_elm, G = elm(d, levels, w_elm, dtype)
    v_bce, s_bce, gs_bce = bce(d["x"].reshape(-1, 4), t(labels, dtype).reshape(-1, 4), valid, ones_weight, probs, dtype)
    v_bce, s_bce, gs_bce = w_bce * v_bce, w_bce * s_bce, w_bce * gs_bce
    out = dict(x=d["x"], d=d, bce=v_bce, elm=v_elm, s_bce=s_bce, s_elm=s_elm, gs_bce=gs_bce,
               gs_elm=expect_grad_scale(d, levels, G, n_rows), c=None, coord=None, s_coord=0.0, gs_coord=None)
    total, s_total = v_bce + v_elm, s_bce + s_elm
    if coord_pred is not None:
        c = t(coord_pred, dtype).clone().requires_grad_(True)
        v_c, s_c, gs_c = coord_loss(c, coord_y, w_coord, l1, dtype)
        out.update(c=c, coord=v_c, s_coord=s_c, gs_coord=gs_c)
        total, s_total = total + v_c, s_total + s_c
    out.update(total=total, s_total=s_total)
    return out


# ---------------------------------------------------------------------------
# the evaluator record  (LandmarkExpectedCoordiantesEvaluator.update, evaluators.py:291-391)
# ---------------------------------------------------------------------------
def _length(x0, y0, x1, y1, px, py, magnitudes=False):
    if magnitudes:
        return torch.sqrt(((x0.abs() + x1.abs()) * px) ** 2 + ((y0.abs() + y1.abs()) * py) ** 2)
    return torch.sqrt(((x0 - x1) * px) ** 2 + ((y0 - y1) * py) ** 2)


def _ordered_sum(terms):
    """sum over dim 0 in ascending order in the terms' own type (the kernel adds the frames in that order in fp32)."""
    s = torch.zeros_like(terms[0])
    for k in range(terms.shape[0]):
        s = s + terms[k]
    return s


def record(pred, gt, vs, px, py, dtype=F64):
    """pred / gt [B,4,2] (h, w), vs [B,4] mean of valid per (frame, landmark) or None (every landmark valid), px / py [B] ->
    dict(history [16]: err[4], flag[4], MAE {ivs, lvid, lvpw}, MPE {ivs, lvid, lvpw}, 0, 0;  detail [B,24]: pred, gt, predicted and
    labelled widths {ivs, lvid, lvpw}, 0, 0;  "history_scale" / "detail_scale": the same with magnitudes).  A landmark without a
    valid row: flag 0, divisor 1; a zero labelled width: MPE inf or NaN as IEEE division gives."""
    p, g = t(pred, dtype).reshape(-1, 4, 2), t(gt, dtype).reshape(-1, 4, 2)
    B = p.shape[0]
    vs = torch.ones(B, 4, dtype=dtype) if vs is None else t(vs, dtype).reshape(B, 4)
    px, py = t(px, dtype).reshape(B), t(py, dtype).reshape(B)
    nv_raw = _ordered_sum(vs)
    nv = torch.where(nv_raw == 0, torch.ones_like(nv_raw), nv_raw)
    res = {}
    for mag in (False, True):
        err = _length(g[:, :, 1], g[:, :, 0], p[:, :, 1], p[:, :, 0], px[:, None], py[:, None], mag) * vs         # [B,4]

        def widths(c):
            return torch.stack([_length(c[:, 3, 1], c[:, 3, 0], c[:, 0, 1], c[:, 0, 0], px, py, mag),
                                _length(c[:, 0, 1], c[:, 0, 0], c[:, 1, 1], c[:, 1, 0], px, py, mag),
                                _length(c[:, 1, 1], c[:, 1, 0], c[:, 2, 1], c[:, 2, 0], px, py, mag)], dim=1)          # [B,3]
        wp, wg = widths(p), widths(g)
        w = torch.stack([vs[:, 3] / nv[3], vs[:, 0] * vs[:, 1] / torch.minimum(nv[0], nv[1]), vs[:, 2] / nv[2]], dim=1)
        dif = (wp + wg) if mag else (wp - wg).abs()
        # (the scale of the MPE divides by the true labelled width, not by its magnitude form)
        wg_true = wg if not mag else res["wg"]
        mae, mpe = dif * w, ((100 * dif) / wg_true) * w
        hist = torch.cat([_ordered_sum(err) / nv, (nv_raw > 0).to(dtype), _ordered_sum(mae), _ordered_sum(mpe), torch.zeros(2, dtype=dtype)])
        det = torch.cat([p.reshape(B, 8), g.reshape(B, 8), wp, wg, torch.zeros(B, 2, dtype=dtype)], dim=1)
        if mag:
            hist[4:8] = 0                                  # flags: exact
            det[:, :16] = det[:, :16].abs()
            res.update(history_scale=hist.to(F64), detail_scale=det.to(F64))
        else:
            res.update(history=hist, detail=det, wg=wg)
    return res


# ---------------------------------------------------------------------------
# input builders: level geometry
# ---------------------------------------------------------------------------
GEOMETRY = {
    "side2": ([(0, 2)], 0, 2),                               # 4 rows: 252 idle threads, three empty waves
    "side32": ([(0, 32)], 0, 2),                             # exactly one full chunk
    "side33": ([(0, 33)], 0, 2),                             # a full chunk + a 65-row tail (wave 1 holds one row, waves 2 and 3 none)
    "stacked": ([(0, 2), (4, 33), (1093, 45)], 0, 2),        # levels that start at rows that are no multiple of anything
    "side256": ([(0, 256)], 0, 2),                           # 64 chunks: one per lane of the final merge
    "side257": ([(0, 257)], 0, 2),                           # 65 chunks: lane 0 takes two, the tail chunk holds 513 rows
    "gaps": ([(3, 5), (33, 33), (1130, 2)], 7, 2),           # rows in no level in front, between and behind
}


def cfg5_levels():
    """BASELINE config 5's table (448 x 448, 8 aux levels) written out: 1 + 1 + 1 + 1 + 1 + 4 + 16 + 64 + 196 chunks."""
    out, start = [], 0
    for s in [2, 4, 8, 16, 32, 64, 128, 256, 448]:
        out.append((start, s))
        start += s * s
    return out


def geometry_case(name):
    """-> (levels, n_rows, batch) and asserts what the case is there for."""
    if name == "cfg5":
        levels, extra, batch = cfg5_levels(), 0, 1
        assert [n_chunks(s) for _, s in levels] == [1, 1, 1, 1, 1, 4, 16, 64, 196]
    else:
        levels, extra, batch = GEOMETRY[name]
    n_rows = n_rows_of(levels, extra)
    sizes = {s: (s * s, n_chunks(s), s * s - (n_chunks(s) - 1) * CHUNK) for _, s in levels}
    if name == "side2":
        assert sizes[2] == (4, 1, 4)
    if name == "side32":
        assert sizes[32] == (1024, 1, 1024)
    if name in ("side33", "stacked", "gaps"):
        assert sizes[33] == (1089, 2, 65) and place(1024 + 64)["wave"] == 1
    if name == "stacked":
        assert sizes[45] == (2025, 2, 1001) and all(s % 4 for s, _ in levels[2:]) and levels[1][0] == 4
    if name == "side256":
        assert sizes[256][1] == WAVE
    if name == "side257":
        assert sizes[257] == (66049, WAVE + 1, 513) and place(66048)["final_lane"] == 0 and place(66048)["final_round"] == 1
    if name == "gaps":
        covered = np.zeros(n_rows, bool)
        for s, side in levels:
            assert not covered[s:s + side * side].any()
            covered[s:s + side * side] = True
        runs = np.flatnonzero(np.diff(np.concatenate([[True], covered, [True]]).astype(int)))
        assert not covered[0] and not covered[-1] and len(runs) == 2 * (len(levels) + 1) and (~covered).sum() >= 4
    return levels, n_rows, batch


def random_inputs(batch, n_rows, seed, sigma=3.0):
    """(logits N(0, sigma), one-hot-ish labels in [0, 1) with one 1.0 per (frame, channel) region, valid 0/1) float32 [B * n_rows, 4]."""
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal((batch * n_rows, 4)) * sigma).astype(np.float32)
    y = (rs.uniform(0, 0.9, (batch * n_rows, 4)) * (rs.uniform(0, 1, (batch * n_rows, 4)) < 0.05)).astype(np.float32)
    v = (rs.uniform(0, 1, (batch * n_rows, 4)) < 0.7).astype(np.float32)
    return x, y, v


# ---------------------------------------------------------------------------
# input builders: exact ties across every merge boundary
# ---------------------------------------------------------------------------
TIE_KINDS = {
    "thread": "the same thread of k_hm_partial (rows r, r + 256)",
    "lanes": "two lanes of one wave",
    "waves": "two waves of one chunk",
    "chunks": "two chunks, two lanes of the final merge",
    "round": "two chunks of ONE lane of the final merge (k, k + 64)",
    "higher": "chunk >= 64 (lane 0, second round) against chunk 1: the earlier row sits in the HIGHER lane",
    "all": "every row equal",
    "separated": "two separated maxima (h1 < h2, w1 > w2): the label coordinate (h1, w2) holds no maximum",
}
_IDX = (3, 70, 131, 200, 259, 300, 515, 700, 1000)


def _tie_condition(kind, a, b):
    if kind == "thread":
        return a["chunk"] == b["chunk"] and a["thread"] == b["thread"] and a["slot"] + 1 == b["slot"]
    if kind == "lanes":
        return a["chunk"] == b["chunk"] and a["wave"] == b["wave"] and a["lane"] != b["lane"] and a["slot"] == b["slot"]
    if kind == "waves":
        return a["chunk"] == b["chunk"] and a["wave"] != b["wave"]
    if kind == "chunks":
        return a["chunk"] != b["chunk"] and a["final_lane"] != b["final_lane"]
    if kind == "round":
        return a["final_lane"] == b["final_lane"] and a["final_round"] + 1 == b["final_round"]
    if kind == "higher":
        return a["chunk"] == 1 and b["chunk"] >= WAVE and b["final_lane"] < a["final_lane"]
    raise KeyError(kind)


def tie_rows(side, kind):
    """(r1 < r2) rows of a level of side `side` that meet TIE_KINDS[kind], preferring a pair with h1 < h2 and w1 > w2 (then the two
    label minima come from different rows); None where the level is too small for the kind.  The condition is asserted."""
    n = side * side
    if kind == "all":
        return None
    if kind == "separated":
        r1, r2 = 1 * side + (side - 2), (side - 2) * side + 1
        assert r1 < r2 < n and r1 // side < r2 // side and r1 % side > r2 % side
        return r1, r2
    chunks1 = {"chunks": (1,), "round": (WAVE, WAVE + 1), "higher": tuple(range(WAVE, min(n_chunks(side), WAVE + 2)))}.get(kind, (0,))
    chunk0 = 1 if kind == "higher" else 0
    best = None
    for c1 in chunks1:
        for i in _IDX:
            for j in _IDX:
                r1, r2 = chunk0 * CHUNK + i, c1 * CHUNK + j
                if not r1 < r2 < n or not _tie_condition(kind, place(r1), place(r2)):
                    continue
                if r1 // side < r2 // side and r1 % side > r2 % side:
                    return r1, r2
                best = best or (r1, r2)
    if best is not None:
        assert _tie_condition(kind, place(best[0]), place(best[1]))
    return best


def tie_sets(side):
    """Lists of four kinds (one per channel) covering every kind the level is large enough for."""
    kinds = [k for k in TIE_KINDS if k in ("all", "separated") or tie_rows(side, k) is not None]
    while len(kinds) % 4:
        kinds.append(kinds[len(kinds) % 3])
    return [tuple(kinds[i:i + 4]) for i in range(0, len(kinds), 4)]


TIE_LEVELS = {"side33": 33, "side257": 257, "cfg5": 448}


def tie_case(level_name, kinds, what, seed=5):
    """what = "logits" | "labels": the named tie of kinds[c] in channel c of the level (for cfg5: of the main grid inside the whole
    table, batch 1; else batch 2, frame 1 holding the ties and frame 0 none).  -> (levels, n_rows, batch, logits, labels, valid,
    level index, frame, expected): expected[c] = the first arg max row (logits) or the (h, w) label coordinate (labels)."""
    side = TIE_LEVELS[level_name]
    levels, n_rows, batch = geometry_case(level_name)
    li = len(levels) - 1
    start = levels[li][0]
    assert levels[li][1] == side
    x, y, v = random_inputs(batch, n_rows, seed)
    frame = batch - 1
    base = frame * n_rows + start
    n = side * side
    expected = []
    for c, kind in enumerate(kinds):
        rows = tie_rows(side, kind)
        arr, top = (x, np.float32(20.0)) if what == "logits" else (y, np.float32(1.0))
        if kind == "all":
            arr[base:base + n, c] = np.float32(0.75) if what == "logits" else np.float32(0.0)      # (labels: an all-zero map)
            expected.append(0 if what == "logits" else (0, 0))
            continue
        assert rows is not None, (level_name, kind)
        r1, r2 = rows
        assert float(arr[base:base + n, c].max()) < float(top)
        arr[base + r1, c] = top
        arr[base + r2, c] = top
        lvl = arr[base:base + n, c]
        assert np.flatnonzero(lvl == lvl.max()).tolist() == [r1, r2]                  # exactly two equal maxima, where intended
        if kind not in ("separated",):
            assert _tie_condition(kind, place(r1), place(r2)), (kind, place(r1), place(r2))
        expected.append(r1 if what == "logits" else (r1 // side, min(r1 % side, r2 % side)))
        if kind == "separated" and what == "labels":
            assert lvl[expected[-1][0] * side + expected[-1][1]] < top              # the answer holds no maximum
        if kind == "round" and what == "labels":
            assert r2 % side < r1 % side                                            # the later chunk brings the smaller w
    return levels, n_rows, batch, x, y, v, li, frame, expected


# ---------------------------------------------------------------------------
# input builders: dynamic range across the chunks
# ---------------------------------------------------------------------------
RANGE_KINDS = ("plus60", "minus80", "minus120", "alternating40", "peak30", "neginf")
RANGE_LEVELS = {"side257": 257, "side45": 45}


def range_case(level_name, kind, seed=9):
    """N(0, 3) logits plus an offset per chunk of a main-only level, batch 2; channel c shifts another chunk (the last channel the
    tail chunk).  -> (levels, n_rows, batch, logits, rows [4] lists of the level rows singled out).  Asserted: what the kind is for."""
    side = RANGE_LEVELS[level_name]
    levels, batch = [(0, side)], 2
    n = side * side
    K = n_chunks(side)
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal((batch, n, 4)) * 3).astype(np.float32)
    chunk_of = np.arange(n) // CHUNK
    picked = []
    for c in range(4):
        k = K - 1 if c == 3 else (c * 23 + 1) % max(K - 1, 1)
        rows = np.flatnonzero(chunk_of == k)
        if kind == "plus60":
            x[:, rows, c] += np.float32(60)
        elif kind == "minus80":
            x[:, rows, c] -= np.float32(80)
        elif kind == "minus120":
            x[:, rows, c] -= np.float32(120)
        elif kind == "alternating40":
            x[:, :, c] += np.where((chunk_of + c) % 2 == 0, np.float32(40), np.float32(-40))[None, :]
        elif kind == "peak30":
            rows = rows[[(17 * (c + 1)) % len(rows)]]
            x[:, rows, c] = np.abs(x[:, rows, c]) + np.float32(30)
        elif kind == "neginf":
            assert len(rows) == CHUNK or k == K - 1                                  # a whole chunk (the tail chunk: all its rows)
            x[:, rows, c] = -np.inf
        picked.append(rows.tolist())
    # what the kind is for, on the fp64 numbers
    xd = x.astype(np.float64)
    for c in range(4):
        rows = np.asarray(picked[c])
        rest = np.setdiff1d(np.arange(n), rows)
        cmax = np.array([xd[:, chunk_of == k, c].max(axis=1) for k in range(K)])          # [K, B]
        M = xd[:, :, c].max(axis=1)                                                       # [B]
        with np.errstate(invalid="ignore"):
            p = np.exp(xd[:, :, c] - M[:, None])
        p /= p.sum(axis=1, keepdims=True)
        assert np.isfinite(p).all()                                                       # the fp64 answer is finite
        if kind == "plus60":
            assert (xd[:, rows, c].min(axis=1) - xd[:, rest, c].max(axis=1) > 20).all() and (p[:, rest].sum(axis=1) < 1e-8).all()
        if kind == "minus80":
            assert (M - xd[:, rows, c].max(axis=1) >= 60).all() and (M - xd[:, rows, c].max(axis=1) <= 104).all()
        if kind == "minus120":
            assert (M - xd[:, rows, c].max(axis=1) >= 104).all()                          # float's exp of the difference is 0
        if kind == "alternating40":
            assert (np.abs(np.diff(cmax, axis=0)) >= 60).all()
        if kind == "peak30":
            assert (p[:, rows[0]] > 0.999).all()
        if kind == "neginf":
            assert np.isneginf(xd[:, rows, c]).all() and np.isfinite(xd[:, rest, c]).all() and (p[:, rows] == 0).all()
    return levels, n, batch, x.reshape(batch * n, 4), picked


# ---------------------------------------------------------------------------
# input builders: the criteria node
# ---------------------------------------------------------------------------
CRIT_LEVELS = [(0, 2), (4, 4), (20, 8), (84, 16)]           # frame 16, 3 aux levels: 340 rows, 4 chunks per frame
CRIT_GAP_LEVELS = [(2, 2), (8, 4), (24, 8), (90, 16)]       # the same levels with rows in no level between them and behind
CRIT_BATCHES = (7, 8, 9, 17, 224, 225)
CRIT_FORMS = (("logits", "mse"), ("probs", "mae"))
VALID_FORMS = ("binary", "fractional", "channel2_invalid")
ONES_WEIGHTS = (0.5, 1.0, 9000.0)
NEAR_ONE = (np.float32(0.999), np.float32(1.0), np.float32(1.0) - np.float32(2.0 ** -24))


def criteria_cases():
    """(batch, form, valid form, ones weight, gaps): every batch with both forms (valid form and weight rotating), batch 9 with every
    valid form x weight, and the table with rows outside every level at batch 9."""
    cases = []
    for i, B in enumerate(CRIT_BATCHES):
        for j, form in enumerate(CRIT_FORMS):
            cases.append((B, form, VALID_FORMS[(i + j) % 3], ONES_WEIGHTS[(i + 2 * j + 2) % 3], False))
    for form in CRIT_FORMS:
        for vf in VALID_FORMS:
            for ow in ONES_WEIGHTS:
                if (9, form, vf, ow, False) not in cases:
                    cases.append((9, form, vf, ow, False))
        cases.append((9, form, "fractional", 9000.0, True))
    return cases


def criteria_case(B, form, valid_form, gaps, seed=None):
    """-> (levels, n_rows, logits-or-probabilities, labels, valid, coord_pred, coord_y) float32.  Labels: sparse 0 / 1 with 0.999,
    1.0 and 1 - 2^-24 placed in every frame; asserted: the loop branches the batch is there for, the BCE partial count, the valid
    form."""
    levels = CRIT_GAP_LEVELS if gaps else CRIT_LEVELS
    n_rows = n_rows_of(levels, 5 if gaps else 0)
    tiled = sum(s * s for _, s in levels) == n_rows
    assert tiled == (not gaps)
    rs = np.random.RandomState(1000 + B if seed is None else seed)
    shape = (B, n_rows, 4)
    if form[0] == "probs":
        x = rs.uniform(0.001, 0.999, shape).astype(np.float32)
    else:
        x = (rs.standard_normal(shape) * 2).astype(np.float32)
    y = (rs.uniform(0, 1, shape) < 0.03).astype(np.float32)
    for k, val in enumerate(NEAR_ONE):
        y[:, 11 + 37 * k, k % 4] = val
        y[:, 200 + k, 3] = val
    assert NEAR_ONE[2] < 1 and float(NEAR_ONE[2]) == 1 - 2.0 ** -24 and all((y == val).any() for val in NEAR_ONE)
    if valid_form == "fractional":
        v = rs.uniform(0, 1, shape).astype(np.float32)
        assert ((v > 0) & (v < 1)).mean() > 0.9
    else:
        v = (rs.uniform(0, 1, shape) < 0.6).astype(np.float32)
    v[0, :, 1] = 0                                                # one (frame, channel) invalid: the other frames carry the slot
    if valid_form == "channel2_invalid":
        v[:, :, 2] = 0                                            # a (level, channel) invalid in EVERY frame: nv == 0 -> 1
        assert not v[:, :, 2].any() and v[:, :, 0].any()
    cp = rs.uniform(0, 15, (4 * B, 2)).astype(np.float32)
    cy = rs.uniform(0, 15, (4 * B, 2)).astype(np.float32)
    cy[1] = cp[1]                                                 # a zero difference: MAE's sign(0) = 0
    # the branches: eights over the batch (rounds, remainder), the 8 x 128 unroll of the BCE partials
    rounds, rem = divmod(B, BATCH_UNROLL)
    partials = B * sum(n_chunks(s) for _, s in levels) if tiled else min(BCE_BLOCKS, max(1, (B * n_rows + 511) // 512))
    unrolled = partials > 7 * 128
    want = {7: (0, 7, False), 8: (1, 0, False), 9: (1, 1, False), 17: (2, 1, False), 224: (28, 0, False), 225: (28, 1, True)}
    if tiled:
        assert (rounds, rem, unrolled) == want[B] and (B != 224 or partials == 896) and (B != 225 or partials == 900)
    return levels, n_rows, x.reshape(-1, 4), y.reshape(-1, 4), v.reshape(-1, 4), cp, cy


# ---------------------------------------------------------------------------
# input builders: the stand-alone BCE
# ---------------------------------------------------------------------------
BCE_SIZES = (1, 2, 3, 5, 1023 * 4 + 3, 4 * (1048576 + 524288 + 300) + 3)
BCE_SPECIAL_LOGITS = (17.0, -100.0, 88.8, 0.0, 100.0, -88.8, -17.0)
BCE_SPECIAL_PROBS = (0.0, 1.0, 0.0, 1.0, 1e-45, 0.5, 1e-45)            # with labels 0, 1, 1, 0, 1, 1, 0
BCE_SPECIAL_LABELS = (0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 0.0)


def bce_case(n, probs, seed=21):
    """(x, y, valid | None) float32 [n]: the special values first (as many as fit, repeated at the end of large arrays so that they
    also meet the strided loop's second iteration and the scalar tail), random values between.  Asserted for the large size: the grid
    is capped, the second iteration runs with the `two` guard true in some lanes and false in others, and 3 tail elements remain."""
    rs = np.random.RandomState(seed + n % 97)
    if probs:
        x = rs.uniform(0, 1, n).astype(np.float32)
        sx = np.array(BCE_SPECIAL_PROBS, np.float32)
    else:
        x = (rs.standard_normal(n) * 4).astype(np.float32)
        sx = np.array(BCE_SPECIAL_LOGITS, np.float32)
    y = (rs.uniform(0, 1, n) < 0.2).astype(np.float32)
    if n > 16:
        y[rs.randint(0, n, 8)] = np.float32(0.999)
    sy = np.array(BCE_SPECIAL_LABELS, np.float32)
    k = min(n, len(sx))
    x[:k], y[:k] = sx[:k], sy[:k]
    if n > 64:
        x[-len(sx):], y[-len(sx):] = sx, sy
        if probs:
            assert (x == 0).any() and (x == 1).any() and ((x > 0) & (x < 1e-44)).any()      # 1e-45: the smallest denormal
    v = None if n in (1, 3, BCE_SIZES[-2]) else (rs.uniform(0, 1, n) < 0.8).astype(np.float32)
    if v is not None:
        v[0] = 1
    n4 = n // 4
    blocks = min(BCE_BLOCKS, max(1, (n4 + 2 * THREADS - 1) // (2 * THREADS)))
    stride = blocks * THREADS
    if n == BCE_SIZES[-1]:
        lanes = np.arange(stride)
        second, second_two = lanes + 2 * stride < n4, lanes + 3 * stride < n4
        assert blocks == BCE_BLOCKS and second.all() and second_two.any() and not second_two.all() and n % 4 == 3
    if n == BCE_SIZES[-2]:
        assert blocks == 2 and n4 == 1023 and n % 4 == 3            # the `two` guard false in the last lane of the first iteration
    return x, y, v


# ---------------------------------------------------------------------------
# input builders: the evaluator record
# ---------------------------------------------------------------------------
RECORD_BATCHES = (255, 256, 257, 600)


def record_coord_case(B, seed=31):
    """(pred, gt [B,4,2], px, py [B]) float32 with a zero labelled width whose predicted width is not zero (lvid of frame 1: MPE inf)
    and, at an even batch, one whose predicted width is zero as well (lvid of the last frame: 0 / 0 = NaN, and inf + NaN = NaN)."""
    rs = np.random.RandomState(seed + B)
    pred = rs.uniform(0, 223, (B, 4, 2)).astype(np.float32)
    gt = np.floor(rs.uniform(0, 224, (B, 4, 2))).astype(np.float32)
    px = rs.uniform(0.2, 0.9, B).astype(np.float32)
    py = rs.uniform(0.2, 0.9, B).astype(np.float32)
    gt[1, 1] = gt[1, 0]
    if B % 2 == 0:
        gt[B - 1, 1] = gt[B - 1, 0]
        pred[B - 1, 1] = pred[B - 1, 0]
    assert (pred[1, 1] != pred[1, 0]).any()
    rounds, rem = divmod(B, RECORD_ROUND)
    assert (rounds, rem) == {255: (0, 255), 256: (1, 0), 257: (1, 1), 600: (2, 88)}[B]
    return pred, gt, px, py


def record_hm_case(B=257, F=4, seed=41):
    """(logits, labels, valid [B * n_rows, 4], px, py, n_rows): frame 4 main grid behind 5 other rows; landmark 2 has no valid row in
    any frame; landmarks 0 and 1 of frame 3 are labelled at the same position (a zero labelled width: MPE inf)."""
    rs = np.random.RandomState(seed)
    n_rows = 5 + F * F
    x = (rs.standard_normal((B, n_rows, 4)) * 3).astype(np.float32)
    y = np.zeros((B, n_rows, 4), np.float32)
    pos = np.stack([rs.permutation(F * F)[:4] for _ in range(B)])          # four different positions per frame: no other zero width
    pos[3, 1] = pos[3, 0]
    for c in range(4):
        y[np.arange(B), 5 + pos[:, c], c] = 1
    v = (rs.uniform(0, 1, (B, n_rows, 4)) < 0.7).astype(np.float32)
    v[:, :, 2] = 0
    v[0::5, :, 3] = 0                                      # some frames without a valid row of landmark 3
    assert not v[:, -F * F:, 2].any() and v[:, -F * F:, 0].any() and divmod(B, RECORD_ROUND) == (1, 1)
    px = rs.uniform(0.2, 0.9, B).astype(np.float32)
    py = rs.uniform(0.2, 0.9, B).astype(np.float32)
    return x.reshape(-1, 4), y.reshape(-1, 4), v.reshape(-1, 4), px, py, n_rows


def split_finite(ref64):
    """(finite mask, the reference with its inf / NaN entries replaced by 0): Report.check takes the finite entries, the others are
    compared as IEEE classes."""
    ok = torch.isfinite(ref64)
    return ok, torch.where(ok, ref64, torch.zeros_like(ref64))


def same_nonfinite(got, ref64):
    got, ref64 = got.detach().cpu().to(F64).reshape(ref64.shape), ref64.to(F64)
    return bool((torch.isnan(got) == torch.isnan(ref64)).all() and (torch.isposinf(got) == torch.isposinf(ref64)).all()
                and (torch.isneginf(got) == torch.isneginf(ref64)).all())
