"""A plain restatement of eg_heatmap_render (csrc/heatmap_render.hip; include/echoglad_hip.h states the arithmetic): torch on the
CPU, no kernels, every function taking ``dtype`` like tests/heatmap_reference.py.  float64 is the truth; the same code in float32 is
"what the host would compute" -- and, for the two images that involve no transcendental (``base``, ``gt``), exactly what the
kernel must compute: correctly rounded fp32 multiplies in the stated order leave no freedom.  The fp32 inputs are converted
exactly, and the constants (0.8, the colours, 255) are the FLOAT constants in both types, as the reference's FloatTensors are.

The rule (coord_reference.Report, imported, not forked):  |kernel - fp64| <= FACTOR * max|ref32 - fp64| + 8 * 2^-23 * scale.
A softmax weight's scale is p * (1 + |x - M| / 16), heatmap_reference.py's convention (its ``decode`` supplies p and |x - M|; the
factor is applied where p > 0, as there); the normalised map e = exp(x - M) takes the same factor.

Bytes (``pred``): a byte is the truncation of the largest of five CANDIDATES times 255 -- the four channels' col * e_c and the base.
Truncation is discontinuous at the integers, so a candidate that lies within its tolerance tau = FACTOR * max|v32 - v64| + 8 * 2^-23 *
scale of an integer in 1..255 may put the kernel's byte on the other side: there the byte may differ from the fp64 byte by exactly
1, everywhere else it must be equal.  An EXCUSED byte is one that differs and is let through by that rule.  The cap: at most 1 % of
the compared bytes of a case may be excused; every builder asserts that the float32 restatement alone stays under it (with tau about
3e-4 around each integer some 0.06 % of random values could be excused at all), so a case over the cap gets another seed, never
another cap.  The exact case (x - M in {0, -inf}, image on the k / 255 lattice) allows none.

The input builders of tests/test_gpu_heatmap_render.py live here; each ASSERTS the condition it was built for, and
tests/test_heatmap_render_reference.py runs every builder of every parametrised case without a GPU."""
import functools
import itertools

import numpy as np
import torch

import heatmap_reference as H
from coord_reference import FACTOR, ULP, Report          # noqa: F401  (the rule itself: one owner)

F64, F32 = torch.float64, torch.float32
COLOURS = ((0.0, 1.0, 1.0), (1.0, 0.7, 0.9), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0))       # evaluators.py:608, channels 0..3
GREY = 0.8
CAP = 0.01                  # excused bytes / compared bytes, per case
PIX = 4                     # pixels per thread of k_hm_render: 12 RGB bytes = 3 dwords
BATCH = 5


def _f(v, dtype):
    """The float constant v in `dtype` (0.7f is not 0.7)."""
    return torch.tensor(float(np.float32(v)), dtype=dtype)


def weight_scale(w, xm):
    """heatmap_reference.py's convention for a softmax weight w: w * (1 + |x - M| / 16), the factor only where w > 0."""
    w, xm = w.to(F64), xm.to(F64)
    return w * (1 + torch.where(w > 0, xm, torch.zeros_like(xm)) / 16)


def to_bytes(v):
    """ToPILImage's mul(255).byte(), saturating: trunc(min(v * 255, 255)); NaN and anything below 0 give 0."""
    s = v * _f(255.0, v.dtype)
    s = torch.where(torch.isnan(s), torch.zeros_like(s), s).clamp(0.0, 255.0)
    return torch.floor(s).to(torch.uint8)


def render(logits, count, n_rows, level_start, side, labels=None, image=None, dtype=F64):
    """logits / labels [count * n_rows, 4] (the rendered frames only), image [count, side, side] | None (black) ->
    dict(heat [count,side,side,4], e (the normalised maps, same shape), xm (|x - M|, 0 where the weight is 0), base / pred / gt: the
    values [count,side,side,3] in `dtype` before the bytes ("v_base", ...) and the uint8 images, cand [count,side,side,3,5]: the
    five candidates of every pred byte times 255, cand_scale: their scales)."""
    n = side * side
    d = H.decode(logits, count, [(level_start, side)], dtype=dtype)
    x = H.t(logits, dtype).reshape(count, n_rows, 4)[:, level_start:level_start + n, :]
    M = x.max(dim=1, keepdim=True).values
    empty = torch.isneginf(M).expand_as(x)                   # a channel without a finite logit: no mass, the map is 0
    zero = torch.zeros_like(x)
    p = torch.where(empty, zero, d["p"][0])
    e = torch.where(empty, zero, torch.exp(x - M))
    xm = torch.where(e > 0, d["xm"][0], zero)
    shape = (count, side, side)
    img = torch.zeros(shape, dtype=dtype) if image is None else H.t(image, dtype).reshape(shape)
    base = torch.maximum(torch.zeros_like(img), _f(GREY, dtype) * img)
    col = torch.tensor([[float(np.float32(v)) for v in c] for c in COLOURS], dtype=dtype)          # [4 channels, 3 RGB]

    def overlay(maps):              # maps [count, n, 4] -> values [count, side, side, 3]: colour * value, then max
        v = base.unsqueeze(-1).expand(*shape, 3)
        for c in range(4):
            v = torch.maximum(v, col[c].view(1, 1, 1, 3) * maps[:, :, c].reshape(*shape, 1))
        return v
    out = dict(heat=p.reshape(*shape, 4), e=e.reshape(*shape, 4), xm=xm.reshape(*shape, 4), v_base=base.unsqueeze(-1).expand(*shape, 3))
    out["v_pred"] = overlay(e)
    cand = torch.stack([col[c].view(1, 1, 1, 3) * e[:, :, c].reshape(*shape, 1) for c in range(4)] + [out["v_base"]], dim=-1)
    out["cand"] = cand * _f(255.0, dtype)
    es = weight_scale(e, xm).reshape(*shape, 4)
    out["cand_scale"] = 255.0 * torch.stack([col[c].to(F64).view(1, 1, 1, 3) * es[..., c:c + 1] for c in range(4)]
                                            + [out["v_base"].to(F64)], dim=-1)
    if labels is not None:
        y = H.t(labels, dtype).reshape(count, n_rows, 4)[:, level_start:level_start + n, :]
        out["v_gt"] = overlay(y)
    for k in ("base", "pred", "gt"):
        if "v_" + k in out:
            out[k] = to_bytes(out["v_" + k])
    return out


def heat_scale(r64):
    return weight_scale(r64["heat"], r64["xm"])


def pred_bytes_rule(got, r64, r32):
    """The byte rule for the pred image -> (bad, excused, compared): `bad` bytes break the rule (differ where no candidate is
    within its tau of an integer in 1..255, or differ by more than 1), `excused` differ by exactly 1 where one is."""
    got = torch.as_tensor(got).cpu().to(torch.int64).reshape(r64["pred"].shape)
    ref = r64["pred"].to(torch.int64)
    v64, v32 = r64["cand"].to(F64), r32["cand"].to(F64)
    ref_err = float((v32 - v64).abs().max())
    tau = FACTOR * ref_err + 8 * ULP * r64["cand_scale"]
    near = torch.round(v64)
    at_edge = ((v64 - near).abs() <= tau) & (near >= 1) & (near <= 255)
    may_differ = at_edge.any(dim=-1)
    diff = (got - ref).abs()
    bad = (diff > 1) | ((diff == 1) & ~may_differ)
    return int(bad.sum()), int(((diff == 1) & may_differ).sum()), diff.numel()


# ---------------------------------------------------------------------------
# input builders
# ---------------------------------------------------------------------------
SIDES = (1, 2, 3, 5, 33, 64)
WHAT = {1: "a single pixel", 2: "fewer pixels than one packed group", 3: "odd: 27 bytes per frame, frame 1 starts misaligned",
        5: "odd", 33: "1089 rows: crosses the 1024-row chunk of the stats kernel, a one-pixel tail", 64: "a level of 4096 rows"}
# (count, first, level_start, rows behind the level, image channels): the 2^(5-2) fractional factorial -- every value of every factor,
# and every pair of values of two factors, occurs
_FACTORS = ((1, 3), (0, 2), (0, 21), (0, 4), (1, 4))
COMBOS = tuple(tuple(f[b] for f, b in zip(_FACTORS, (a, b, c, a ^ b, a ^ c))) for a, b, c in itertools.product((0, 1), repeat=3))
CASES = [(side,) + combo for side in SIDES for combo in COMBOS]
OUTPUT_SETS = (("heat",), ("pred",), ("gt",), ("base",), ("heat", "pred", "gt", "base"))
SEED = {}                   # (side, count, first, start, behind, channels) -> seed, where the default misses the cap (none does)


def _assert_design():
    for i, j in itertools.combinations(range(5), 2):
        assert {(c[i], c[j]) for c in COMBOS} == set(itertools.product(_FACTORS[i], _FACTORS[j])), (i, j)


@functools.lru_cache(maxsize=None)
def case(side, count, first, start, behind, channels):
    """-> dict(logits, labels [5 * n_rows, 4], image [5, channels, side, side], n_rows, level, r64, r32 (render() of the frames
    first .. first + count - 1), sl (those frames' rows)).  Every frame: channel 0 N(0, 3^2); channel 1 with one row 40 above the rest;
    channel 2 all -inf inside the level (finite outside); channel 3 with -inf on every fourth row.  Labels: channels 0 and 1 one-hot,
    2 and 3 fractional.  Image: [0, 1], pixel (idx + 3 frame) % 5 == 1 below 0 and == 2 above 1.25."""
    _assert_design()
    n = side * side
    n_rows = start + n + behind
    key = (side, count, first, start, behind, channels)
    rs = np.random.RandomState(SEED.get(key, 7 + side + 100 * count + 10 * first + start + behind + channels))
    x = (rs.standard_normal((BATCH, n_rows, 4)) * 3).astype(np.float32)
    lv = slice(start, start + n)
    peak = rs.randint(0, n, BATCH)
    for b in range(BATCH):
        x[b, start + peak[b], 1] = x[b, lv, 1].max() + np.float32(40)
    x[:, lv, 2] = -np.inf
    x[:, start + 1:start + n:4, 3] = -np.inf
    y = np.zeros((BATCH, n_rows, 4), np.float32)
    y[:, :, 2:] = (rs.uniform(0, 0.9, (BATCH, n_rows, 2)) * (rs.uniform(0, 1, (BATCH, n_rows, 2)) < 0.3)).astype(np.float32)
    y[:, start, 2] = np.float32(0.37)                         # (a fractional label in the level also where it is one row)
    for b in range(BATCH):
        y[b, start + rs.randint(0, n), 0] = 1
        y[b, start + rs.randint(0, n), 1] = 1
        y[b, rs.randint(0, n_rows), 0] = 1                    # (anywhere in the frame: a row outside the level must not be drawn)
    img = rs.uniform(0, 1, (BATCH, channels, side, side)).astype(np.float32)
    which = (np.arange(n)[None, :] + 3 * np.arange(BATCH)[:, None]) % 5
    plane = img[:, 0].reshape(BATCH, n)
    plane[which == 1] = -rs.uniform(0.01, 0.5, int((which == 1).sum())).astype(np.float32)
    plane[which == 2] = rs.uniform(1.26, 2.0, int((which == 2).sum())).astype(np.float32)
    img[:, 0] = plane.reshape(BATCH, side, side)
    # what the case is there for
    sl = slice(first * n_rows, (first + count) * n_rows)
    xs, ys, ims = x.reshape(-1, 4)[sl], y.reshape(-1, 4)[sl], img[first:first + count, 0]
    xl = x[first:first + count, lv]
    assert first + count <= BATCH and np.isneginf(xl[:, :, 2]).all() and np.isfinite(x[:, :start, 2]).all() and np.isfinite(x[:, start + n:, 2]).all()
    assert ((np.sort(xl[:, :, 1], axis=1)[:, -1] - (np.sort(xl[:, :, 1], axis=1)[:, -2] if n > 1 else -np.inf)) >= 40).all()
    if n >= 4:
        assert np.isneginf(xl[:, :, 3]).any() and np.isfinite(xl[:, :, 3]).any(axis=1).all()
    if n * count >= 5:
        assert (ims < 0).any() and (ims > 1.25).any()
    assert ((ims >= 0) & (ims <= 1)).any() or n * count < 3
    assert (y[:, lv, :2].sum(axis=1) >= 1).all() and ((y[:, lv, 2:] > 0) & (y[:, lv, 2:] < 1)).any(axis=(1, 2)).all()
    if side % 2 and count > 1:
        assert (n * 3) % 4 != 0                               # frame 1's bytes start at no multiple of 4: the byte-store path
    if side == 33:
        assert n == H.CHUNK + 65 and n % PIX == 1             # two chunks of the stats kernel; the last thread owns ONE pixel
    if side == 2:
        assert n * 3 == 3 * PIX                               # exactly one packed group
    r64 = render(xs, count, n_rows, start, side, ys, ims)
    r32 = render(xs, count, n_rows, start, side, ys, ims, dtype=F32)
    out = dict(logits=x.reshape(-1, 4), labels=y.reshape(-1, 4), image=img, n_rows=n_rows, level=(start, side), r64=r64, r32=r32, sl=sl)
    assert_cap(out, key)
    return out


def assert_cap(c, key):
    """The float32 restatement alone breaks the byte rule nowhere and is excused on at most CAP of the bytes."""
    bad, excused, total = pred_bytes_rule(c["r32"]["pred"], c["r64"], c["r32"])
    assert bad == 0 and excused <= CAP * total, (key, bad, excused, total)
    return excused, total


@functools.lru_cache(maxsize=None)
def exact_case(side=33, count=2):
    """Only exact values: every logit of the level is its channel's maximum or -inf (x - M in {0, -inf}: e in {1, 0}), the image
    k / 255 with k % 5 != 0 -- 0.8 k is then at least 0.2 away from every integer, where 0.8f (a little above 0.8) times k / 255
    rounded to float times 255 would otherwise land on either side of one -- and the labels 0 / 1.  The candidates are 0, 255,
    178.5 and 229.5 up to rounding and the base: no byte sits at a truncation edge, and none is excused."""
    n = side * side
    n_rows = 3 + n + 2
    rs = np.random.RandomState(255)
    x = np.full((count, n_rows, 4), -np.inf, np.float32)
    top = np.array([2.5, -7.0, 0.0, 31.0], np.float32)
    hot = rs.uniform(0, 1, (count, n, 4)) < 0.2
    hot[:, 0, :] = True
    x[:, 3:3 + n, :] = np.where(hot, top[None, None, :], np.float32(-np.inf))
    x[:, :3, :] = 50.0                                        # larger values outside the level: not the level's maximum
    x[:, 3 + n:, :] = 50.0
    k = rs.randint(0, 256, (count, 1, side, side))
    k = np.where(k % 5 == 0, k + 1, k)
    img = (k.astype(np.float32) / np.float32(255)).astype(np.float32)
    y = (rs.uniform(0, 1, (count, n_rows, 4)) < 0.1).astype(np.float32)
    r64 = render(x.reshape(-1, 4), count, n_rows, 3, side, y.reshape(-1, 4), img[:, 0])
    r32 = render(x.reshape(-1, 4), count, n_rows, 3, side, y.reshape(-1, 4), img[:, 0], dtype=F32)
    assert set(np.unique(r64["e"].numpy())) == {0.0, 1.0} and (k % 5 != 0).all() and (k <= 256).all()
    frac = (r64["cand"] - torch.floor(r64["cand"]))
    edge = (r64["cand"] >= 1) & (r64["cand"] < 255) & ((frac < 0.1) | (frac > 0.9))
    assert not edge.any()
    for name in ("pred", "gt", "base"):
        assert torch.equal(r32[name], r64[name]), name
    return dict(logits=x.reshape(-1, 4), labels=y.reshape(-1, 4), image=img, n_rows=n_rows, level=(3, side), r64=r64, r32=r32, count=count)


def real_levels(frame=224, naux=7):
    """The row layout of the default model (224 x 224, 7 aux levels 2, 4, ..., 128 in front of the main grid) -> (levels, n_rows)."""
    out, start = [], 0
    for s in [2 ** (k + 1) for k in range(naux)] + [frame]:
        out.append((start, s))
        start += s * s
    return out, start


@functools.lru_cache(maxsize=None)
def full_case(frame=224, batch=2, seed=224):
    """Batch 2 at F = 224 with the real 224 / 7 rows: N(0, 3^2) logits with a peaked channel, frames in [0, 1], one-hot labels."""
    levels, n_rows = real_levels(frame)
    assert n_rows == 72020 and levels[-1] == (n_rows - frame * frame, frame)
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal((batch, n_rows, 4)) * 3).astype(np.float32)
    start, n = levels[-1][0], frame * frame
    for b in range(batch):
        x[b, start + rs.randint(0, n), 1] += np.float32(40)
    y = np.zeros((batch, n_rows, 4), np.float32)
    for b in range(batch):
        for c in range(4):
            y[b, start + rs.randint(0, n), c] = 1
    img = rs.uniform(0, 1, (batch, 1, frame, frame)).astype(np.float32)
    r64 = render(x.reshape(-1, 4), batch, n_rows, start, frame, y.reshape(-1, 4), img[:, 0])
    r32 = render(x.reshape(-1, 4), batch, n_rows, start, frame, y.reshape(-1, 4), img[:, 0], dtype=F32)
    out = dict(logits=x.reshape(-1, 4), labels=y.reshape(-1, 4), image=img, n_rows=n_rows, level=levels[-1], r64=r64, r32=r32, batch=batch)
    assert_cap(out, ("full", frame, batch))
    return out
