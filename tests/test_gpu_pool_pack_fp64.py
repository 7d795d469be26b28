"""-m gpu: the average-pool pyramid (csrc/pool.hip) and the node packing with and without the 1 x 1 convolution (csrc/pack.hip)
against tests/pool_reference.py in float64, with torch's own operators on the CPU in float32 as the yardstick, under the rule of
coord_reference.Report.check:

    |kernel - fp64| <= 4 max|ref32 - fp64| + 8 ulp x scale,    scale = the per-output sum of the summands' magnitudes.

Every pool case asserts its route plan (pool_reference.plan) before a kernel runs: derived levels read from global memory and from
LDS, two derived chains in one launch, the 16-level instantiation of the backward, missing level gradients and the frame's own
gradient, bands of 28 rows with a last band of 1, 2 or 3, frames under 4 and over 256 columns, and every side of three frames
(the device's own window arithmetic).  Inputs are zero-mean standard normal unless a case says otherwise."""
import ctypes as ct

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import pool_reference as R
from coord_reference import Report
from echoglad_amd import _lib, ops
from echoglad_amd.ops import pack as P
from echoglad_amd.ops._core import raw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


def _randn(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32))


def _torch32(x, sides, grads, frame_grad=None):
    """torch's own adaptive_avg_pool2d and its autograd on the CPU in float32 -> (maps, dx)."""
    x = x.detach().clone().requires_grad_(True)
    maps = [TF.adaptive_avg_pool2d(x, (p, p)) for p in sides]
    have = [(m, g) for m, g in zip(maps, grads) if g is not None]
    dx = torch.zeros_like(x)
    if have:
        dx, = torch.autograd.grad([m for m, _ in have], x, [g for _, g in have])
    if frame_grad is not None:
        dx = frame_grad + dx
    return [m.detach() for m in maps], dx


def _finish(rep, capsys, title, bad=()):
    with capsys.disabled():
        print(rep.table(title))
    assert not rep.failed() and not bad, (rep.failed(), list(bad))


def _pool_both_ways(rep, F, sides, planes, seed, bad, twice=True):
    """Forward and x.grad of ops.avg_pool_pyramid under the rule; the bits of a second call."""
    rs = np.random.RandomState(seed)
    x = _randn(rs, *planes, F, F)
    gs = [_randn(rs, *planes, p, p) for p in sides]
    ref64, scale = R.pool_fwd(x, sides), R.pool_fwd_scale(x, sides)
    maps32, dx32 = _torch32(x, sides, gs)
    dx64, dscale = R.pool_bwd(gs, None, sides, x.shape), R.pool_bwd_scale(gs, None, sides, x.shape)
    gd = [g.to(DEV) for g in gs]
    xd = x.to(DEV).requires_grad_(True)
    got = ops.avg_pool_pyramid(xd, sides)
    dx, = torch.autograd.grad(got, xd, gd)
    for p, g, r64, r32, sc in zip(sides, got, ref64, maps32, scale):
        assert g.shape == r32.shape
        if not rep.check("pool forward", g, r64, r32, sc):
            bad.append(("forward", F, p))
    if not rep.check("pool x.grad", dx, dx64, dx32, dscale):
        bad.append(("x.grad", F, tuple(sides)))
    if twice:
        xd2 = x.to(DEV).requires_grad_(True)
        got2 = ops.avg_pool_pyramid(xd2, sides)
        dx2, = torch.autograd.grad(got2, xd2, gd)
        assert all(torch.equal(a, b) for a, b in zip(got, got2)) and torch.equal(dx, dx2)


# ---------------------------------------------------------------------------
# 1. the pool, forward and backward, on the routes of csrc/pool.hip
# ---------------------------------------------------------------------------
def _d(p, src, kept):
    return (p, "derived", src, kept)


NAMED = {
    # a derived level too large for LDS (92 x 92 > 8192 floats): the next one reads it back from global memory
    "derived-from-global-184": (184, [23, 46, 92, 184], (2, 2),
                                [(184, "direct"), _d(92, "global", False), _d(46, "global", True), _d(23, "lds", False)]),
    "derived-from-global-256": (256, [32, 64, 128, 256], (1, 2),
                                [(256, "direct"), _d(128, "global", False), _d(64, "global", True), _d(32, "lds", False)]),
    "derived-from-global-512": (512, [64, 128, 256], (1, 2), [(256, "direct"), _d(128, "global", False), _d(64, "global", False)]),
    # two derived chains in one launch, direct levels between them
    "two-chains-24": (24, [1, 2, 3, 5, 6, 12, 24], (2, 2),
                      [(24, "direct"), _d(12, "global", True), _d(6, "lds", False), (5, "direct"), (3, "direct"), (2, "direct"),
                       _d(1, "global", False)]),
    # 16 levels: k_pool_pyramid_bwd<16>
    "sixteen-levels-40": (40, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 20, 24, 32, 40], (2, 2),
                          [(p, "direct") for p in (40, 32, 24, 20, 16, 12, 10, 9, 8, 7, 6, 5, 4, 3, 2)] + [_d(1, "global", False)]),
    # the model's own frame
    "model-224": (224, [2, 4, 8, 16, 32, 64, 128], (2, 2),
                  [(128, "direct"), (64, "direct"), (32, "direct"), _d(16, "global", True), _d(8, "lds", True), _d(4, "lds", True),
                   _d(2, "lds", False)]),
}


@pytest.mark.parametrize("name", list(NAMED))
def test_pool_routes(name, capsys):
    F, sides, planes, plan = NAMED[name]
    assert R.plan(F, sides) == plan                    # the case reaches the route it is named for
    rep, bad = Report(), []
    _pool_both_ways(rep, F, sides, planes, 100 + F, bad)
    _finish(rep, capsys, f"pool {name}: F {F}, sides {sides}, planes {planes}", bad)


EDGES = {
    1: [1], 2: [1, 2], 3: [1, 2, 3],                                # frames under 4 columns, side 1, side == F
    29: [2, 4, 28, 29],                                             # a last band of one row
    30: [1, 2, 4, 8, 15, 30], 31: [1, 2, 4, 8, 16, 31],             # ... of two and of three rows
    257: [1, 128, 129, 256, 257],                                   # a second column pass with one column
    511: [1, 2, 255, 256, 510, 511],
    512: [1, 2, 3, 255, 257, 341, 511, 512],
}


@pytest.mark.parametrize("F", list(EDGES))
def test_pool_edges(F, capsys):
    rep, bad = Report(), []
    _pool_both_ways(rep, F, EDGES[F], (2, 2) if F < 100 else (1, 2), 200 + F, bad)
    _finish(rep, capsys, f"pool edges: F {F}, sides {EDGES[F]}", bad)


@pytest.mark.parametrize("F,planes", [(29, (1, 2)), (61, (1, 2)), (257, (1, 1))])
def test_pool_every_side_of_a_frame(F, planes, capsys):
    """Every side 1 .. F in calls of 16 ascending sides: the device's own windows_of (the float32 guess and the candidates around
    it) and the direct kernel's rs, re, cs, ce at every (F, p), and k_pool_pyramid_bwd<16> with irregular windows."""
    rep, bad = Report(), []
    for lo in range(1, F + 1, 16):
        _pool_both_ways(rep, F, list(range(lo, min(lo + 16, F + 1))), planes, 300 + F + lo, bad, twice=False)
    _finish(rep, capsys, f"pool sweep: F {F}, every side", bad)


# ---------------------------------------------------------------------------
# 2. missing level gradients and the frame's own gradient (eg_avg_pool_pyramid_bwd through ops.pack._pool_bwd)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two-chains-24", "sixteen-levels-40"])
def test_pool_backward_with_missing_levels_and_a_frame_gradient(name, capsys):
    F, sides, planes, _ = NAMED[name]
    rs = np.random.RandomState(400 + F)
    shape = (*planes, F, F)
    x = _randn(rs, *shape)
    gs = [_randn(rs, *planes, p, p) for p in sides]
    gf = _randn(rs, *shape)
    n = len(sides)
    rep, bad = Report(), []
    for tag, missing in (("levels 1 and 3 missing", {1, 3}), ("all but the last missing", set(range(n - 1)))):
        for frame_grad in (None, gf):
            g = [None if l in missing else gl for l, gl in enumerate(gs)]
            dx = P._pool_bwd([None if t is None else t.to(DEV) for t in g], None if frame_grad is None else frame_grad.to(DEV), sides, shape, DEV)
            dx32 = _torch32(x, sides, g, frame_grad)[1]
            if not rep.check("dx, " + tag + (", frame_grad" if frame_grad is not None else ""), dx, R.pool_bwd(g, frame_grad, sides, shape),
                             dx32, R.pool_bwd_scale(g, frame_grad, sides, shape)):
                bad.append((tag, frame_grad is not None))
    dx = P._pool_bwd([None] * n, gf.to(DEV), sides, shape, DEV)
    assert torch.equal(dx.cpu(), gf)                                  # nothing but the frame's own gradient: its bits
    _finish(rep, capsys, f"pool backward, NULL levels: F {F}, {n} levels", bad)


# ---------------------------------------------------------------------------
# 3. ops.pyramid_pack: the model's node (pool + packing as one autograd node)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("row_offset,spare", [(0, 0), (5, 3), (0, 3), (5, 0)])
@pytest.mark.parametrize("F,sides,batch", [(24, [2, 4, 8], 3), (30, [2, 4, 8, 16], 2)])
def test_pyramid_pack(F, sides, batch, row_offset, spare, capsys):
    rs = np.random.RandomState(500 + F + row_offset + spare)
    x = _randn(rs, batch, 128, F, F)
    used = sum(p * p for p in sides) + F * F
    n_rows = row_offset + used + spare
    g = _randn(rs, batch * n_rows, 128)
    x64 = x.to(F64)
    pk = lambda maps: R.pack_rows(maps, batch, n_rows, row_offset)
    ref64, scale = pk(R.pool_fwd(x, sides) + [x64]), pk(R.pool_fwd_scale(x, sides) + [x64.abs()])
    x32 = x.clone().requires_grad_(True)
    ref32 = pk([TF.adaptive_avg_pool2d(x32, (p, p)) for p in sides] + [x32])
    dx32, = torch.autograd.grad(ref32, x32, g)
    gl = R.unpack_rows(g.to(F64), sides + [F], batch, n_rows, row_offset)
    dx64, dscale = R.pool_bwd(gl[:-1], gl[-1], sides, x.shape), R.pool_bwd_scale(gl[:-1], gl[-1], sides, x.shape)

    xd = x.to(DEV).requires_grad_(True)
    got = ops.pyramid_pack(xd, sides, batch, n_rows, row_offset)
    dx, = torch.autograd.grad(got, xd, g.to(DEV))
    rep = Report()
    rep.check("node rows", got, ref64, ref32.detach(), scale)
    rep.check("x.grad", dx, dx64, dx32, dscale)
    v = got.detach().view(batch, n_rows, 128)
    assert not v[:, :row_offset].any() and not v[:, row_offset + used:].any()          # rows no level covers: exactly zero
    assert torch.equal(v[:, row_offset + used - F * F:row_offset + used].cpu(), x.permute(0, 2, 3, 1).reshape(batch, F * F, 128))
    # out=: the allocating call's bits, rows outside the levels zeroed; not differentiable
    out = torch.full((batch * n_rows, 128), float("nan"), device=DEV)
    with torch.no_grad():
        ops.pyramid_pack(x.to(DEV), sides, batch, n_rows, row_offset, out=out)
    assert torch.equal(out, got.detach())
    with pytest.raises(RuntimeError, match="not differentiable"):
        ops.pyramid_pack(xd, sides, batch, n_rows, row_offset, out=out)
    _finish(rep, capsys, f"pyramid_pack: F {F}, sides {sides}, batch {batch}, row_offset {row_offset}, spare {spare}")


# ---------------------------------------------------------------------------
# 4. one thread's sequential sum over a large window, data with an offset: a measurement under the first-order worst case
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("F,side", [(250, 2), (512, 1)])
def test_direct_sum_over_a_large_window_with_offset_data(F, side, capsys):
    """k_pool_direct sums a window with one thread, element after element.  With x = N(0, 1) + 3 a sequential float32 sum misses the
    8-ulp rule (on the CPU: off by 1.5e-5 at 512 / 1 where torch's op is off by 3e-7), so this asserts only the first-order worst
    case of an n-term sequential sum, (n - 1) 2^-24 x scale, and prints the kernel's error next to torch's float32 operators'.
    Measured on an MI355X: 250 / 2: kernel 1.13e-5, torch CPU 1.13e-5, torch GPU 1.13e-5 (not the same bits);
    512 / 1: kernel 7.06e-6, torch CPU and GPU 9.8e-8 (72 x; a side of 1 is no side of the model's pyramid: those are 2^g, g >= 1)."""
    assert R.plan(F, [side]) == [(side, "direct")]
    rs = np.random.RandomState(600 + F)
    x = _randn(rs, 1, 2, F, F) + 3.0
    ref64, = R.pool_fwd(x, [side])
    scale, = R.pool_fwd_scale(x, [side])
    n = (-(-F // side)) ** 2
    got, = ops.avg_pool_pyramid(x.to(DEV), [side])
    err = (got.cpu().to(F64) - ref64).abs()
    e_cpu = float((TF.adaptive_avg_pool2d(x, (side, side)).to(F64) - ref64).abs().max())
    t_gpu = TF.adaptive_avg_pool2d(x.to(DEV), (side, side))
    e_gpu = float((t_gpu.cpu().to(F64) - ref64).abs().max())
    e = float(err.max())
    with capsys.disabled():
        print(f"\n  direct sum, F {F}, side {side}, n {n}, x = N(0,1) + 3: max|kernel - fp64| {e:.3e}, torch CPU float32 {e_cpu:.3e}, "
              f"torch GPU float32 {e_gpu:.3e}; kernel / CPU {e / e_cpu:.2f}, kernel / GPU {e / e_gpu:.2f}; "
              f"bits of torch's GPU op: {torch.equal(got, t_gpu)}; bound (n - 1) 2^-24 scale {float(((n - 1) * 2.0 ** -24 * scale).min()):.3e}")
    assert bool((err <= (n - 1) * 2.0 ** -24 * scale).all()), (e, e_cpu, e_gpu)


# ---------------------------------------------------------------------------
# 5. relu(conv1x1) fused into the packing
# ---------------------------------------------------------------------------
# the seed of every case: chosen on the CPU so that, on the references alone, the float32 mask is the float64 mask and
# min|s64| >= 64 max|s32 - s64| (the backward recomputes the mask in float32)
CONV_SEEDS = {
    (((2, 3, 8), (32, 31, 64), 2, 0, 0), "all"): 1, (((2, 3, 8), (32, 31, 64), 2, 0, 0), "none"): 1,           # ratios 75, 135
    (((2, 3, 8), (32, 31, 64), 2, 0, 0), "mixed"): 1,                                                             # 75
    (((1, 4, 17), (1, 33, 5), 1, 2, 3), "all"): 2, (((1, 4, 17), (1, 33, 5), 1, 2, 3), "none"): 4,               # 89, 80
    (((1, 4, 17), (1, 33, 5), 1, 2, 3), "mixed"): 2,                                                              # 92
    (((6,), (512,), 2, 0, 1), "all"): 3, (((6,), (512,), 2, 0, 1), "none"): 0, (((6,), (512,), 2, 0, 1), "mixed"): 3,   # 246, 124, 246
}


def conv_case_under_the_rule(rep, case, bias, seed):
    """One conv-pack case against float64: the condition on the references first, then the kernel; values and all gradients."""
    fx = R.conv_fixture(*case, bias, seed)
    r64 = R.conv_pack64(fx["feats"], fx["weights"], fx["biases"], fx["batch"], fx["n_rows"], fx["row_offset"], dnodes=fx["dnodes"])
    r32 = R.conv_torch32(fx)
    same, ratio = R.relu_margin(r64["s"], r32["s"])
    assert same and ratio >= R.MARGIN, (case, bias, seed, same, ratio)          # before any kernel runs
    dev = lambda t: None if t is None else t.to(DEV).requires_grad_(True)
    feats, ws, bs = [dev(t) for t in fx["feats"]], [dev(t) for t in fx["weights"]], [dev(t) for t in fx["biases"]]
    got = ops.conv1x1_relu_pack_levels(feats, ws, bs, fx["batch"], fx["n_rows"], fx["row_offset"])
    grads = list(torch.autograd.grad(got, feats + ws + [b for b in bs if b is not None], fx["dnodes"].to(DEV)))
    n = len(feats)
    rep.check("node rows", got, r64["out"], r32["out"], r64["scale"])             # every element, no zero pattern left out
    v = got.detach().view(fx["batch"], fx["n_rows"], 128)
    used = sum(p * p for p in fx["sides"])
    assert not v[:, :fx["row_offset"]].any() and not v[:, fx["row_offset"] + used:].any()
    db = iter(grads[2 * n:])
    for l in range(n):
        rep.check("d features", grads[l], r64["dfeat"][l], r32["dfeat"][l], r64["dfeat_scale"][l])
        rep.check("d weight", grads[n + l], r64["dw"][l], r32["dw"][l], r64["dw_scale"][l])
        if bs[l] is not None:
            rep.check("d bias", next(db), r64["db"][l], r32["db"][l], r64["db_scale"][l])
    return ratio


@pytest.mark.parametrize("bias", R.BIAS_MODES)
@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: "-".join(map(str, c[0])) + "x" + "-".join(map(str, c[1])))
def test_conv1x1_relu_pack_against_float64(case, bias, capsys):
    """Whole CP_CC passes (32, 64 channels), one short of a pass (31), one over (33), one channel, 512 channels; sides 1 .. 17, the
    16-byte and the element-wise route; biases present, absent (NULL) and mixed."""
    rep = Report()
    ratio = conv_case_under_the_rule(rep, case, bias, CONV_SEEDS[(case, bias)])
    _finish(rep, capsys, f"conv1x1_relu_pack {case}, biases {bias} (min|s64| / max|s32 - s64| = {ratio:.0f})")


# ---------------------------------------------------------------------------
# 6. 16-byte accesses and addresses that are no multiple of 16
# ---------------------------------------------------------------------------
def _odd_view(t):
    """A contiguous view of t's values that starts one element into a buffer: 4 bytes past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:] = t.reshape(-1)
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _ptrs(*tensors):
    return (ct.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def test_entry_points_refuse_unaligned_16_byte_operands():
    """Through the raw entry points: an even-side map, the node rows or a bias at an address that is no multiple of 16 is EG_ERR_ARG
    before any launch (the destination keeps its bits); an odd-side map goes element by element and is taken."""
    rs = np.random.RandomState(7)
    even, odd = _randn(rs, 1, 128, 4, 4).to(DEV), _randn(rs, 1, 128, 3, 3).to(DEV)
    one = (ct.c_int * 1)
    mark = torch.full((16, 128), 7.0, device=DEV)
    nodes = mark.clone()
    assert raw("eg_pack_levels", _ptrs(_odd_view(even)), one(4), 1, 1, 16, 0, nodes) == _lib.EG_ERR_ARG
    assert "16-byte" in _lib.last_error()
    assert raw("eg_pack_levels", _ptrs(even), one(4), 1, 1, 16, 0, _odd_view(mark)) == _lib.EG_ERR_ARG
    gmap = _odd_view(torch.full((1, 128, 4, 4), 7.0, device=DEV))
    assert raw("eg_unpack_levels", nodes, _ptrs(gmap), one(4), 1, 1, 16, 0) == _lib.EG_ERR_ARG
    assert raw("eg_unpack_levels", _odd_view(mark), _ptrs(torch.empty_like(even)), one(4), 1, 1, 16, 0) == _lib.EG_ERR_ARG
    feat, w, b = _randn(rs, 1, 8, 4, 4).to(DEV), _randn(rs, 128, 8).to(DEV), _randn(rs, 128).to(DEV)
    conv = lambda f, bias, dst, side: raw("eg_conv1x1_relu_pack_levels", _ptrs(f), _ptrs(w), _ptrs(bias), one(8), one(side), 1, 1, 16, 0, dst)
    assert conv(_odd_view(feat), b, nodes, 4) == _lib.EG_ERR_ARG
    assert conv(feat, _odd_view(b), nodes, 4) == _lib.EG_ERR_ARG
    assert conv(feat, b, _odd_view(mark), 4) == _lib.EG_ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(nodes, mark) and torch.equal(gmap, torch.full_like(gmap, 7.0))          # nothing was launched
    # the element-wise route takes any float address
    odd_v = _odd_view(odd)
    assert raw("eg_pack_levels", _ptrs(odd_v), one(3), 1, 1, 16, 0, nodes) == _lib.EG_OK
    want = R.pack_rows([odd], 1, 16, 0)
    assert torch.equal(nodes[:9], want[:9]) and torch.equal(nodes[9:], mark[9:])
    back = _odd_view(torch.zeros_like(odd))
    assert raw("eg_unpack_levels", nodes, _ptrs(back), one(3), 1, 1, 16, 0) == _lib.EG_OK
    assert torch.equal(back, odd)
    feat3 = _randn(rs, 1, 8, 3, 3).to(DEV)
    assert conv(_odd_view(feat3), b, nodes, 3) == _lib.EG_OK
    aligned = mark.clone()
    assert conv(feat3, b, aligned, 3) == _lib.EG_OK
    assert torch.equal(nodes, aligned)


def test_wrappers_take_contiguous_views_at_odd_offsets():
    """ops.pack_levels and ops.conv1x1_relu_pack_levels copy such operands (as ops.bce_logits does): the bits of aligned clones,
    forward and backward."""
    rs = np.random.RandomState(8)
    sides, batch = [2, 3, 4], 2
    n_rows = 1 + sum(p * p for p in sides) + 2
    maps = [_randn(rs, batch, 128, p, p).to(DEV) for p in sides]
    g = _randn(rs, batch * n_rows, 128).to(DEV)
    res = []
    for view in (lambda t: t.clone(), _odd_view):
        ms = [view(m).requires_grad_(True) for m in maps]
        out = ops.pack_levels(ms, batch, n_rows, 1)
        res.append([out.detach()] + list(torch.autograd.grad(out, ms, view(g))))
        dst = view(torch.full((batch * n_rows, 128), float("nan"), device=DEV))
        with torch.no_grad():
            ops.pack_levels([view(m) for m in maps], batch, n_rows, 1, out=dst)
        res[-1].append(dst)
    assert torch.equal(res[0][0], R.pack_rows(maps, batch, n_rows, 1))
    assert all(torch.equal(a, b) for a, b in zip(*res)) and torch.equal(res[1][0], res[1][-1])
    chans = [8, 5, 33]
    feats = [_randn(rs, batch, c, p, p).to(DEV) for p, c in zip(sides, chans)]
    ws = [(_randn(rs, 128, c) / c ** 0.5).to(DEV) for c in chans]
    bs = [_randn(rs, 128).to(DEV), None, _randn(rs, 128).to(DEV)]
    res = []
    for view in (lambda t: t.clone(), _odd_view):
        leaf = lambda t: None if t is None else view(t).requires_grad_(True)
        f, w, b = [leaf(t) for t in feats], [leaf(t) for t in ws], [leaf(t) for t in bs]
        out = ops.conv1x1_relu_pack_levels(f, w, b, batch, n_rows, 1)
        res.append([out.detach()] + list(torch.autograd.grad(out, f + w + [t for t in b if t is not None], view(g))))
    assert all(torch.equal(a, b) for a, b in zip(*res))
    assert float(res[0][0].abs().max()) > 0
