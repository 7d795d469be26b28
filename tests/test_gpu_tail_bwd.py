"""-m gpu: the UNet tail's HIP backward (csrc/pack_train.hip, ops.conv1x1_relu_pack_levels(..., backward="hip")) against
tests/pool_reference.py in float64, with torch's own operators on the CPU in float32 as the yardstick, under the rule of
coord_reference.Report.check:

    |kernel - fp64| <= 4 max|ref32 - fp64| + 8 ulp x scale,    scale = the per-output sum of the summands' magnitudes.

The kernel takes the ReLU's mask from the forward's float32 output, the float64 reference from its own pre-activations: every case
first asserts, on the references alone, that the two masks cannot differ.  The small cases do so with a margin (seeds chosen on the
CPU); the multi-slice cases use inputs whose pre-activations are exact in float32 (small integers), ties at 0 included."""
import ctypes as ct

import numpy as np
import pytest
import torch

import pool_reference as R
from coord_reference import Report
from echoglad_amd import _lib, ops
from echoglad_amd.ops import pack as P
from echoglad_amd.ops._core import raw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64

# CONV_SEEDS of tests/test_gpu_pool_pack_fp64.py: under these, on the references alone, the float32 mask is the float64 mask and
# min|s64| >= 64 max|s32 - s64|
CONV_SEEDS = {
    (((2, 3, 8), (32, 31, 64), 2, 0, 0), "all"): 1, (((2, 3, 8), (32, 31, 64), 2, 0, 0), "none"): 1,
    (((2, 3, 8), (32, 31, 64), 2, 0, 0), "mixed"): 1,
    (((1, 4, 17), (1, 33, 5), 1, 2, 3), "all"): 2, (((1, 4, 17), (1, 33, 5), 1, 2, 3), "none"): 4,
    (((1, 4, 17), (1, 33, 5), 1, 2, 3), "mixed"): 2,
    (((6,), (512,), 2, 0, 1), "all"): 3, (((6,), (512,), 2, 0, 1), "none"): 0, (((6,), (512,), 2, 0, 1), "mixed"): 3,
}

# (sides, chans, batch, front, back) -> the plan (slices, tiles per slice) per level, asserted before the kernel runs.  With the cap
# clamp(4096 / c, 16, 1024) the first four take one tile per slice; the last two reach several tiles per slice, slices that cross a
# frame boundary and a short last slice, on the 16-byte route with 8 channel passes and on the element-wise route with one.
EXACT_CASES = {
    ((2, 40), (64, 4), 3, 1, 2): ([3, 75], [1, 1]),
    ((1, 3, 65), (33, 64, 5), 1, 2, 0): ([1, 1, 67], [1, 1, 1]),
    ((4, 72), (16, 4), 2, 0, 0): ([2, 162], [1, 1]),
    ((2, 4, 8, 16), (512, 256, 31, 1), 5, 0, 4): ([5, 5, 5, 20], [1, 1, 1, 1]),
    ((3, 12), (40, 256), 7, 1, 1): ([7, 11], [1, 2]),                  # 21 tiles of 3 per frame in slices of 2: the last holds 1
    ((105,), (8,), 3, 0, 0): ([260], [2]),                             # 519 tiles of 173 per frame in slices of 2: the last holds 1
}


def _ids(case):
    return "-".join(map(str, case[0])) + "x" + "-".join(map(str, case[1]))


def _ints(v):
    return (ct.c_int * len(v))(*v)


def _ptrs(*tensors):
    return (ct.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _plan(sides, chans, batch):
    n = len(sides)
    slices, tps = (ct.c_int * n)(), (ct.c_int * n)()
    assert raw("eg_conv1x1_relu_pack_bwd_plan", _ints(chans), _ints(sides), n, batch, slices, tps) == _lib.EG_OK
    return list(slices), list(tps)


def exact_fixture(sides, chans, batch, front, back, bias):
    """Inputs whose pre-activations are exact in float32: features integers in [-2, 2], weights in {-1, 0, 1}, biases integers in
    [-3, 2] plus 0.5, a standard normal upstream gradient; drawn from RandomState(0) in that order, per level as R.conv_fixture."""
    rs = np.random.RandomState(0)
    f32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.float32))
    feats = [f32(rs.randint(-2, 3, (batch, c, p, p))) for p, c in zip(sides, chans)]
    weights = [f32(rs.randint(-1, 2, (128, c))) for c in chans]
    drawn = [f32(rs.randint(-3, 3, 128) + 0.5) for _ in chans]
    biases = [b if bias == "all" or (bias == "mixed" and l % 2 == 0) else None for l, b in enumerate(drawn)]
    n_rows = front + sum(p * p for p in sides) + back
    return dict(feats=feats, weights=weights, biases=biases, batch=batch, n_rows=n_rows, row_offset=front, sides=list(sides),
                dnodes=f32(rs.standard_normal((batch * n_rows, 128))))


def _references(fx):
    r64 = R.conv_pack64(fx["feats"], fx["weights"], fx["biases"], fx["batch"], fx["n_rows"], fx["row_offset"], dnodes=fx["dnodes"])
    return r64, R.conv_torch32(fx)


_cache = {}


def _small(case, bias):
    """(fixture, float64 reference, float32 yardstick) of a small case, computed once and shared."""
    key = ("small", case, bias)
    if key not in _cache:
        fx = R.conv_fixture(*case, bias, CONV_SEEDS[(case, bias)])
        r64, r32 = _references(fx)
        same, ratio = R.relu_margin(r64["s"], r32["s"])
        assert same and ratio >= R.MARGIN, (case, bias, same, ratio)                       # before any kernel runs
        _cache[key] = (fx, r64, r32)
    return _cache[key]


def _exact(case, bias):
    key = ("exact", case, bias)
    if key not in _cache:
        fx = exact_fixture(*case, bias)
        r64, r32 = _references(fx)
        for s64, s32 in zip(r64["s"], r32["s"]):                                           # before any kernel runs
            assert torch.equal(s32.double(), s64), (case, bias)
        _cache[key] = (fx, r64, r32)
    return _cache[key]


def _leaves(fx, grad=(True, True, True), view=None):
    view = view or (lambda t: t.clone())
    mk = lambda t, g: None if t is None else view(t.to(DEV)).requires_grad_(g)
    return ([mk(t, grad[0]) for t in fx["feats"]], [mk(t, grad[1]) for t in fx["weights"]], [mk(t, grad[2]) for t in fx["biases"]])


def _run(fx, backward="hip", grad=(True, True, True), view=None):
    """Forward + backward on fresh tensors -> (node rows, dfeat, dw, db) with None where no gradient is wanted."""
    feats, ws, bs = _leaves(fx, grad, view)
    got = ops.conv1x1_relu_pack_levels(feats, ws, bs, fx["batch"], fx["n_rows"], fx["row_offset"], backward=backward)
    ins = [t for t in feats + ws + bs if t is not None and t.requires_grad]
    g = (view or (lambda t: t))(fx["dnodes"].to(DEV))
    grads = iter(torch.autograd.grad(got, ins, g)) if ins else iter(())
    take = lambda ts: [next(grads) if t is not None and t.requires_grad else None for t in ts]
    return got.detach(), take(feats), take(ws), take(bs)


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def _check_all(rep, fx, r64, r32, res):
    out, df, dw, db = res
    rep.check("node rows", out, r64["out"], r32["out"], r64["scale"])
    for l in range(len(fx["sides"])):
        assert df[l].shape == fx["feats"][l].shape and dw[l].shape == fx["weights"][l].shape
        rep.check("d features", df[l], r64["dfeat"][l], r32["dfeat"][l], r64["dfeat_scale"][l])
        rep.check("d weight", dw[l], r64["dw"][l], r32["dw"][l], r64["dw_scale"][l])
        if fx["biases"][l] is not None:
            rep.check("d bias", db[l], r64["db"][l], r32["db"][l], r64["db_scale"][l])
        else:
            assert db[l] is None


def _finish(rep, capsys, title):
    with capsys.disabled():
        print(rep.table(title))
    assert not rep.failed(), rep.failed()


# ---------------------------------------------------------------------------
# 1. small cases, random normal inputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bias", R.BIAS_MODES)
@pytest.mark.parametrize("case", R.CONV_CASES, ids=_ids)
def test_small_cases_against_float64(case, bias, capsys):
    """1, 31, 32, 33, 64 and 512 channels, sides 1 .. 17, the 16-byte and the element-wise route, biases present, absent and mixed."""
    fx, r64, r32 = _small(case, bias)
    rep = Report()
    _check_all(rep, fx, r64, r32, _run(fx))
    _finish(rep, capsys, f"tail backward {case}, biases {bias}")


# ---------------------------------------------------------------------------
# 2. multi-slice cases with exact pre-activations
# ---------------------------------------------------------------------------
def test_the_exact_cases_reach_both_routes_and_a_short_last_slice():
    tiles = lambda case: [case[2] * -(-p * p // 64) for p in case[0]]
    levels = [(n, s, t) for case, (slices, tps) in EXACT_CASES.items() for n, s, t in zip(tiles(case), slices, tps)]
    assert any(t == 1 and s > 1 for _, s, t in levels) and any(t > 1 for _, s, t in levels)
    assert any(t > 1 and n % t for n, s, t in levels)                                     # a short last slice


@pytest.mark.parametrize("bias", R.BIAS_MODES)
@pytest.mark.parametrize("case", list(EXACT_CASES), ids=_ids)
def test_multi_slice_cases_against_float64(case, bias, capsys):
    fx, r64, r32 = _exact(case, bias)
    assert _plan(case[0], case[1], case[2]) == EXACT_CASES[case]                          # the route the case is there for
    if bias == "none":
        zero = sum(int((s == 0).sum()) for s in r64["s"]) / sum(s.numel() for s in r64["s"])
        assert zero > 0.01, zero                                                          # the tie case: pre-activations of exactly 0
    rep = Report()
    _check_all(rep, fx, r64, r32, _run(fx))
    _finish(rep, capsys, f"tail backward, exact pre-activations {case}, biases {bias}")


# ---------------------------------------------------------------------------
# 3. bits: two calls, and a captured graph
# ---------------------------------------------------------------------------
BITS = [("small", R.CONV_CASES[0], "mixed"), ("exact", ((3, 12), (40, 256), 7, 1, 1), "all"), ("exact", ((4, 72), (16, 4), 2, 0, 0), "none")]


def _fixture(family, case, bias):
    return (_small if family == "small" else _exact)(case, bias)[0]


@pytest.mark.parametrize("family,case,bias", BITS, ids=lambda v: _ids(v) if isinstance(v, tuple) else v)
def test_two_calls_give_the_same_bits(family, case, bias):
    fx = _fixture(family, case, bias)
    a, b = _run(fx), _run(fx)
    assert torch.equal(a[0], b[0]) and all(_same(x, y) for x, y in zip(a[1:], b[1:]))


@pytest.mark.parametrize("family,case,bias", BITS, ids=lambda v: _ids(v) if isinstance(v, tuple) else v)
def test_a_captured_graph_replays_the_eager_bits(family, case, bias):
    fx = _fixture(family, case, bias)
    eager = _run(fx)                                                                      # also the warm-up: scratch, library load
    feats, ws, bs = _leaves(fx)
    ins = feats + ws + [b for b in bs if b is not None]
    g = fx["dnodes"].to(DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):                                                       # the scratch cache is per stream: warm it here
        torch.autograd.grad(ops.conv1x1_relu_pack_levels(feats, ws, bs, fx["batch"], fx["n_rows"], fx["row_offset"], backward="hip"), ins, g)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = ops.conv1x1_relu_pack_levels(feats, ws, bs, fx["batch"], fx["n_rows"], fx["row_offset"], backward="hip")
        grads = torch.autograd.grad(out, ins, g)
    want = [t for t in eager[1] + eager[2] + eager[3] if t is not None]
    for _ in range(2):
        for t in grads:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.detach(), eager[0]) and len(grads) == len(want) and all(torch.equal(a, b) for a, b in zip(grads, want))


# ---------------------------------------------------------------------------
# 4. selective outputs, views at odd offsets, the raw entry point's refusals
# ---------------------------------------------------------------------------
def test_selective_outputs_keep_the_bits():
    fx = _exact(((3, 12), (40, 256), 7, 1, 1), "mixed")[0]
    full = _run(fx)
    no_f = _run(fx, grad=(False, True, True))
    assert all(t is None for t in no_f[1]) and _same(no_f[2], full[2]) and _same(no_f[3], full[3])
    only_f = _run(fx, grad=(True, False, False))
    assert _same(only_f[1], full[1]) and all(t is None for t in only_f[2] + only_f[3])
    only_b = _run(fx, grad=(False, False, True))                                          # the bias of level 0 alone
    assert _same(only_b[3], full[3]) and full[3][1] is None and full[3][0] is not None
    frozen = _run(fx, grad=(False, False, False))
    assert torch.equal(frozen[0], full[0]) and all(t is None for t in frozen[1] + frozen[2] + frozen[3])


def test_a_call_that_wants_nothing_launches_nothing():
    """Raw: every output NULL (as arrays of NULLs and as NULL arrays), no features, no weights, no workspace: EG_OK.  Through the
    wrapper with everything frozen the output has no autograd node at all."""
    d = torch.zeros(16, 128, device=DEV)
    none = _ptrs(None)
    assert raw("eg_conv1x1_relu_pack_bwd", d, d, none, none, _ints([8]), _ints([4]), 1, 1, 16, 0, None, none, none, none) == _lib.EG_OK
    assert raw("eg_conv1x1_relu_pack_bwd", d, d, None, None, _ints([8]), _ints([4]), 1, 1, 16, 0, None, None, None, None) == _lib.EG_OK
    torch.cuda.synchronize()
    fx = _small(R.CONV_CASES[0], "all")[0]
    feats, ws, bs = _leaves(fx, grad=(False, False, False))
    out = ops.conv1x1_relu_pack_levels(feats, ws, bs, fx["batch"], fx["n_rows"], fx["row_offset"], backward="hip")
    assert out.grad_fn is None and not out.requires_grad


def _odd_view(t):
    """A contiguous view of t's values that starts one element into a buffer: 4 bytes past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:] = t.reshape(-1)
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def test_wrapper_takes_views_at_odd_offsets():
    """Even-side features and a d_nodes 4 bytes past a 16-byte boundary: the wrapper copies them, the bits are those of aligned clones."""
    fx = _exact(((4, 72), (16, 4), 2, 0, 0), "all")[0]
    a, b = _run(fx), _run(fx, view=_odd_view)
    assert torch.equal(a[0], b[0]) and all(_same(x, y) for x, y in zip(a[1:], b[1:]))
    assert float(a[1][1].abs().max()) > 0 and float(a[2][1].abs().max()) > 0


def test_raw_entry_point_refuses_unaligned_16_byte_operands():
    rs = np.random.RandomState(9)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(DEV)
    feat, w, dn = t(1, 8, 4, 4), t(128, 8), t(16, 128)
    nodes = torch.relu(t(16, 128))
    nbytes = int(raw("eg_conv1x1_relu_pack_bwd_workspace_bytes", _ints([8]), _ints([4]), 1, 1))
    assert nbytes == 4 * 1 * 128 * 9
    ws = torch.full((nbytes,), 7, dtype=torch.uint8, device=DEV)
    mark = lambda *s: torch.full(s, 7.0, device=DEV)
    df, dw, db = mark(1, 8, 4, 4), mark(128, 8), mark(128)

    def bwd(d_nodes=dn, y=nodes, f=feat, d_f=df, side=4):
        return raw("eg_conv1x1_relu_pack_bwd", d_nodes, y, _ptrs(f), _ptrs(w), _ints([8]), _ints([side]), 1, 1, 16, 0, ws, _ptrs(d_f), _ptrs(dw), _ptrs(db))

    for kw in (dict(d_nodes=_odd_view(dn)), dict(y=_odd_view(nodes)), dict(f=_odd_view(feat)), dict(d_f=_odd_view(df))):
        assert bwd(**kw) == _lib.EG_ERR_ARG, list(kw)
        assert "16-byte" in _lib.last_error()
    torch.cuda.synchronize()
    assert all(bool((x == 7).all()) for x in (df, dw, db, ws))                             # nothing was launched
    # the element-wise route (odd side) takes any float address for the features and dF
    feat3 = t(1, 8, 3, 3)
    df3a, df3b = _odd_view(mark(1, 8, 3, 3)), mark(1, 8, 3, 3)
    dwa, dba = mark(128, 8), mark(128)
    assert raw("eg_conv1x1_relu_pack_bwd", dn, nodes, _ptrs(_odd_view(feat3)), _ptrs(w), _ints([8]), _ints([3]), 1, 1, 16, 0, ws, _ptrs(df3a), _ptrs(dwa), _ptrs(dba)) == _lib.EG_OK
    assert bwd(f=feat3, d_f=df3b, side=3) == _lib.EG_OK
    assert torch.equal(df3a, df3b) and torch.equal(dwa, dw) and torch.equal(dba, db) and not bool((df3b == 7).any())


# ---------------------------------------------------------------------------
# 5. the default route is what it was
# ---------------------------------------------------------------------------
def test_backward_torch_is_the_direct_autograd_node():
    fx = _small(R.CONV_CASES[1], "mixed")[0]
    default = _run(fx, backward="torch")
    feats, ws, bs = _leaves(fx)
    got = P._ConvReluPackFn.apply(fx["batch"], fx["n_rows"], fx["row_offset"], len(feats), *feats, *ws, *bs)
    ins = feats + ws + [b for b in bs if b is not None]
    grads = list(torch.autograd.grad(got, ins, fx["dnodes"].to(DEV)))
    assert got.grad_fn.name().startswith("_ConvReluPackFn")
    assert torch.equal(got.detach(), default[0])
    n = len(feats)
    # the feature gradients and biases are sums in a fixed order; MIOpen's weight gradient may differ in the last bits between runs
    assert all(torch.equal(a, b) for a, b in zip(grads[:n], default[1]))
    for a, b in zip(grads[n:2 * n], default[2]):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    feats, ws, bs = _leaves(fx)
    plain = ops.conv1x1_relu_pack_levels(feats, ws, bs, fx["batch"], fx["n_rows"], fx["row_offset"])
    assert plain.grad_fn.name().startswith("_ConvReluPackFn") and torch.equal(plain.detach(), default[0])
    hip = ops.conv1x1_relu_pack_levels(feats, ws, bs, fx["batch"], fx["n_rows"], fx["row_offset"], backward="hip")
    assert hip.grad_fn.name().startswith("_ConvReluPackHipFn") and torch.equal(hip.detach(), default[0])
