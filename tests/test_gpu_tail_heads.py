"""-m gpu: eg_conv1x1_relu_heads_fwd (csrc/tail_heads.hip), the UNet tail and the four heads in one launch -- bit for bit against
the two launches it replaces (eg_conv1x1_relu_pack_levels, eg_classifier_fwd), against tests/nognn_reference.py in float64 under
coord_reference.Report's rule as tests/test_gpu_eval_fp64.py section c applies it, row coverage, frame independence and capture."""
import itertools

import pytest
import torch

import eval_reference as E
import nognn_reference as N
import train_reference as T
from coord_reference import Report
from echoglad_amd import ops
from echoglad_amd.ops._core import call
from echoglad_amd.ops.infer import _HEAD_KEYS
from echoglad_amd.ops.pack import _addresses, _ints

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
# (sides, channels, B): levels under one tile, a last tile of 16 and of 1 position, p^2 % 4 != 0 (the scalar-load path), channel
# counts below, at, one over and many times the 32-channel pass
CASES = [((2, 3, 8), (32, 31, 64), 2), ((1, 4, 17), (1, 33, 5), 1), ((6,), (512,), 2), ((2, 40), (64, 4), 3), ((3, 12), (40, 256), 3),
         ((2, 4, 8, 16), (512, 256, 128, 64), 1)]
DEFAULT = ((2, 4, 8, 16, 32, 64, 128, 224), (512, 256, 128, 64, 32, 16, 8, 4), 1)        # 1127 tiles: longer than the grid of 512
_ids = lambda c: "-".join(map(str, c[0])) + f"-b{c[2]}"


@pytest.fixture(scope="module")
def heads_sets():
    sets = (("oracle heads", E.pack_heads(T.oracle_heads())), ("uniform", E.uniform_heads(7)))
    return [(name, packed, {k: v.to(DEV) for k, v in packed.items()}) for name, packed in sets]


def _dev(ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _rows(sides):
    return sum(p * p for p in sides)


def _two_launches(feats, weights, biases, B, pg, sigmoid):
    n = _rows([f.shape[2] for f in feats])
    nodes = ops.conv1x1_relu_pack_levels(feats, weights, biases, B, n)
    return ops.classifier_fwd(nodes, B, n, 0, n, pg, sigmoid)


def _bits(case, heads_sets, seed):
    sides, chans, B = case
    for bias in (True, False):
        f, w, b = (_dev(t) for t in N.level_inputs(sides, chans, B, seed, bias))
        for (name, _, pg), sigmoid in itertools.product(heads_sets, (False, True)):
            got = ops.conv1x1_relu_heads(f, w, b, B, pg, sigmoid)
            want = _two_launches(f, w, b, B, pg, sigmoid)
            assert got.shape == want.shape == (B * _rows(sides), 4)
            assert torch.equal(got, want), (bias, name, sigmoid, float((got - want).abs().max()))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_one_launch_equals_the_two_launches_bit_for_bit(case, heads_sets):
    _bits(case, heads_sets, seed=3)


def test_one_launch_equals_the_two_launches_at_the_default_shape(heads_sets):
    _bits(DEFAULT, heads_sets[:1], seed=4)


def _scaled(feats, mags):
    return [f * torch.tensor(mags, dtype=F32).view(-1, 1, 1, 1) for f in feats]


@pytest.mark.parametrize("case", CASES[:3], ids=_ids)
def test_against_float64(case, heads_sets, capsys):
    """|kernel - fp64| <= 4 max|ref32 - fp64| + 8 ulp x scale per element, nothing left out; the second input set (frames scaled
    1e-3, 1, 30, 1e4) frame by frame, so that a large frame's float32 yardstick does not excuse a small one."""
    sides, chans, B = case
    n = _rows(sides)
    rep = Report()
    f1, w, b = N.level_inputs(sides, chans, B, seed=5)
    f2 = _scaled(N.level_inputs(sides, chans, len(E.MAGNITUDES), seed=6)[0], E.MAGNITUDES)
    for tag, feats, Bx, apart in (("", f1, B, False), ("magnitudes: ", f2, len(E.MAGNITUDES), True)):
        fg, wg, bg = _dev(feats), _dev(w), _dev(b)
        for (name, packed, pg), sigmoid in itertools.product(heads_sets, (False, True)):
            (r64, s64), (r32, _) = (N.tail_heads(feats, w, b, Bx, packed, sigmoid, dtype=dt) for dt in (F64, F32))
            got = ops.conv1x1_relu_heads(fg, wg, bg, Bx, pg, sigmoid).cpu()
            what = f"{tag}{'sigmoid' if sigmoid else 'logits'}, {name}"
            for rows in ([slice(k * n, (k + 1) * n) for k in range(Bx)] if apart else [slice(None)]):
                rep.check(what, got[rows], r64[rows], r32[rows], s64[rows])
    with capsys.disabled():
        print(rep.table(f"tail + heads {case}"))
    assert not rep.failed(), rep.failed()


def _raw(feats, weights, biases, B, pg, sigmoid, out):
    chans, sides = [f.shape[1] for f in feats], [f.shape[2] for f in feats]
    call("eg_conv1x1_relu_heads_fwd", _addresses(feats), _addresses(weights), _addresses(biases), _ints(chans), _ints(sides), len(feats), B,
         *[pg[k] for k in _HEAD_KEYS], sigmoid, out)
    return out


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_every_row_is_written_and_a_frame_does_not_depend_on_its_neighbours(case, heads_sets):
    sides, chans, _ = case
    B, n, pg = 3, _rows(sides), heads_sets[0][2]
    f, w, b = (_dev(t) for t in N.level_inputs(sides, chans, B, seed=7))
    out = _raw(f, w, b, B, pg, False, torch.full((B * n, 4), float("nan"), device=DEV))
    assert out.shape == (B * n, 4) and bool(torch.isfinite(out).all())
    assert torch.equal(out, ops.conv1x1_relu_heads(f, w, b, B, pg))
    alone = ops.conv1x1_relu_heads([t[1:2].contiguous() for t in f], w, b, 1, pg)
    assert torch.equal(out.view(B, n, 4)[1], alone)


def test_captured_launch_replays_equal_eager(heads_sets):
    sides, chans, B = CASES[0]
    pg = heads_sets[0][2]
    f, w, b = (_dev(t) for t in N.level_inputs(sides, chans, B, seed=8))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.conv1x1_relu_heads(f, w, b, B, pg, True)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = ops.conv1x1_relu_heads(f, w, b, B, pg, True)
    for k in range(3):
        for t, new in zip(f, N.level_inputs(sides, chans, B, seed=20 + k)[0]):
            t.copy_(new)
        graph.replay()
        assert torch.equal(out, ops.conv1x1_relu_heads(f, w, b, B, pg, True)), k
