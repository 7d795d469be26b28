"""The reference of tests/test_gpu_pool_pack_fp64.py (tests/pool_reference.py) against torch's own operators on the CPU in float64,
the host arithmetic behind csrc/pool.hip's window tables, and the route plan of the cases the GPU tests are named for.  No GPU."""
import numpy as np
import pytest
import torch

import pool_reference as R

F64 = torch.float64
BIG = [(F, p) for F in (224, 257, 511, 512) for p in (1, 2, 3, F // 2, F // 2 + 1, F - 1, F)]


def _matrix_is_torch(F, p, rs):
    x = torch.from_numpy(rs.standard_normal((2, F, F))).requires_grad_(True)
    want = torch.nn.functional.adaptive_avg_pool2d(x, (p, p))
    got, = R.pool_fwd(x, [p])
    scale, = R.pool_fwd_scale(x, [p])
    assert float(((got - want.detach()).abs() / scale).max()) <= 2.0 ** -44, (F, p)
    g = torch.from_numpy(rs.standard_normal((2, p, p)))
    want_dx, = torch.autograd.grad(want, x, g)
    got_dx = R.pool_bwd([g], None, [p], x.shape)
    assert float(((got_dx - want_dx).abs() / R.pool_bwd_scale([g], None, [p], x.shape).clamp_min(1e-300)).max()) <= 2.0 ** -44, (F, p)


def test_matrix_forward_and_backward_are_adaptive_avg_pool2d_up_to_64():
    rs = np.random.RandomState(0)
    for F in range(1, 65):
        for p in range(1, F + 1):
            _matrix_is_torch(F, p, rs)


@pytest.mark.parametrize("F,p", BIG)
def test_matrix_forward_and_backward_are_adaptive_avg_pool2d_large(F, p):
    _matrix_is_torch(F, p, np.random.RandomState(F + p))


def test_matrix_rows_sum_to_one_and_frame_gradient_is_added():
    m = R.pool_matrix(29, 7)
    assert torch.equal(m.sum(1), torch.ones(7, dtype=F64)) or float((m.sum(1) - 1).abs().max()) < 1e-15
    gf = torch.arange(9.0, dtype=F64).view(1, 3, 3)
    assert torch.equal(R.pool_bwd([None, None], gf, [1, 2], (1, 3, 3)), gf)
    g = torch.ones(1, 1, 1, dtype=F64)
    assert torch.equal(R.pool_bwd([g, None], gf, [1, 2], (1, 3, 3)), gf + 1.0 / 9)


def test_no_pixel_lies_in_more_than_two_windows_and_the_float32_guess_covers_them():
    """Host arithmetic only: for all 1 <= p <= F <= 512 the windows that contain index r are floor(r p / F) .. ceil((r + 1) p / F) - 1,
    at most two, and windows_of's float32 guess i0 = int(float(r) * float(p) / float(F)) (IEEE float32) is within one of each.  What
    the device's own arithmetic does is the GPU sweep's business."""
    f32 = np.float32
    uncovered = 0
    for F in range(1, 513):
        r = np.arange(F, dtype=np.int64)[None, :]
        p = np.arange(1, F + 1, dtype=np.int64)[:, None]
        lo = r * p // F                               # smallest i with r < ceil((i + 1) F / p)
        hi = -((-(r + 1) * p) // F) - 1               # largest i with floor(i F / p) <= r
        assert (lo <= hi).all() and (hi - lo <= 1).all() and (hi < p).all(), F
        i0 = (r.astype(f32) * p.astype(f32) / f32(F)).astype(np.int64)
        uncovered += int(((lo < i0 - 1) | (hi > i0 + 1)).sum())
    assert uncovered == 0
    # the closed form above is the definition: spot-check it against the windows themselves
    for F, p in ((7, 5), (29, 28), (257, 129), (512, 341)):
        for r in range(F):
            inside = [i for i in range(p) if R.window(F, p, i)[0] <= r < R.window(F, p, i)[1]]
            assert inside == list(range(r * p // F, -((-(r + 1) * p) // F))), (F, p, r)


def _d(p, src, kept):
    return (p, "derived", src, kept)


PLANS = {
    (184, (23, 46, 92, 184)): [(184, "direct"), _d(92, "global", False), _d(46, "global", True), _d(23, "lds", False)],
    (256, (32, 64, 128, 256)): [(256, "direct"), _d(128, "global", False), _d(64, "global", True), _d(32, "lds", False)],
    (512, (64, 128, 256)): [(256, "direct"), _d(128, "global", False), _d(64, "global", False)],
    (24, (1, 2, 3, 5, 6, 12, 24)): [(24, "direct"), _d(12, "global", True), _d(6, "lds", False), (5, "direct"), (3, "direct"), (2, "direct"),
                                    _d(1, "global", False)],
    (40, (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 20, 24, 32, 40)):
        [(p, "direct") for p in (40, 32, 24, 20, 16, 12, 10, 9, 8, 7, 6, 5, 4, 3, 2)] + [_d(1, "global", False)],
    (224, (2, 4, 8, 16, 32, 64, 128)): [(128, "direct"), (64, "direct"), (32, "direct"), _d(16, "global", True), _d(8, "lds", True),
                                        _d(4, "lds", True), _d(2, "lds", False)],
}


@pytest.mark.parametrize("case", list(PLANS), ids=lambda c: f"F{c[0]}x{len(c[1])}")
def test_plan_of_the_named_cases(case):
    assert R.plan(case[0], list(case[1])) == PLANS[case]


def test_pack_rows_and_its_inverse():
    rs = np.random.RandomState(1)
    sides, batch, front, back = [1, 3, 4], 2, 2, 3
    maps = [torch.from_numpy(rs.standard_normal((batch, 128, p, p))) for p in sides]
    n_rows = front + sum(p * p for p in sides) + back
    nodes = R.pack_rows(maps, batch, n_rows, front)
    v = nodes.view(batch, n_rows, 128)
    assert float(v[:, :front].abs().max()) == 0 and float(v[:, n_rows - back:].abs().max()) == 0
    assert float(v[1, front + 1 + 3 * 1 + 2, 77]) == float(maps[1][1, 77, 1, 2])          # level 1, pixel (1, 2), channel 77
    for a, b in zip(R.unpack_rows(nodes, sides, batch, n_rows, front), maps):
        assert torch.equal(a, b)


def test_conv_pack64_is_relu_conv2d_and_its_autograd():
    rs = np.random.RandomState(2)
    sides, chans, batch = [2, 3], [5, 33], 2
    mk = lambda *s: torch.from_numpy(rs.standard_normal(s)).requires_grad_(True)
    feats = [mk(batch, c, p, p) for p, c in zip(sides, chans)]
    ws = [mk(128, c) for c in chans]
    bs = [mk(128), None]
    n_rows = 1 + 4 + 9
    g = torch.from_numpy(rs.standard_normal((batch * n_rows, 128)))
    r = R.conv_pack64(feats, ws, bs, batch, n_rows, 1, dnodes=g)
    maps = [torch.relu(torch.nn.functional.conv2d(f, w.view(128, -1, 1, 1), b)) for f, w, b in zip(feats, ws, bs)]
    want = R.pack_rows(maps, batch, n_rows, 1)
    assert float((r["out"] - want.detach()).abs().max()) < 1e-12
    assert bool((r["scale"] >= r["out"].abs() - 1e-12).all())
    grads = torch.autograd.grad(want, feats + ws + [bs[0]], g)
    for a, b in zip(r["dfeat"] + r["dw"] + [r["db"][0]], grads):
        assert float((a - b).abs().max()) < 1e-11
    assert r["db"][1] is None and r["db_scale"][1] is None
    same, ratio = R.relu_margin(r["s"], [t.float() for t in r["s"]])
    assert same and ratio > 64
