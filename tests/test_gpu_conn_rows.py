"""-m gpu: the connection rows' fixed-order means (csrc/conn_rows.hip) from the kernel up to the models.

Forward, against float64 column means, under a bound that is derived and not measured: with u = 2^-24, gamma_k = k u / (1 - k u)
and d(rows) the documented longest chain of additions (ops.conn_rows_chain), a mean over `rows` rows misses the exact one by at most
gamma_{d+1} * sum_i |x_ic| / rows (d additions and one division).  The kernel tests also assert that this bound lies below
0.25 min|x| / rows at every shape they use, so a lost or doubled row cannot hide inside it -- and compare with a numpy float32
restatement of the documented order bit for bit, as they do for the backward (the documented operation order).

Gradients, through ops and the models: the rule of coord_reference.Report.check (tests/test_gpu_tail_bwd.py),
|kernel - fp64| <= 4 max|ref32 - fp64| + 8 ulp x scale, where ref32 is the route the switch replaces -- the packing and
connection_embed from torch's mean, float32 on the CPU -- and scale the per-output sum of the summands' magnitudes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_reference as R
from coord_reference import Report
from fixtures_util import fill_state_dict
from gpu_util import DEV, graph_tensors, model_pair
from echoglad_amd import data, engine, losses, ops
from echoglad_amd.examples import UNetNodeFeatureModel
from echoglad_amd.nn import CNN, CNNHierarchicalPatchModel
from echoglad_amd.ops import pack as P
from echoglad_amd.synthetic import initial_coords, synthetic_frames

pytestmark = pytest.mark.gpu
C = 128
U = 2.0 ** -24
F64 = torch.float64


def gamma(k):
    return k * U / (1 - k * U)


# ---------------------------------------------------------------------------
# the documented orders, restated in numpy float32
# ---------------------------------------------------------------------------
def np_mean(x):
    """The forward's order on one source x [rows, 128] float32: per chunk, row lane h adds rows h, h + 8, .. ascending to 0, the 8
    lane sums ascending; the chunk sums ascending; one division by float32(rows)."""
    rows = x.shape[0]
    chunks, rpc = ops.conn_rows_plan(rows)
    parts = []
    for k in range(chunks):
        c = x[k * rpc:(k + 1) * rpc]
        pad = np.zeros((-(-c.shape[0] // 8) * 8, C), np.float32)
        pad[:c.shape[0]] = c                                     # (+ 0.0f is exact: a lane that has run out of rows)
        lanes = np.zeros((8, C), np.float32)
        for s in pad.reshape(-1, 8, C):
            lanes = lanes + s
        tot = lanes[0]
        for h in range(1, 8):
            tot = tot + lanes[h]
        parts.append(tot)
    tot = parts[0]
    for p in parts[1:]:
        tot = tot + p
    return tot / np.float32(rows)


def np_bwd(d, batch, n_rows, base, rows):
    """The backward's order on d [batch * n_rows, 128] float32: per distinct source, t = the products d[b, j] * (float32(1) /
    float32(rows_j)) of the rows j that name it, j ascending, the first one starting the sum; then one add per row of the source."""
    src = d.reshape(batch, n_rows, C)
    out = src.copy()
    done = set()
    for j0, key in enumerate(zip(base, rows)):
        if key in done:
            continue
        done.add(key)
        t = None
        for j in range(j0, len(base)):
            if (base[j], rows[j]) == key:
                pr = src[:, j] * (np.float32(1) / np.float32(rows[j]))
                t = pr if t is None else t + pr
        out[:, key[0]:key[0] + key[1]] = src[:, key[0]:key[0] + key[1]] + t[:, None, :]
    return out.reshape(batch * n_rows, C)


# ---------------------------------------------------------------------------
# 1. the kernels on free level tables
# ---------------------------------------------------------------------------
RPC = 128                                                        # asserted against the plan below
POOL = [1, 4, 63, 64, 65, 400, 4097, RPC - 1, RPC, RPC + 1, 2 * RPC + 1]
# (batch, the rows of every connection row's source; ("same", j): the source of row j once more)
TABLES = {
    "n1-b1": (1, [4097]),
    "n1-b3": (3, [RPC + 1]),
    "n4-b1": (1, [1, 63, RPC, 2 * RPC + 1]),
    "n4-b3": (3, [4, 64, RPC - 1, 400]),
    "n4-b3-repeated": (3, [2 * RPC + 1, 65, ("same", 0), ("same", 0)]),
    "n8-b3": (3, [1, 4, 63, 64, 65, 400, 4097, RPC + 1]),
    "n8-b1-repeated": (1, [65, RPC - 1, RPC, ("same", 1), 2 * RPC + 1, 400, ("same", 4), 1]),
}


def _table(spec):
    """(src_base, src_rows, n_rows): the distinct sources in order behind the connection rows, gaps of 3, 4, .. rows no range covers
    in front of each, 5 trailing rows."""
    n = len(spec)
    base, rows, at = [], [], n
    for i, s in enumerate(spec):
        if isinstance(s, tuple):
            base.append(base[s[1]])
            rows.append(rows[s[1]])
        else:
            at += 3 + i
            base.append(at)
            rows.append(s)
            at += s
    return base, rows, at + 5


_fixtures = {}


def _fixture(name):
    """(batch, n_rows, base, rows, x float32 CPU [batch * n_rows, 128], the kernel's result on the CPU), computed once."""
    if name not in _fixtures:
        assert ops.conn_rows_plan(1)[1] == RPC
        batch, spec = TABLES[name]
        base, rows, n_rows = _table(spec)
        rs = np.random.RandomState(len(name) + 7 * batch)
        x = (rs.uniform(0.5, 1.5, (batch * n_rows, C)) * rs.choice([-1.0, 1.0], (batch * n_rows, C))).astype(np.float32)
        x = torch.from_numpy(x)
        got = ops.conn_rows_fwd(x.to(DEV), batch, n_rows, base, rows).cpu()
        _fixtures[name] = (batch, n_rows, base, rows, x, got)
    return _fixtures[name]


def test_the_tables_draw_every_size_of_the_pool():
    used = {s for _, spec in TABLES.values() for s in spec if not isinstance(s, tuple)}
    assert used == set(POOL)
    assert {len(spec) for _, spec in TABLES.values()} == {1, 4, 8} and {b for b, _ in TABLES.values()} == {1, 3}


@pytest.mark.parametrize("name", list(TABLES))
def test_forward_against_float64_means(name):
    batch, n_rows, base, rows, x, got = _fixture(name)
    n = len(base)
    xv, gv = x.view(batch, n_rows, C), got.view(batch, n_rows, C)
    assert torch.equal(gv[:, n:], xv[:, n:])                                               # rows >= n_conn: only read
    worst = 0.0
    for j in range(n):
        d = ops.conn_rows_chain(rows[j])
        assert (d + 1) * rows[j] < 2.8e6
        src = xv[:, base[j]:base[j] + rows[j]].to(F64)
        bound = gamma(d + 1) * src.abs().sum(dim=1) / rows[j]
        assert float(bound.max()) < 0.25 * float(src.abs().min()) / rows[j]                # a lost or doubled row cannot hide
        err = (gv[:, j].to(F64) - src.mean(dim=1)).abs()
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (name, j, rows[j], float((err / bound).max()))
    print(f"{name}: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("name", list(TABLES))
def test_forward_is_the_documented_order_bit_for_bit(name):
    batch, n_rows, base, rows, x, got = _fixture(name)
    xv, gv = x.view(batch, n_rows, C).numpy(), got.view(batch, n_rows, C).numpy()
    for b in range(batch):
        for j in range(len(base)):
            want = np_mean(xv[b, base[j]:base[j] + rows[j]])
            assert np.array_equal(gv[b, j], want), (name, b, j, rows[j])
    for j in range(len(base)):                                                             # equal sources give equal bits
        for k in range(j):
            if (base[j], rows[j]) == (base[k], rows[k]):
                assert np.array_equal(gv[:, j], gv[:, k])


def test_forward_of_a_source_whose_chunks_grow_past_128_rows():
    """70,000 rows: 511 chunks of 137, the last one short.  (Outside the derived bound's reach, (d + 1) rows > 2.8e6: bits only.)"""
    rows, n_rows = 70000, 70010
    assert ops.conn_rows_plan(rows) == (511, 137)
    rs = np.random.RandomState(5)
    x = torch.from_numpy((rs.uniform(0.5, 1.5, (n_rows, C)) * rs.choice([-1.0, 1.0], (n_rows, C))).astype(np.float32))
    got = ops.conn_rows_fwd(x.to(DEV), 1, n_rows, [7, 7], [rows, rows]).cpu()
    assert torch.equal(got[2:], x[2:])
    want = np_mean(x[7:7 + rows].numpy())
    assert np.array_equal(got[0].numpy(), want) and np.array_equal(got[1].numpy(), want)


@pytest.mark.parametrize("name", ["n4-b3-repeated", "n8-b3"])
def test_a_frame_has_the_bits_it_has_alone_and_two_calls_agree(name):
    batch, n_rows, base, rows, x, got = _fixture(name)
    assert torch.equal(ops.conn_rows_fwd(x.to(DEV), batch, n_rows, base, rows).cpu(), got)
    for b in range(batch):
        alone = ops.conn_rows_fwd(x.view(batch, n_rows, C)[b].contiguous().to(DEV), 1, n_rows, base, rows).cpu()
        assert torch.equal(alone, got.view(batch, n_rows, C)[b]), b


def _captured(fn, buf, contents):
    """fn(buf) captured once (after a warm-up outside the capture), replayed on every tensor of `contents` written into buf."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        buf.copy_(contents[0])
        fn(buf)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn(buf)
    outs = []
    for t in contents:
        buf.copy_(t)
        g.replay()
        outs.append(buf.clone())
    return outs


def test_a_captured_forward_and_backward_replay_on_new_contents():
    batch, n_rows, base, rows, x, got = _fixture("n8-b1-repeated")
    y = torch.flip(x, dims=[0]).contiguous()
    for fn in (ops.conn_rows_fwd, ops.conn_rows_bwd):
        eager = [fn(t.to(DEV), batch, n_rows, base, rows) for t in (x, y)]
        buf = torch.empty_like(eager[0])
        outs = _captured(lambda t: fn(t, batch, n_rows, base, rows), buf, [x.to(DEV), y.to(DEV)])
        assert torch.equal(outs[0], eager[0]) and torch.equal(outs[1], eager[1]) and not torch.equal(outs[0], outs[1])
    assert torch.equal(eager[0].cpu(), torch.from_numpy(np_bwd(x.numpy(), batch, n_rows, base, rows)))


@pytest.mark.parametrize("name", list(TABLES))
def test_backward_is_the_documented_order_bit_for_bit(name):
    batch, n_rows, base, rows, x, _ = _fixture(name)
    got = ops.conn_rows_bwd(x.to(DEV), batch, n_rows, base, rows).cpu()
    want = torch.from_numpy(np_bwd(x.numpy(), batch, n_rows, base, rows))
    assert torch.equal(got, want)
    covered = torch.zeros(n_rows, dtype=torch.bool)
    for b0, r in zip(base, rows):
        covered[b0:b0 + r] = True
    keep = ~covered
    assert int(keep.sum()) >= len(base) + 5                                                # connection rows, gaps, trailing rows
    assert torch.equal(got.view(batch, n_rows, C)[:, keep], x.view(batch, n_rows, C)[:, keep])
    assert not torch.equal(got.view(batch, n_rows, C)[:, covered], x.view(batch, n_rows, C)[:, covered])


# ---------------------------------------------------------------------------
# 2. ops: the three packing calls with conn_rows=
# ---------------------------------------------------------------------------
def _level_table(mode, level_rows):
    n = len(level_rows)
    base, at = [], n
    for r in level_rows:
        base.append(at)
        at += r
    return ([base[-1]] * n, [level_rows[-1]] * n) if mode == "frame" else (base, list(level_rows))


def _check_conn_rows(nodes, batch, n_rows, base, rows):
    """The connection rows of `nodes` against the float64 means of its own source rows, under the derived bound."""
    v = nodes.detach().cpu().view(batch, n_rows, C)
    for j in range(len(base)):
        src = v[:, base[j]:base[j] + rows[j]].to(F64)
        bound = gamma(ops.conn_rows_chain(rows[j]) + 1) * src.abs().sum(dim=1) / rows[j]
        err = (v[:, j].to(F64) - src.mean(dim=1)).abs()
        assert bool((err <= bound).all()), (j, rows[j], float(err.max()), float(bound.min()))


def _dprime(dnodes, batch, n_rows, base, rows):
    """float64: the node gradient with the connection rows' share added to their source rows."""
    d = dnodes.detach().to(F64).reshape(batch, n_rows, C).clone()
    src = dnodes.detach().to(F64).reshape(batch, n_rows, C)
    for j in range(len(base)):
        d[:, base[j]:base[j] + rows[j]] += src[:, j:j + 1] / rows[j]
    return d.reshape(batch * n_rows, C)


def _torch_route(maps_fn, leaves, mode, batch, n_rows, dnodes, dtype):
    """What the switch replaces, on the CPU in `dtype`: the reference's packing, connection_embed from torch's mean written over
    the first rows, torch's autograd -> (node rows, gradients of the leaves that are not None)."""
    leaves = [None if t is None else t.detach().cpu().to(dtype).requires_grad_(True) for t in leaves]
    maps = maps_fn(leaves)
    n = len(maps)
    packed = R.pack_rows(maps, batch, n_rows, n).view(batch, n_rows, C)
    means = [m.mean(dim=(2, 3)) for m in maps]
    conn = torch.stack(means if mode == "level" else [means[-1]] * n, dim=1)
    out = torch.cat([conn, packed[:, n:]], dim=1).reshape(batch * n_rows, C)
    grads = torch.autograd.grad(out, [t for t in leaves if t is not None], dnodes.to(dtype))
    return out.detach(), list(grads)


def _finish(rep, capsys, title):
    with capsys.disabled():
        print(rep.table(title))
    assert not rep.failed(), rep.failed()


PACK_CASES = [((2, 3, 8), 2, 2), ((1, 4, 17), 1, 0)]                # (sides, batch, trailing rows); row_offset = the levels


@pytest.mark.parametrize("mode", ["level", "frame"])
@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: "-".join(map(str, c[0])))
def test_pack_levels_with_conn_rows(case, mode, capsys):
    sides, batch, back = case
    n = len(sides)
    level_rows = [p * p for p in sides]
    n_rows = n + sum(level_rows) + back
    base, rows = _level_table(mode, level_rows)
    rs = np.random.RandomState(3)
    maps = [torch.from_numpy(rs.standard_normal((batch, C, p, p)).astype(np.float32)) for p in sides]
    dnodes = torch.from_numpy(rs.standard_normal((batch * n_rows, C)).astype(np.float32))
    leaves = [m.to(DEV).requires_grad_(True) for m in maps]
    got = ops.pack_levels(leaves, batch, n_rows, n, conn_rows=mode)
    plain = ops.pack_levels([m.to(DEV) for m in maps], batch, n_rows, n)
    assert torch.equal(got.detach().view(batch, n_rows, C)[:, n:], plain.view(batch, n_rows, C)[:, n:])
    _check_conn_rows(got, batch, n_rows, base, rows)
    out = torch.full((batch * n_rows, C), 7.0, device=DEV)
    with torch.no_grad():
        assert ops.pack_levels([m.to(DEV) for m in maps], batch, n_rows, n, out=out, conn_rows=mode) is out
    assert torch.equal(out, got.detach())
    g_dev = dnodes.to(DEV)
    grads = torch.autograd.grad(got, leaves, g_dev)
    assert torch.equal(g_dev.cpu(), dnodes)                                                # the caller's gradient tensor is not ours
    want = R.unpack_rows(_dprime(dnodes, batch, n_rows, base, rows), sides, batch, n_rows, n)
    scale = R.unpack_rows(_dprime(dnodes.abs(), batch, n_rows, base, rows), sides, batch, n_rows, n)
    _, ref32 = _torch_route(lambda ls: ls, maps, mode, batch, n_rows, dnodes, torch.float32)
    rep = Report()
    for l in range(n):
        rep.check(f"d map {sides[l]}", grads[l], want[l], ref32[l], scale[l])
    _finish(rep, capsys, f"pack_levels conn_rows={mode} {sides}")


@pytest.mark.parametrize("frame,sides,batch", [(12, (2, 4), 2), (9, (1, 2, 5), 1)])
def test_pyramid_pack_with_conn_rows(frame, sides, batch, capsys):
    mode, n = "frame", len(sides) + 1
    level_rows = [p * p for p in sides] + [frame * frame]
    n_rows = n + sum(level_rows) + 3
    base, rows = _level_table(mode, level_rows)
    x = synthetic_frames(batch, C, frame, 17)
    dnodes = torch.from_numpy(np.random.RandomState(4).standard_normal((batch * n_rows, C)).astype(np.float32))
    leaf = x.to(DEV).requires_grad_(True)
    got = ops.pyramid_pack(leaf, list(sides), batch, n_rows, n, conn_rows=mode)
    plain = ops.pyramid_pack(x.to(DEV), list(sides), batch, n_rows, n)
    assert torch.equal(got.detach().view(batch, n_rows, C)[:, n:], plain.view(batch, n_rows, C)[:, n:])
    _check_conn_rows(got, batch, n_rows, base, rows)
    out = torch.full((batch * n_rows, C), 7.0, device=DEV)
    with torch.no_grad():
        ops.pyramid_pack(x.to(DEV), list(sides), batch, n_rows, n, out=out, conn_rows=mode)
    assert torch.equal(out, got.detach())
    dx, = torch.autograd.grad(got, [leaf], dnodes.to(DEV))
    all_sides = list(sides) + [frame]
    g64 = R.unpack_rows(_dprime(dnodes, batch, n_rows, base, rows), all_sides, batch, n_rows, n)
    a64 = R.unpack_rows(_dprime(dnodes.abs(), batch, n_rows, base, rows), all_sides, batch, n_rows, n)
    want = R.pool_bwd(g64[:-1], g64[-1], list(sides), tuple(x.shape))
    scale = R.pool_bwd_scale(a64[:-1], a64[-1], list(sides), tuple(x.shape))
    maps_fn = lambda ls: [F.adaptive_avg_pool2d(ls[0], (p, p)) for p in sides] + [ls[0]]
    _, ref32 = _torch_route(maps_fn, [x], mode, batch, n_rows, dnodes, torch.float32)
    rep = Report()
    rep.check("d frame", dx, want, ref32[0], scale)
    _finish(rep, capsys, f"pyramid_pack conn_rows={mode} frame {frame} sides {sides}")


# (sides, chans, batch, front = the levels, back), bias mode, seed: the seeds of tests/test_gpu_tail_bwd.py's CONV_SEEDS for these
# sides and channels (features, weights and biases are drawn in front of the gradient, so the pre-activations are the same); the
# margin is asserted on the references before any kernel runs
CONV_CASES = [(((2, 3, 8), (32, 31, 64), 2, 3, 0), "mixed", 1), (((1, 4, 17), (1, 33, 5), 1, 3, 3), "all", 2)]


@pytest.mark.parametrize("backward", ["torch", "hip"])
@pytest.mark.parametrize("case,bias,seed", CONV_CASES, ids=lambda v: "-".join(map(str, v[0])) if isinstance(v, tuple) else str(v))
def test_conv1x1_relu_pack_levels_with_conn_rows(case, bias, seed, backward, capsys):
    mode = "level"
    fx = R.conv_fixture(*case, bias, seed)
    sides, batch, n_rows, n = fx["sides"], fx["batch"], fx["n_rows"], len(fx["sides"])
    assert fx["row_offset"] == n
    base, rows = _level_table(mode, [p * p for p in sides])
    dn = fx["dnodes"]
    r64 = R.conv_pack64(fx["feats"], fx["weights"], fx["biases"], batch, n_rows, n, dnodes=_dprime(dn, batch, n_rows, base, rows))
    a64 = R.conv_pack64(fx["feats"], fx["weights"], fx["biases"], batch, n_rows, n, dnodes=_dprime(dn.abs(), batch, n_rows, base, rows))
    same, ratio = R.relu_margin(r64["s"], R.conv_torch32(fx)["s"])
    assert same and ratio >= R.MARGIN, (same, ratio)                                       # the float32 mask is the float64 mask
    mk = lambda t: None if t is None else t.to(DEV).requires_grad_(True)
    feats, ws, bs = [mk(t) for t in fx["feats"]], [mk(t) for t in fx["weights"]], [mk(t) for t in fx["biases"]]
    got = ops.conv1x1_relu_pack_levels(feats, ws, bs, batch, n_rows, n, backward=backward, conn_rows=mode)
    with torch.no_grad():
        plain = ops.conv1x1_relu_pack_levels(feats, ws, bs, batch, n_rows, n)
        out = torch.full((batch * n_rows, C), 7.0, device=DEV)
        ops.conv1x1_relu_pack_levels(feats, ws, bs, batch, n_rows, n, out=out, conn_rows=mode)
    assert torch.equal(got.detach().view(batch, n_rows, C)[:, n:], plain.view(batch, n_rows, C)[:, n:])
    assert torch.equal(out, got.detach())
    _check_conn_rows(got, batch, n_rows, base, rows)
    ins = [t for t in feats + ws + bs if t is not None]
    grads = iter(torch.autograd.grad(got, ins, dn.to(DEV)))
    take = lambda ts: [next(grads) if t is not None else None for t in ts]
    df, dw, db = take(feats), take(ws), take(bs)

    def maps_fn(ls):
        f, w, b = ls[:n], ls[n:2 * n], ls[2 * n:]
        return [torch.relu(F.conv2d(fi, wi.view(C, -1, 1, 1), bi)) for fi, wi, bi in zip(f, w, b)]
    _, g32 = _torch_route(maps_fn, fx["feats"] + fx["weights"] + fx["biases"], mode, batch, n_rows, dn, torch.float32)
    g32 = iter(g32)
    f32, w32 = [next(g32) for _ in range(n)], [next(g32) for _ in range(n)]
    b32 = [None if b is None else next(g32) for b in fx["biases"]]
    rep = Report()
    for l in range(n):
        rep.check("d features", df[l], r64["dfeat"][l], f32[l], a64["dfeat_scale"][l])
        rep.check("d weight", dw[l], r64["dw"][l], w32[l], a64["dw_scale"][l])
        if fx["biases"][l] is not None:
            rep.check("d bias", db[l], r64["db"][l], b32[l], a64["db_scale"][l])
    _finish(rep, capsys, f"conv1x1_relu_pack_levels conn_rows={mode} backward={backward} {sides}")


def test_a_retained_or_hooked_gradient_is_not_modified(monkeypatch):
    """The add goes in place only into a buffer that is the node's alone: a gradient that a hook kept, and the one retain_grad()
    stores, keep their bits; the inputs' gradients are the same bits either way."""
    sides, batch = (2, 3, 8), 2
    n = len(sides)
    n_rows = n + sum(p * p for p in sides) + 2
    rs = np.random.RandomState(8)
    maps = [torch.from_numpy(rs.standard_normal((batch, C, p, p)).astype(np.float32)).to(DEV) for p in sides]
    w = torch.from_numpy(rs.standard_normal((batch * n_rows, C)).astype(np.float32)).to(DEV)
    verdicts = []
    inner = P._grad_is_ours
    monkeypatch.setattr(P, "_grad_is_ours", lambda g, counts: verdicts.append(inner(g, counts)) or verdicts[-1])

    def run(hook, retain, mode="level"):
        leaves = [m.clone().requires_grad_(True) for m in maps]
        nodes = ops.pack_levels(leaves, batch, n_rows, n, conn_rows=mode)
        kept = []
        if hook:
            nodes.register_hook(lambda g: kept.append(g))
        if retain:
            nodes.retain_grad()
        (nodes * w).sum().backward()
        return [l.grad for l in leaves], kept, nodes.grad if retain else None

    plain, _, _ = run(False, False)
    assert verdicts == [True]                                                              # a fresh buffer of the multiply's backward: in place
    hooked, kept, _ = run(True, False)
    assert verdicts == [True, False] and len(kept) == 1 and torch.equal(kept[0], w)        # the hook's tensor: a copy took the add
    retained, _, grad = run(False, True)
    assert torch.equal(grad, w)
    both, kept, grad = run(True, True)
    assert torch.equal(grad, w) and torch.equal(kept[0], w)
    for other in (hooked, retained, both):
        assert all(torch.equal(a, b) for a, b in zip(plain, other))
    without, _, _ = run(False, False, mode=None)
    assert not any(torch.equal(a, b) for a, b in zip(plain, without))                      # the connection rows' share did arrive


# ---------------------------------------------------------------------------
# 3. the models
# ---------------------------------------------------------------------------
NAUX, BATCH = 3, 2
UNET_KW = dict(encoder_embedding_widths=[8, 4, 2], encoder_embedding_dims=[8, 16, 32])
MODEL_KW = dict(num_aux_graphs=NAUX, node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32, num_gnn_layers=2,
                output_activation="logit", use_connection_nodes=True)


def _model(kind, frame, coord):
    if kind == "base":
        return model_pair(frame, NAUX, 2, coord=coord, seed=5, use_connection_nodes=True)[0], C, "frame"
    kw = dict(MODEL_KW, frame_size=frame, use_coordinate_graph=coord)
    m = CNNHierarchicalPatchModel(cnn_layers_out_width=[8, 4, 2], **kw) if kind == "cnn" else UNetNodeFeatureModel(**UNET_KW, **kw)
    fill_state_dict(m, 9)
    m = m.to(DEV).eval()
    # the maps in front of the packing from the HIP front-ends: torch's convolutions do not repeat their bits from call to call
    m = m.enable_hip_pyramid() if kind == "cnn" else m.enable_hip_frontend(True)
    return m, (C if kind == "cnn" else 4), "level"


@pytest.mark.parametrize("coord", [False, True], ids=["plain", "coord"])
@pytest.mark.parametrize("frame", [16, 20])
@pytest.mark.parametrize("kind", ["base", "cnn", "unet"])
def test_create_node_pixels_behind_the_switch(kind, frame, coord):
    m, chans, mode = _model(kind, frame, coord)
    x = synthetic_frames(BATCH, chans, frame, 23).to(DEV)
    nc = initial_coords(BATCH, frame).to(DEV).reshape(BATCH, 4, 2) if coord else None
    n_rows, n_conn = m._row_ranges()[:2]
    assert n_conn == NAUX + 1
    with torch.no_grad():
        off = m.create_node_pixels(x, BATCH, nc)
        on = m.enable_hip_conn_rows().create_node_pixels(x, BATCH, nc)
        again = m.enable_hip_conn_rows(False).create_node_pixels(x, BATCH, nc)
    assert torch.equal(again, off)
    assert torch.equal(on.view(BATCH, n_rows, C)[:, n_conn:], off.view(BATCH, n_rows, C)[:, n_conn:])
    base, rows = _level_table(mode, [4 ** g for g in range(1, NAUX + 1)] + [frame * frame])
    _check_conn_rows(on, BATCH, n_rows, base, rows)
    assert not torch.equal(on.view(BATCH, n_rows, C)[:, :n_conn], torch.zeros_like(on.view(BATCH, n_rows, C)[:, :n_conn]))
    # and the route it replaces is within float32 rounding of it (both are float32 sums of the same numbers)
    diff = (on - off).view(BATCH, n_rows, C)[:, :n_conn].abs().max()
    assert float(diff) <= 1e-5 * float(off.view(BATCH, n_rows, C)[:, n_conn:].abs().max())


@pytest.mark.parametrize("coord", [False, True], ids=["plain", "coord"])
@pytest.mark.parametrize("frame", [16, 20])
def test_eval_logits_of_the_base_model_against_the_float64_oracle(frame, coord):
    """|switch on - fp64| <= 4 max|switch off - fp64| + 8 ulp x max|fp64|: both are float32 evaluations of the oracle's forward."""
    hip, ref = model_pair(frame, NAUX, 2, coord=coord, seed=5, use_connection_nodes=True)
    topo, ei, nt, bi = graph_tensors(frame, NAUX, BATCH, coord=coord, conn=True)
    x = synthetic_frames(BATCH, C, frame, 29)
    c0 = initial_coords(BATCH, frame) if coord else None
    with torch.no_grad():
        want = ref.double()(x=x.double(), edge_index=ei, node_type=nt, batch_idx=bi, node_coords=None if c0 is None else c0.double())[0]
        run = lambda: hip(x=x.to(DEV), edge_index=ei.to(DEV), node_coords=None if c0 is None else c0.clone().to(DEV))[0].cpu().double()
        off = run()
        on = (hip.enable_hip_conn_rows(), run())[1]
    err_off, err_on = float((off - want).abs().max()), float((on - want).abs().max())
    print(f"frame {frame} coord {coord}: max|off - fp64| {err_off:.3e}, max|on - fp64| {err_on:.3e}")
    assert err_on <= 4 * err_off + 8 * U * float(want.abs().max())


def test_base_model_under_a_captured_graph_replays_on_a_second_batch():
    frame = 16
    hip, _ = model_pair(frame, NAUX, 2, seed=5, use_connection_nodes=True)
    hip.enable_hip_conn_rows()
    _, ei, _, _ = graph_tensors(frame, NAUX, BATCH, conn=True)
    ei = ei.to(DEV)
    frames = [synthetic_frames(BATCH, C, frame, 40 + k).to(DEV) for k in range(3)]
    with torch.no_grad():
        eager = [hip(x=f, edge_index=ei)[0].clone() for f in frames]
        hip.enable_hip_graph(True)
        for k in (0, 1, 2, 1):
            assert torch.equal(hip(x=frames[k], edge_index=ei)[0], eager[k]), k
    assert hip.hip_graph_captures == 1 and not torch.equal(eager[0], eager[1])


# ---------------------------------------------------------------------------
# 4. the hole this closes: the UNet model with connection nodes, every backward in HIP, bit-reproducible
# ---------------------------------------------------------------------------
FRAME = 16


def _build():
    np.random.seed(11)
    ds = data.SyntheticEchoDataset(num_aux_graphs=NAUX, frame_size=FRAME, use_connection_nodes=True)
    batch = data.to_device(data.collate([ds[i] for i in range(BATCH)], ds.topology), DEV)
    landmark = UNetNodeFeatureModel(**UNET_KW, **dict(MODEL_KW, frame_size=FRAME, use_coordinate_graph=False, gnn_dropout_p=0.5,
                                                      classifier_dropout_p=0.5)).to(DEV).train()
    landmark.enable_hip_conn_rows().enable_hip_frontend(True, train=True, tail=True)
    embedder = CNN(out_channels=[4], cnn_dropout_p=0.1).to(DEV).train().enable_hip(True, train=True)
    crit = {"bce": losses.WeightedBCEWithLogitsLoss("none", 9000, 1), "elm": losses.ExpectedLandmarkMSE(10, BATCH, FRAME, NAUX)}
    params = list(landmark.parameters()) + list(embedder.parameters())
    opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
    model = {"embedder": embedder, "landmark": landmark}

    def loss_fn():
        preds, coord_preds = engine.forward_batch(model, batch, False)
        ls = engine.compute_loss(crit, preds, batch.y, coord_preds, None, batch.valid_labels, BATCH)
        return sum(ls.values()), preds
    return landmark, embedder, opt, loss_fn


def test_two_training_steps_from_the_same_state_agree_bit_for_bit(monkeypatch):
    """Connection nodes, dropout 0.5, torch.backends.cudnn.deterministic False: logits, loss and every gradient repeat."""
    assert torch.backends.cudnn.deterministic is False
    conn_calls = []
    inner = P._conn_bwd
    monkeypatch.setattr(P, "_conn_bwd", lambda *a: conn_calls.append(1) or inner(*a))
    epoch0 = ops.dropout_epoch()
    try:
        runs = []
        for _ in range(2):
            ops.dropout_epoch_set(5)
            torch.manual_seed(123)
            lm, emb, _, loss_fn = _build()
            torch.manual_seed(77)
            loss, preds = loss_fn()
            loss.backward()
            named = list(lm.named_parameters()) + list(emb.named_parameters())
            assert all(q.grad is not None for _, q in named)
            runs.append([("loss", loss.detach()), ("logits", preds.detach())] + [(k, q.grad) for k, q in named])
        assert len(conn_calls) == 2                                                        # the connection rows' backward ran in HIP
        for (na, a), (nb, b) in zip(*runs):
            assert na == nb and torch.equal(a, b), na
        assert any(k == "linears.3.weight" for k, _ in runs[0])
    finally:
        ops.dropout_epoch_set(epoch0)


def test_the_step_captures_into_a_graphed_train_step_and_replays():
    """The protocol of tests/test_gpu_tail_engine.py: replay k of the captured step equals the eager step under epoch k."""
    warm, replays = 1, 2
    epoch0 = ops.dropout_epoch()
    try:
        ops.dropout_epoch_set(0)
        torch.manual_seed(123)
        lm_g, emb_g, opt_g, loss_g = _build()
        torch.manual_seed(77)
        step = engine.GraphedTrainStep(loss_g, opt_g, warmup=warm)
        e0 = ops.dropout_epoch()
        losses_g, preds_g = [], []
        for _ in range(replays):
            out = step()
            losses_g.append(float(out[0]))
            preds_g.append(out[1].clone())
        ops.dropout_epoch_set(e0)
        torch.manual_seed(123)
        lm_e, emb_e, opt_e, loss_e = _build()
        torch.manual_seed(77)

        def eager():
            out = loss_e()
            opt_e.zero_grad(set_to_none=True)
            out[0].backward()
            opt_e.step()
            return out
        for _ in range(warm):
            eager()
        rng = torch.get_rng_state()
        for k in range(replays):
            torch.set_rng_state(rng)
            ops.dropout_epoch_set(e0 + k + 1)
            out = eager()
            assert float(out[0].detach()) == losses_g[k], (k, float(out[0].detach()), losses_g[k])
            assert torch.equal(out[1].detach(), preds_g[k]), k
        for a, b in ((emb_g, emb_e), (lm_g, lm_e)):
            for (na, pa), (nb, pb) in zip(a.named_parameters(), b.named_parameters()):
                assert na == nb and torch.equal(pa.detach(), pb.detach()), na
        assert len(set(losses_g)) == replays, losses_g
    finally:
        ops.dropout_epoch_set(epoch0)
