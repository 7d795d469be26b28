"""-m gpu: the eval-mode forward on the routes float64 had not seen -- 'grid-diagonal' and connection-node handles on both routes of
the plain layer (split and fp32), the symmetric kernel's CSR, clustered-tile, stencil and aggregation-free forms, eg_gcn_aggregate,
the stand-alone heads and the fused last layer + heads, unfolded and folded -- per quantity against tests/eval_reference.py in
float64 under coord_reference.Report's rule: |kernel - fp64| <= 4 max|ref32 - fp64| + 8 ulp x scale, scale = the same expression on
absolute values per output element.  The forward is continuous: no element of any compared array is left out.  Every group runs
a second input set whose frames are scaled 1e-3, 1, 30, 1e4 and mixed per element; there the rule is applied frame by frame, so
that the float32 yardstick of a large frame does not excuse a small one."""
import contextlib
import itertools
import os

import numpy as np
import pytest
import torch

import eval_reference as E
import train_reference as T
from echoglad_amd import ops
from echoglad_amd.nn._heads import fold_last_into_heads

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C = 128
F64, F32 = torch.float64, torch.float32
COMBOS = list(itertools.product((True, False), repeat=3))               # relu, residual x, affine


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def _topo_graph(handle, split=None):
    """The handle of (frame, naux, main_only, coord, conn, diag_main, diag_aux); split "0": the fp32 route (EG_LAYER_SPLIT is read
    when the handle is created)."""
    frame, naux, main_only, coord, conn, dm, da = handle
    with _env("EG_LAYER_SPLIT", split):
        return ops.Graph.topo(frame, naux, main_only, coord, use_connection_nodes=conn, diag_main=dm, diag_aux=da)


def _one_launch(g, fn):
    before = g.ps_launches
    got = fn()
    assert g.ps_launches == before + 1                      # the producer / consumer kernel, once
    return got


def _finish(rep, title, capsys):
    with capsys.disabled():
        print(rep.table(title))
    assert not rep.failed(), rep.failed()


def _check(rep, name, got, r64, r32, scale, groups=None):
    """Report.check on the whole array, or group of rows by group (the second input set: a frame, or the rows of one magnitude)."""
    if groups is None:
        rep.check(name, got, r64, r32, scale)
        return
    got = got.detach().cpu()
    for rows in groups:
        rep.check(name, got[rows], r64[rows], r32[rows], scale[rows])


def _frames(B, rows_per_frame):
    return [slice(b * rows_per_frame, (b + 1) * rows_per_frame) for b in range(B)]


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


# ---------------------------------------------------------------------------
# a. the plain eval layer on diagonal and connection-node handles, both routes
# ---------------------------------------------------------------------------
ROUTES = {"split": None, "fp32": "0"}                                   # EG_LAYER_SPLIT when the handle is created


def _plain_forms(rep, handle, B, x, seed, apart, routes=("split", "fp32")):
    topo, Eg = E.topology(*handle), E.topo_edges(*handle)
    n = topo.num_nodes
    graphs = tuple((r, _topo_graph(handle, ROUTES[r])) for r in routes)
    kid_rows = graphs[0][1].kidsum_rows
    assert all(g.num_nodes == n and g.hybrid and g.kidsum_rows == kid_rows for _, g in graphs)
    assert kid_rows in (0, topo.main.base)
    w, sc, sh = E.layer_params(seed)
    xg, wg, scg, shg = _dev(x, w, sc, sh)
    x_keep = xg.clone()
    forms = E.FORMS if kid_rows > 0 else E.FORMS[:1]
    # kidsum_in: the float64 child sums of x, rounded once -- nothing of a kernel in it
    kin = E.kidsum(topo, x, B)[0].to(F32).to(DEV) if kid_rows > 0 else None
    fr, kfr = (_frames(B, n), _frames(B, kid_rows)) if apart else (None, None)
    for relu, residual, affine in COMBOS:
        scale, shift = (sc, sh) if affine else (None, None)
        r64, r32 = (E.layer_eval(Eg, B, x, w, scale, shift, "x" if residual else None, relu, dtype=dt) for dt in (F64, F32))
        if kid_rows > 0:
            k64, k_scale = E.kidsum(topo, r64["out"], B, out_scale=r64["out_scale"])
            k32 = E.kidsum(topo, r32["out"], B, F32)[0]
        for form, (route, g) in itertools.product(forms, graphs):
            ka = kin if "in" in form.split() else None
            kb = ops.new_kidsum(g, B) if "out" in form.split() else None
            got = _one_launch(g, lambda: ops.gcn_layer_fwd(g, B, xg, wg, scg if affine else None, shg if affine else None,
                                                           xg if residual else None, relu, kidsum_in=ka, kidsum_out=kb))
            _check(rep, f"out {route}, {form}", got, r64["out"], r32["out"], r64["out_scale"], fr)
            if kb is not None:
                assert kb.shape == k64.shape
                _check(rep, f"child sums {route}, {form}", kb, k64, k32, k_scale, kfr)
    assert torch.equal(xg, x_keep)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("handle", E.DIAG_HANDLES + E.CONN_HANDLES, ids=str)
def test_plain_layer_on_diagonal_and_connection_node_handles(handle, B, capsys):
    """Every ReLU / residual / affine combination, pulled, handed in (kidsum_in from the CPU), handed out, handed in and out, on the
    split and on the fp32 route; the handed-out sums against kidsum of the float64 output; one launch per call."""
    rep = E.Report()
    n = E.topology(*handle).num_nodes
    _plain_forms(rep, handle, B, E.rand_rows(B * n, seed=9), 31, apart=False)
    _finish(rep, f"a. plain layer {handle} B={B}", capsys)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("handle", E.DIAG_HANDLES + E.CONN_HANDLES, ids=str)
def test_plain_layer_over_seven_orders_of_magnitude(handle, route, capsys):
    """The second input set, the rule applied frame by frame.

    This is the test that found the fp32 route (EG_LAYER_SPLIT=0) adding the shift as the accumulators' initial value: in the frame
    scaled 1e-3, at elements that are the shift to three digits (0.135 + products of 1e-4), the shift went through every rounding
    of the 128-term fp32 chain, |err| 2.2e-7 = 12.8 ulp of the scale -- 1.11 x the bound on (17, 3) coordinate + diagonal, 1.17 on
    (64, 5) diagonal, 1.04 on (64, 5) connection + diagonal, 1.08 on (64, 6) connection nodes, 0.78 .. 0.98 on the other eight.
    gcn_layer_ps.hip now adds it behind the chain on that route (SHIFT_LATE): 0.15.  The split route accumulates onto the
    shift as before, 48 roundings in place of 128: 0.51 .. 0.73, the routes nearest the bound in this file."""
    rep = E.Report()
    n = E.topology(*handle).num_nodes
    _plain_forms(rep, handle, E.MIXED_B, E.mixed_rows(n, seed=13), 33, apart=True, routes=(route,))
    _finish(rep, f"a. plain layer {handle}, {route} route, frames scaled 1e-3, 1, 30, 1e4, mixed", capsys)


@pytest.mark.parametrize("handle", E.IDENTITY_HANDLES, ids=str)
def test_identity_weight_returns_the_fp32_routes_bits(handle, capsys):
    """W = I: the split route's hi + mid + lo is the aggregated row itself, the fp32 route's bits -- and those are A_hat x under the rule."""
    Eg, n = E.topo_edges(*handle), E.topology(*handle).num_nodes
    g_s, g_f = _topo_graph(handle), _topo_graph(handle, "0")
    eye = torch.eye(C, device=DEV)
    B = 3
    rep = E.Report()
    for mag in (1.0, 1e-3, 1e4):
        x = E.rand_rows(B * n, seed=5) * mag
        xg = x.to(DEV)
        for chained in (False, True) if g_s.kidsum_rows > 0 else (False,):
            ka = E.kidsum(E.topology(*handle), x, B)[0].to(F32).to(DEV) if chained else None
            want = _one_launch(g_f, lambda: ops.gcn_layer_fwd(g_f, B, xg, eye, kidsum_in=ka))
            got = _one_launch(g_s, lambda: ops.gcn_layer_fwd(g_s, B, xg, eye, kidsum_in=ka))
            assert torch.equal(got, want), (mag, chained, float((got - want).abs().max()))
            r64, r32 = (E.layer_eval(Eg, B, x, eye.cpu(), dtype=dt) for dt in (F64, F32))
            rep.check(f"A_hat x (W = I){', handed in' if chained else ''}", got, r64["agg"], r32["agg"], r64["agg_scale"])
    _finish(rep, f"a. W = I {handle}", capsys)


@pytest.mark.parametrize("handle", E.PER_TERM_HANDLES, ids=str)
def test_error_per_term_on_a_diagonal_and_a_connection_node_handle(handle, capsys):
    """|err| / sum_k |a_k||w_k| <= 1e-6 per output element (test 3 of tests/test_gpu_layer_split.py, the same constant), a = A_hat x
    in float64 from x alone."""
    Eg, n = E.topo_edges(*handle), E.topology(*handle).num_nodes
    B = E.MIXED_B
    x, w = E.mixed_rows(n, seed=13), E.glorot(7)
    a = E.ahat(Eg, x.double(), B)
    want, denom = a @ w.double().t(), a.abs() @ w.double().abs().t()
    assert float(denom.min()) > 0.0
    worst = {}
    for route, split in (("split", None), ("fp32", "0")):
        g = _topo_graph(handle, split)
        out = _one_launch(g, lambda: ops.gcn_layer_fwd(g, B, x.to(DEV), w.to(DEV)))
        ratio = ((out.cpu().double() - want).abs() / denom).view(B, n, C)
        worst[route] = [float(ratio[b].max()) for b in range(B)]
    with capsys.disabled():
        print(f"\n  a. {handle}: worst |err| / sum|a||w| per frame (1e-3, 1, 30, 1e4, mixed): split {worst['split']}, fp32 {worst['fp32']}")
    assert max(worst["split"]) <= E.PER_TERM_BOUND and max(worst["fp32"]) <= E.PER_TERM_BOUND, worst


@pytest.mark.parametrize("handle", E.ALONE_HANDLES, ids=str)
def test_a_frame_does_not_depend_on_its_neighbours(handle):
    topo = E.topology(*handle)
    n, B = topo.num_nodes, 3
    x, (w, sc, sh) = E.rand_rows(B * n, seed=17), E.layer_params(35)
    xg, wg, scg, shg = _dev(x, w, sc, sh)
    for split in (None, "0"):
        g = _topo_graph(handle, split)
        f1 = lambda t: None if t is None else t.view(B, -1, C)[1].contiguous()
        for chained in (False, True) if g.kidsum_rows > 0 else (False,):
            ka = E.kidsum(topo, x, B)[0].to(F32).to(DEV) if chained else None
            kb, kb1 = (ops.new_kidsum(g, B), ops.new_kidsum(g, 1)) if chained else (None, None)
            out = _one_launch(g, lambda: ops.gcn_layer_fwd(g, B, xg, wg, scg, shg, xg, relu=True, kidsum_in=ka, kidsum_out=kb))
            alone = _one_launch(g, lambda: ops.gcn_layer_fwd(g, 1, f1(xg), wg, scg, shg, f1(xg), relu=True, kidsum_in=f1(ka), kidsum_out=kb1))
            assert torch.equal(out.view(B, n, C)[1], alone), (split, chained)
            if chained:
                assert torch.equal(kb.view(B, -1, C)[1], kb1), split


# ---------------------------------------------------------------------------
# b. the symmetric kernel and the aggregation
# ---------------------------------------------------------------------------
def _layer_forms(rep, tag, g, gb, Eg, B, x, res, w, sc, sh, groups=None, own=True):
    """plain, affine + ReLU + residual x, A_hat x; own: also a residual tensor of its own, and the transposed weight on g.bwd against
    A_hat^T.  (g, gb): the handle and the batch its launches take; (Eg, B): the edges and frames the reference walks."""
    xg, rg, wg, scg, shg = _dev(x, res, w, sc, sh)
    forms = (("plain", (None, None, None, False)), ("affine relu res x", (sc, sh, "x", True)), ("own residual", (sc, sh, res, True)))
    for name, (scale, shift, residual, relu) in forms if own else forms[:2]:
        r64, r32 = (E.layer_eval(Eg, B, x, w, scale, shift, residual, relu, dtype=dt) for dt in (F64, F32))
        got = ops.gcn_layer_fwd(g, gb, xg, wg, None if scale is None else scg, None if shift is None else shg,
                                None if residual is None else (xg if isinstance(residual, str) else rg), relu)
        _check(rep, f"{tag}{name}", got, r64["out"], r32["out"], r64["out_scale"], groups)
    if own:
        Et = E.transposed(Eg)
        r64, r32 = (E.layer_eval(Et, B, x, w, None, None, res, False, transpose_w=True, dtype=dt) for dt in (F64, F32))
        got = ops.gcn_layer_fwd(g.bwd, gb, xg, wg, None, None, rg, False, transpose_w=True)
        _check(rep, f"{tag}transposed, own residual", got, r64["out"], r32["out"], r64["out_scale"], groups)
    _check(rep, f"{tag}A_hat x", ops.gcn_aggregate(g, gb, xg), E.ahat(Eg, x.double(), B), E.ahat(Eg, x, B), E.ahat(Eg, x.double().abs(), B), groups)


@pytest.mark.parametrize("tiles", ["0", "1", None], ids=["rows", "consecutive", "default"])
@pytest.mark.parametrize("kind", E.CSR_GRAPHS)
def test_symmetric_kernel_on_csr_handles(kind, tiles, capsys):
    """k_gcn_layer<AGG_CSR> / <AGG_CSRT> and k_aggregate under EG_CSR_TILES = 0, 1 and the default; two frames on a per-frame handle
    and as one batched edge list; the second input set, frame by frame."""
    ei, n = E.csr_graph(kind)
    Eg = E.edges_of(ei, n)
    w, sc, sh = E.layer_params(41)
    rep = E.Report()
    with _env("EG_CSR_TILES", tiles):
        g = ops.Graph.csr(torch.from_numpy(ei).to(DEV), n)
        g2 = ops.Graph.csr(torch.from_numpy(E.batched(ei, n, 2)).to(DEV), 2 * n)
    assert not g.structured and g.kidsum_rows == 0 and (g.bwd is not g) == (kind not in ("star", "cycle"))
    _layer_forms(rep, "", g, 1, Eg, 1, E.rand_rows(n, seed=3), E.rand_rows(n, seed=4), w, sc, sh)
    x2, res2 = E.rand_rows(2 * n, seed=5), E.rand_rows(2 * n, seed=6)
    _layer_forms(rep, "B = 2: ", g, 2, Eg, 2, x2, res2, w, sc, sh)
    _layer_forms(rep, "batched list: ", g2, 1, Eg, 2, x2, res2, w, sc, sh)
    _layer_forms(rep, "magnitudes: ", g, E.MIXED_B, Eg, E.MIXED_B, E.mixed_rows(n, seed=13), E.rand_rows(E.MIXED_B * n, seed=7), w, sc, sh,
                 groups=_frames(E.MIXED_B, n))
    _finish(rep, f"b. CSR handle, {kind}, EG_CSR_TILES={tiles}", capsys)


@pytest.mark.parametrize("frame,naux,main_only,coord", E.STENCIL_HANDLES)
def test_symmetric_stencil_kernel_where_the_producer_consumer_kernel_declines(frame, naux, main_only, coord, capsys):
    """k_gcn_layer<AGG_STENCIL, true | false>: a topology handle without a child-sum buffer and with more than one level."""
    handle = (frame, naux, main_only, coord, False, False, False)
    Eg, n = E.topo_edges(*handle), E.topology(*handle).num_nodes
    g = _topo_graph(handle)
    assert g.structured and not g.hybrid and g.kidsum_rows == 0 and naux > 0 and not main_only
    w, sc, sh = E.layer_params(43)
    rep = E.Report()
    for B, x, groups, tag in ((2, E.rand_rows(2 * n, seed=3), None, ""), (E.MIXED_B, E.mixed_rows(n, seed=13), _frames(E.MIXED_B, n), "magnitudes: ")):
        ps, every = g.ps_launches, g.layer_launches
        _layer_forms(rep, tag, g, B, Eg, B, x, None, w, sc, sh, groups, own=False)       # no residual, residual x: the two instantiations
        assert g.ps_launches == ps and g.layer_launches == every + 2          # the symmetric kernel, both times
    _finish(rep, f"b. symmetric stencil kernel ({frame}, {naux})", capsys)


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("rows", E.LINEAR_ROWS)
def test_linear128_against_fp64(rows, transpose, capsys):
    """k_gcn_layer<AGG_NONE>: no edges, A_hat = I."""
    Eg = E.edges_of(np.zeros((2, 0), dtype=np.int64), rows)
    w, sc, sh = E.layer_params(45)
    rep = E.Report()
    for tag, x in (("", E.rand_rows(rows, seed=rows)), ("magnitudes: ", E.mixed_rows(rows, seed=13)[4 * rows:].contiguous())):     # (the frame that mixes them)
        res = E.rand_rows(rows, seed=rows + 1)
        for name, (scale, shift, residual, relu) in (("plain", (None, None, None, False)), ("scale shift relu residual", (sc, sh, res, True))):
            r64, r32 = (E.layer_eval(Eg, 1, x, w, scale, shift, residual, relu, transpose_w=transpose, dtype=dt) for dt in (F64, F32))
            got = ops.linear128_fwd(x.to(DEV), w.to(DEV), *_dev(scale, shift, residual), relu=relu, transpose_w=transpose)
            groups = None if not tag else [slice(r, r + 1) for r in range(rows)]                 # row by row
            _check(rep, tag + name, got, r64["out"], r32["out"], r64["out_scale"], groups)
    _finish(rep, f"b. linear128, {rows} rows, transpose_w={transpose}", capsys)


@pytest.mark.parametrize("handle", E.AGGREGATE_HANDLES, ids=str)
def test_aggregate_on_topology_handles(handle, capsys):
    Eg, n = E.topo_edges(*handle), E.topology(*handle).num_nodes
    g = _topo_graph(handle)
    rep = E.Report()
    for B, x, groups, tag in ((2, E.rand_rows(2 * n, seed=3), None, ""), (E.MIXED_B, E.mixed_rows(n, seed=13), _frames(E.MIXED_B, n), "magnitudes: ")):
        _check(rep, tag + "A_hat x", ops.gcn_aggregate(g, B, x.to(DEV)), E.ahat(Eg, x.double(), B), E.ahat(Eg, x, B), E.ahat(Eg, x.double().abs(), B), groups)
    _finish(rep, f"b. gcn_aggregate {handle}", capsys)


# ---------------------------------------------------------------------------
# c. the stand-alone heads
# ---------------------------------------------------------------------------
def _heads_sets():
    return (("oracle heads", E.pack_heads(T.oracle_heads())), ("uniform", E.uniform_heads(7)))


@pytest.mark.parametrize("n,row_lo,n_valid,B", E.HEADS_SHAPES)
def test_classifier_against_fp64_and_rows_outside_the_filter_are_never_read(n, row_lo, n_valid, B, capsys):
    rep = E.Report()
    inside = T.frame_rows(B, n, row_lo, row_lo + n_valid)
    h = E.rand_rows(B * n, seed=3, scale=1.5)
    # the second input set: rows of magnitude 1e-3, 1, 30, 1e4 in turn, every fifth row mixing them per element; checked class by class
    cls = torch.arange(B * n) % E.MIXED_B
    mags = torch.tensor(E.MAGNITUDES + (1.0,), dtype=F32)
    h2 = h * mags[cls][:, None]
    mix = cls == len(E.MAGNITUDES)
    h2[mix] *= mags[torch.from_numpy(np.random.RandomState(2).randint(0, len(E.MAGNITUDES), (int(mix.sum()), C)))]
    valid_cls = cls[inside]
    groups = [torch.nonzero(valid_cls == k).reshape(-1) for k in range(E.MIXED_B) if bool((valid_cls == k).any())]
    for (pname, packed), sigmoid, (tag, hh, gr) in itertools.product(_heads_sets(), (False, True), (("", h, None), ("magnitudes: ", h2, groups))):
        pg = {k: v.to(DEV) for k, v in packed.items()}
        (r64, s64), (r32, _) = (E.heads_eval(packed, hh, B, n, row_lo, n_valid, sigmoid, dtype=dt) for dt in (F64, F32))
        got = ops.classifier_fwd(hh.to(DEV), B, n, row_lo, n_valid, pg, sigmoid)
        assert got.shape == (B * n_valid, 4)
        _check(rep, f"{tag}{'sigmoid' if sigmoid else 'logits'}, {pname}", got, r64, r32, s64, gr)
        poisoned = hh.clone()
        poisoned[~inside] = float("nan")
        assert torch.equal(ops.classifier_fwd(poisoned.to(DEV), B, n, row_lo, n_valid, pg, sigmoid), got), (pname, sigmoid, tag)
    _finish(rep, f"c. heads (n, row_lo, n_valid, B) = {(n, row_lo, n_valid, B)}", capsys)


# ---------------------------------------------------------------------------
# d. last layer + heads in one launch
# ---------------------------------------------------------------------------
def _cls_launches(g, B, xg, wg, scg, shg, residual, pg, sigmoid, kin):
    fold = fold_last_into_heads(wg, scg, shg, pg["w1"], pg["s1"], pg["t1"], residual)
    return (("unfolded", _one_launch(g, lambda: ops.gcn_layer_cls_fwd(g, B, xg, wg, scg, shg, xg if residual else None, False, pg, sigmoid, kidsum_in=kin))),
            ("folded", _one_launch(g, lambda: ops.gcn_layer_cls_fold_fwd(g, B, xg, fold, residual, pg, sigmoid, kidsum_in=kin))))


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("handle", E.CLS_HANDLES, ids=str)
def test_last_layer_and_heads_against_fp64_from_x_alone(handle, B, capsys):
    """eg_gcn_layer_cls_fwd and eg_gcn_layer_cls_fold_fwd against the UNFOLDED formula in float64, started from x: no aggregation of the
    library in the reference.  Residual, affine, sigmoid on and off; pulled and with kidsum_in from the CPU; both parameter sets;
    the second input set; on connection-node handles the connection rows at 1e4 times the rest."""
    args = E.cls_args(handle)
    topo, Eg = E.topology(*args), E.topo_edges(*args)
    n, n_conn = topo.num_nodes, topo.n_conn
    g = _topo_graph(args)
    assert g.fused_classifier_ok and g.num_conn == n_conn == ((handle[1] + 1) if handle[3] else 0)
    w, sc, sh = E.layer_params(51)
    wg, scg, shg = _dev(w, sc, sh)
    rep, layers = E.Report(), {}
    inputs = [("", B, E.rand_rows(B * n, seed=9), None, True), ("magnitudes: ", E.MIXED_B, E.mixed_rows(n, seed=13), _frames(E.MIXED_B, n - n_conn), False)]
    if n_conn:
        xc = E.rand_rows(B * n, seed=11).view(B, n, C)
        xc[:, :n_conn] *= E.CONN_ROWS_FACTOR
        inputs.append(("connection rows x 1e4: ", B, xc.reshape(B * n, C).contiguous(), None, False))
    for tag, Bx, x, groups, full in inputs:
        xg = x.to(DEV)
        kin = E.kidsum(topo, x, Bx)[0].to(F32).to(DEV) if g.kidsum_rows > 0 else None
        for residual, affine, (pname, packed), sigmoid in itertools.product((True, False), (True, False), _heads_sets() if full else _heads_sets()[:1],
                                                                            (False, True)):
            if not full and not affine:
                continue
            pg = {k: v.to(DEV) for k, v in packed.items()}
            scale, shift = (sc, sh) if affine else (None, None)
            key = (tag, residual, affine)
            if key not in layers:
                layers.clear()
                layers[key] = [E.layer_eval(Eg, Bx, x, w, scale, shift, "x" if residual else None, dtype=dt) for dt in (F64, F32)]
            (r64, s64), (r32, _) = (E.last_layer_heads(Eg, Bx, x, w, scale, shift, residual, packed, n_conn, sigmoid, dtype=dt, layer=L)
                                    for dt, L in zip((F64, F32), layers[key]))
            for how, k in (("pulled", None), ("handed in", kin)) if kin is not None and full else (("pulled", None),):
                for entry, got in _cls_launches(g, Bx, xg, wg, scg if affine else None, shg if affine else None, residual, pg, sigmoid, k):
                    assert got.shape == (Bx * (n - n_conn), 4)                 # no row for a connection node
                    _check(rep, f"{tag}{entry} {'sigmoid' if sigmoid else 'logits'}, {how}, {pname}", got, r64, r32, s64, groups)
    _finish(rep, f"d. last layer + heads {handle} B={B}", capsys)


@pytest.mark.parametrize("handle", E.CLS_DECLINED, ids=str)
def test_handles_the_fused_classifier_declines_raise_from_both_entry_points(handle):
    g = _topo_graph(E.cls_args(handle))
    assert not g.fused_classifier_ok
    B, n = 2, g.num_nodes
    w, sc, sh = _dev(*E.layer_params(51))
    pg = {k: v.to(DEV) for k, v in E.uniform_heads(7).items()}
    x = E.rand_rows(B * n, seed=9).to(DEV)
    fold = fold_last_into_heads(w, sc, sh, pg["w1"], pg["s1"], pg["t1"], True)
    for launch in (lambda: ops.gcn_layer_cls_fwd(g, B, x, w, sc, sh, x, False, pg), lambda: ops.gcn_layer_cls_fold_fwd(g, B, x, fold, True, pg)):
        with pytest.raises(RuntimeError, match="unsupported"):
            launch()
