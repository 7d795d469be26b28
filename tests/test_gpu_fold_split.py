"""-m gpu: the bf16 body of the folded last layer + heads (k_gcn_layer_ps FSPLIT, eg_gcn_layer_cls_fold_split_fwd: exact 3-piece
splits of both operands, v_mfma_f32_16x16x32_bf16, the lo planes of FOLD = 1 streamed from a table) against float64 through
tests/eval_reference.py under coord_reference.Report's rule -- the bound of the folded cases of tests/test_gpu_eval_fp64.py --, with
the fp32 body (a handle created under EG_LAYER_SPLIT=0) measured beside it; the pairing of the streamed lo fragments; the switch;
launch-to-launch and batch determinism, once at full grid.

Which lo fragment goes with which (matrix, k-step, column block) is NOT pinned by the float64 cases over whole arrays: a lo plane
is worth 2^-16 of a product, and the rule's yardstick, the worst fp32 error of the array, leaves room for that (mutation builds,
profiles/fold_split_ab.txt 8; nor does it see a left-out mid.mid product, node by node either: tests/test_gpu_fold_probe.py is
what catches that, product by product through probe heads, profiles/fold_probe_mutations.txt).  Each half is therefore checked alone with a hand-made table over zero hi and mid planes: W1s exactly, with inputs that are powers of two, M -- which
multiplies aggregated rows, which are not -- within the bound that hi()'s 8 significant bits give."""
import contextlib
import os

import numpy as np
import pytest
import torch

import eval_reference as E
import train_reference as T
from echoglad_amd import ops
from echoglad_amd.nn._heads import fold_last_into_heads
from echoglad_amd.ops._core import call

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C = 128
F64, F32 = torch.float64, torch.float32
HEAD_KEYS = E.HEAD_KEYS

# (frame, naux, main_only, coord, conn, diag_main, diag_aux), batch: ragged tiles, about one tile per workgroup / 1 200 tiles, four
# to five per workgroup, so that the ring and both LDS buffers reach their steady state
SHAPES = [((16, 3, False, False, False, False, False), 2), ((16, 3, False, False, False, True, True), 2),
          ((64, 6, False, False, False, False, False), 8), ((64, 6, False, False, False, True, True), 8)]


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


def _graph(handle, split=None):
    frame, naux, main_only, coord, conn, dm, da = handle
    with _env("EG_LAYER_SPLIT", split):          # read when the handle is created
        return ops.Graph.topo(frame, naux, main_only, coord, use_connection_nodes=conn, diag_main=dm, diag_aux=da)


def _one_launch(g, fn):
    before = g.ps_launches
    got = fn()
    assert g.ps_launches == before + 1
    return got


def _direct_fp32(g, B, x, fold, residual, pg, sigmoid=False, kin=None):
    """eg_gcn_layer_cls_fold_fwd itself: the fp32 body on every handle."""
    out = torch.empty((g.num_nodes - g.num_conn) * B, 4, dtype=F32, device=x.device)
    call("eg_gcn_layer_cls_fold_fwd", g._h, B, x, bool(residual), kin, *fold[:3], *[pg[k] for k in HEAD_KEYS[3:]], sigmoid, out)
    return out


_REF = {}


def _reference(handle, B, mag, residual):
    """(x, float64 logits, float32 logits, scale) of the unfolded formula, started from x alone; computed once per case."""
    key = (handle, B, mag, residual)
    if key not in _REF:
        _REF.clear()                                                   # (cases arrive grouped: one input set is held at a time)
        topo, Eg = E.topology(*handle), E.topo_edges(*handle)
        x = E.rand_rows(B * topo.num_nodes, seed=9) * mag
        w, sc, sh = E.layer_params(51)
        packed = E.pack_heads(T.oracle_heads())
        layers = [E.layer_eval(Eg, B, x, w, sc, sh, "x" if residual else None, dtype=dt) for dt in (F64, F32)]
        (r64, s64), (r32, _) = (E.last_layer_heads(Eg, B, x, w, sc, sh, residual, packed, 0, False, dtype=dt, layer=L)
                                for dt, L in zip((F64, F32), layers))
        _REF[key] = (topo, x, (w, sc, sh), packed, r64, r32, s64)
    return _REF[key]


@pytest.mark.parametrize("mag", [1e-3, 1.0, 1e4])
@pytest.mark.parametrize("handle,B", SHAPES, ids=str)
def test_both_folds_against_fp64_beside_the_fp32_body(handle, B, mag, capsys):
    """FOLD 1 and 2, pulled and with kidsum_in, rows scaled 1e-3, 1 and 1e4 (a case each: the float64 reference of the larger shape
    takes seconds per input set); the condition is Report's rule on the split body, the fp32 body's ratio is printed beside it (and
    held to the same rule: it is the parent's code)."""
    g_split, g_fp32 = _graph(handle), _graph(handle, "0")
    rep = E.Report()
    if True:
        for residual in (True, False):
            topo, x, (w, sc, sh), packed, r64, r32, s64 = _reference(handle, B, mag, residual)
            xg, pg = x.to(DEV), {k: v.to(DEV) for k, v in packed.items()}
            fold = fold_last_into_heads(w.to(DEV), sc.to(DEV), sh.to(DEV), pg["w1"], pg["s1"], pg["t1"], residual)
            kin = E.kidsum(topo, x, B)[0].to(F32).to(DEV) if g_split.kidsum_rows > 0 else None
            for how, k in (("pulled", None), ("handed in", kin)) if kin is not None else (("pulled", None),):
                for body, g in (("split", g_split), ("fp32", g_fp32)):
                    got = _one_launch(g, lambda: ops.gcn_layer_cls_fold_fwd(g, B, xg, fold, residual, pg, kidsum_in=k))
                    rep.check(f"{body} x{mag:g} fold {1 if residual else 2} {how}", got, r64, r32, s64)
    with capsys.disabled():
        print(rep.table(f"folded last layer + heads, bf16 body beside fp32 body, {handle} B={B} rows x{mag:g}"))
    assert not rep.failed(), rep.failed()


def _tail(u, packed, dtype, absolute=False):
    """The heads behind their first pre-activation u [rows, 128] (no sigmoid); absolute: the same expression on absolute values."""
    d = (lambda t: t.detach().cpu().to(dtype).abs()) if absolute else (lambda t: t.detach().cpu().to(dtype))
    h = torch.relu(u).view(-1, 4, 32)
    z = torch.einsum("nhk,hok->nho", h, d(packed["w2"]))
    z = torch.relu(d(packed["s2"]).view(4, 16) * z + d(packed["t2"]).view(4, 16))
    return (z * d(packed["w3"])).sum(-1) + d(packed["b3"])


def _folded_eval(Eg, B, x, fold, packed, dtype):
    """u = (A_hat x) m1^T + x w1s^T + c1 and the heads' tail in `dtype`, from x alone -> (logits, Report's scale)."""
    m1, w1s, c1 = (t.detach().cpu().to(dtype) for t in fold[:3])
    xd = x.detach().cpu().to(dtype)
    u = E.ahat(Eg, xd, B) @ m1.T + xd @ w1s.T + c1
    ua = E.ahat(Eg, xd.abs(), B) @ m1.abs().T + xd.abs() @ w1s.abs().T + c1.abs()
    return _tail(u, packed, dtype), _tail(ua, packed, dtype, absolute=True)


def _report_rule(name, got, Eg, B, x, fold, packed):
    (r64, s64), (r32, _) = (_folded_eval(Eg, B, x, fold, packed, dt) for dt in (F64, F32))
    rep = E.Report()
    rep.check(name, got, r64, r32, s64)
    print(rep.table(name))
    return rep


def _pow2_rows(rows, seed):
    rs = np.random.RandomState(seed)
    return torch.from_numpy((np.ldexp(1.0, rs.randint(-3, 2, (rows, C))) * rs.choice((-1.0, 1.0), (rows, C))).astype(np.float32))


def _bf16_exact(t):
    return (t.contiguous().view(torch.int32) & -65536).view(F32)


@pytest.mark.parametrize("handle,B", SHAPES[1:3], ids=str)
def test_streamed_lo_fragments_meet_their_k_step_and_column_block(handle, B):
    """m1 = w1s = 0 (zero hi and mid planes) and a hand-made table: the W1s half holds a bf16-exact random matrix, the M half zeros.
    The only product left is lo(W1s) . hi(x), and with x powers of two hi(x) = x: the fp32 body on (0, that matrix) computes the same
    sums of exactly representable products.  A fragment paired with another k-step, matrix or column block gives another matrix."""
    g, g_fp32 = _graph(handle), _graph(handle, "0")
    n = g.num_nodes
    x = _pow2_rows(B * n, 5).to(DEV)
    pg = {k: v.to(DEV) for k, v in E.uniform_heads(7).items()}
    wb = _bf16_exact(E.glorot(77)).to(DEV)
    zero = torch.zeros(C, C, device=DEV)
    c1 = (0.1 * E.rand_rows(1, 3)).reshape(C).to(DEV)
    ch, k = ops.fold_lo_index(DEV)
    table = torch.zeros(2, 4, 4, 2, 4, 16, 8, dtype=torch.int16, device=DEV)
    table[1] = (wb.view(torch.int32) >> 16).to(torch.int16)[ch, k]
    got = _one_launch(g, lambda: ops.gcn_layer_cls_fold_fwd(g, B, x, (zero, zero, c1, table), True, pg))
    Eg = E.topo_edges(*handle)
    # every product is exact: the float64 rule holds for the formula with (0, that matrix), for the fp32 body and for this one
    assert not _report_rule("lo(W1s) alone", got, Eg, B, x, (zero, wb, c1), pg).failed()
    assert not _report_rule("fp32 body", _direct_fp32(g_fp32, B, x, (zero, wb, c1), True, pg), Eg, B, x, (zero, wb, c1), pg).failed()
    wrong = table.clone()
    wrong[1, 0], wrong[1, 1] = table[1, 1], table[1, 0]              # (the check sees a swap of two k-steps)
    bad = ops.gcn_layer_cls_fold_fwd(g, B, x, (zero, zero, c1, wrong), True, pg)
    assert _report_rule("two k-steps swapped", bad, Eg, B, x, (zero, wb, c1), pg).failed()


@pytest.mark.parametrize("handle,B", SHAPES[1:3], ids=str)
def test_streamed_lo_fragments_of_the_first_matrix(handle, B):
    """The M half alone: m1 = w1s = 0, table[0] holds a bf16-exact random matrix Wb.  What is left is lo(M) . hi(A_hat x), and the
    aggregated rows are no powers of two: hi() cuts them to 8 significant bits, |hi(a) - a| < 2^-7 |a|.  Against the fp32 body on
    (Wb, 0) the bound is therefore derived, not exact: 2^-7 sum |w||a| per hidden unit, carried through the heads' tail on absolute
    values (ReLU is 1-Lipschitz), plus the float64 rule's share for the fp32 body's own rounding.  A fragment of another k-step is
    another matrix: its error is of the order of sum |w||a| itself."""
    g, g_fp32 = _graph(handle), _graph(handle, "0")
    x = E.rand_rows(B * g.num_nodes, seed=5).to(DEV)
    pg = {k: v.to(DEV) for k, v in E.uniform_heads(7).items()}
    wb = _bf16_exact(E.glorot(78)).to(DEV)
    zero = torch.zeros(C, C, device=DEV)
    c1 = (0.1 * E.rand_rows(1, 3)).reshape(C).to(DEV)
    ch, k = ops.fold_lo_index(DEV)
    table = torch.zeros(2, 4, 4, 2, 4, 16, 8, dtype=torch.int16, device=DEV)
    table[0] = (wb.view(torch.int32) >> 16).to(torch.int16)[ch, k]
    got = _one_launch(g, lambda: ops.gcn_layer_cls_fold_fwd(g, B, x, (zero, zero, c1, table), True, pg))
    want = _direct_fp32(g_fp32, B, x, (wb, zero, c1), True, pg)
    agg = ops.gcn_aggregate(g, B, x).double().cpu()
    du = 2.0 ** -7 * (agg.abs() @ wb.double().cpu().abs().T)
    d = lambda t: t.double().cpu().abs()
    dz = d(pg["s2"]).view(4, 16) * torch.einsum("nhk,hok->nho", du.view(-1, 4, 32), d(pg["w2"]))
    bound = (dz * d(pg["w3"])).sum(-1) + 1e-5 * (1.0 + want.double().cpu().abs())
    err = (got.double().cpu() - want.double().cpu()).abs()
    print("lo(M) alone: worst error / derived bound", float((err / bound).max()))
    assert bool((err <= bound).all())
    wrong = table.clone()
    wrong[0, 0], wrong[0, 1] = table[0, 1], table[0, 0]
    bad = ops.gcn_layer_cls_fold_fwd(g, B, x, (zero, zero, c1, wrong), True, pg)
    worst = float(((bad.double().cpu() - want.double().cpu()).abs() / bound).max())
    print("two k-steps swapped: worst error / derived bound", worst)
    assert worst > 1.0


@pytest.mark.parametrize("matrix,step", [(0, 0), (0, 3), (1, 1), (1, 2)])
def test_weights_in_one_k_step_of_one_matrix(matrix, step):
    """Weights that are nonzero only in the 32 k of one step of one matrix (k = koff(kq) + 8 step + e): the bf16 body and the fp32
    body on the same handle pair, each inside the float64 rule of the folded formula with those weights."""
    handle, B = SHAPES[2]
    g, g_fp32 = _graph(handle), _graph(handle, "0")
    topo, x, (w, sc, sh), packed, _, _, _ = _reference(handle, B, 1.0, True)
    xg, pg = x.to(DEV), {k: v.to(DEV) for k, v in packed.items()}
    m1, w1s, c1 = fold_last_into_heads(w.to(DEV), sc.to(DEV), sh.to(DEV), pg["w1"], pg["s1"], pg["t1"], True)
    keep = torch.zeros(C, dtype=torch.bool, device=DEV)
    for kq, off in enumerate((0, 64, 32, 96)):
        keep[off + 8 * step: off + 8 * step + 8] = True
    mats = [m1, w1s]
    mats[matrix] = mats[matrix] * keep
    mats[1 - matrix] = torch.zeros_like(m1)
    fold = (mats[0].contiguous(), mats[1].contiguous(), c1)
    got = ops.gcn_layer_cls_fold_fwd(g, B, xg, fold, True, pg)
    want = _direct_fp32(g_fp32, B, xg, fold, True, pg)
    full = _direct_fp32(g_fp32, B, xg, (m1, w1s, c1), True, pg)
    assert float((want - full).abs().max()) > 1e-3                   # the step carries weight
    Eg = E.topo_edges(*handle)
    assert not _report_rule(f"split, matrix {matrix} step {step}", got, Eg, B, x, fold, packed).failed()
    assert not _report_rule(f"fp32, matrix {matrix} step {step}", want, Eg, B, x, fold, packed).failed()


def test_switch_selects_the_body():
    handle, B = SHAPES[2]
    g, g_fp32 = _graph(handle), _graph(handle, "0")
    topo, x, (w, sc, sh), packed, r64, r32, s64 = _reference(handle, B, 1.0, True)
    xg, pg = x.to(DEV), {k: v.to(DEV) for k, v in packed.items()}
    fold = fold_last_into_heads(w.to(DEV), sc.to(DEV), sh.to(DEV), pg["w1"], pg["s1"], pg["t1"], True)
    direct = _direct_fp32(g, B, xg, fold, True, pg)                     # the old entry point: fp32 on every handle
    assert torch.equal(_direct_fp32(g_fp32, B, xg, fold, True, pg), direct)
    assert torch.equal(ops.gcn_layer_cls_fold_fwd(g_fp32, B, xg, fold, True, pg), direct)      # EG_LAYER_SPLIT=0: the fp32 body
    split = ops.gcn_layer_cls_fold_fwd(g, B, xg, fold, True, pg)
    assert not torch.equal(split, direct)                               # another summation: some bits differ ...
    rep = E.Report()
    rep.check("split", split, r64, r32, s64)                            # ... inside the rule
    assert not rep.failed(), rep.failed()


@pytest.mark.parametrize("frame,naux,B", [(64, 6, 8), (224, 7, 8)])
def test_200_launches_give_the_same_bits(frame, naux, B):
    """(224, 7) B = 8 is the one full-size case: the packed-instruction fault of the plain split layer showed only with the grid full."""
    g = ops.Graph.topo(frame, naux)
    n = g.num_nodes
    x = torch.randn(B * n, C, device=DEV, generator=torch.Generator(DEV).manual_seed(6))
    w, sc, sh = (t.to(DEV) for t in E.layer_params(51))
    pg = {k: v.to(DEV) for k, v in E.uniform_heads(7).items()}
    fold = fold_last_into_heads(w, sc, sh, pg["w1"], pg["s1"], pg["t1"], True)
    fold = fold + (ops.fold_lo_table(fold[0], fold[1]),)
    first = ops.gcn_layer_cls_fold_fwd(g, B, x, fold, True, pg)
    differ = torch.zeros((), dtype=torch.int64, device=DEV)
    for _ in range(199):
        differ += (ops.gcn_layer_cls_fold_fwd(g, B, x, fold, True, pg) != first).sum()
    assert int(differ) == 0
    if frame == 64:                                                     # one frame alone equals its rows in the batch
        alone = ops.gcn_layer_cls_fold_fwd(g, 1, x[3 * n:4 * n].contiguous(), fold, True, pg)
        assert torch.equal(first.view(B, n, 4)[3], alone)
