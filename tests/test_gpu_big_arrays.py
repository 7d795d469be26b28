"""-m gpu: node arrays of 2 GiB and more -- batch 59+ at 224 / 7 -- on the routes that only exist at that size.

Every [rows, 128] fp32 array the other GPU tests put on the device is 1.18 GB or smaller; the code changes behaviour at 2 GiB per array
(72,020 rows x 512 B per frame at 224 / 7: batch 58 is below, batch 59 above):
  * eg_classifier_bwd / _bwd_sums: k_cls_first_bwd<SUMS, false> (first_bwd_role_flat, flat 32-bit ELEMENT offsets) instead of the
    buffer-descriptor form, and no recompute_h -- nn._train keeps the last layer's output h in full and the heads' backward reads it;
  * eg_launch_bn_bwd: the generic k_bn_bwd_apply_dw<false, true> with an EMPTY row map instead of the buffer-descriptor form;
  * the descriptor forms at their upper edge (a tile's overhang, 32-bit byte offsets just below 2^31);
  * everything else of a step (per-frame descriptors of the layer kernels, tile-order activation pass, pooling pyramid and packing,
    the coordinate update's taps, the dropout counters) sees byte offsets >= 2^31 and row numbers >= 4.19 M for the first time.

Scope: arrays from 2 GiB to below 4 GiB.  Arrays of 8 GiB and more (2^31 elements, batch 233+ at 224 / 7) and first_bwd_covers' limit of
2^32 elements are NOT covered here.

References and bounds.  Kernel- and head-level: the same operation in plain torch in fp64 ON THE DEVICE (no CPU oracle on a big batch, no
host-made inputs: torch.randn with a device generator plus a per-channel scale and offset), under the project's derived rule
(test_gpu_train.test_cfg4_train_step_error_against_fp64_is_the_references_own): per quantity
        |hip - fp64| <= 4 x |torch fp32 on the device - fp64| + 8 ulp x scale            (scale = the quantity's largest fp64 entry)
with the fp32 torch run evaluated in the same test; err, ref_err and their ratio are printed for every quantity.  Frame-local
quantities: bit equality with the same frame run alone.  The whole step (part 4): the bounds of
test_gpu_train.test_cfg4_train_full_batch_32_properties.

Every test checks torch.cuda.mem_get_info() first (skip with the needed / free amounts only when the card cannot hold it), frees what
it built, and prints its peak device memory."""
import copy
import functools
import gc

import pytest
import torch

from gpu_util import DEV, model_pair
from echoglad_amd import ops

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
FACTOR = 4.0
GIB = float(1 << 30)
R_HI = 4_200_037            # 2.15 GB per array; no multiple of 4, 64 or 128
R_EDGE = 4_194_303          # the last row count eg_launch_bn_bwd still takes in its buffer-descriptor form (rows * 512 < 2^31)
WORST = {}                  # part -> worst err / tol seen (printed with every table)


def _big(need_gib):
    """The test needs `need_gib` GiB of device memory: skip when the card has less free (needed and free amounts in the reason);
    afterwards the test's tensors are gone (they were locals of the wrapped function), the cache is emptied and the peak is printed."""
    def deco(fn):
        @functools.wraps(fn)
        def wrapper(*args, **kw):
            free = torch.cuda.mem_get_info()[0]
            if free < need_gib * GIB:
                pytest.skip(f"needs {need_gib} GiB of device memory, {free / GIB:.1f} GiB are free")
            torch.cuda.reset_peak_memory_stats()
            try:
                return fn(*args, **kw)
            finally:
                gc.collect()
                torch.cuda.empty_cache()
                with kw["capsys"].disabled():
                    print(f"    [{fn.__name__}] peak device memory {torch.cuda.max_memory_allocated() / GIB:.2f} GiB")
        return wrapper
    return deco


def _rows(rows, seed, scale=1.0, offset=0.0, cols=128):
    """[rows, cols] fp32 made ON the device: standard normal x a per-channel scale + a per-channel offset."""
    g = torch.Generator(DEV)
    g.manual_seed(seed)
    x = torch.randn(rows, cols, generator=g, device=DEV)
    c = torch.arange(cols, device=DEV, dtype=torch.float32)
    return x.mul_(scale * (1.0 + 0.25 * torch.sin(c))).add_(offset * torch.cos(0.7 * c))


def _vec(kind):
    c = torch.arange(128, device=DEV, dtype=torch.float32)
    return {"gamma": 1.0 + 0.3 * torch.sin(1.3 * c), "beta": 0.1 * torch.cos(2.1 * c), "mean": 0.2 * torch.cos(0.7 * c),
            "invstd": 1.0 / (1.5 * (1.0 + 0.25 * torch.sin(c)))}[kind].contiguous()


def _kernel_mask(rows, p, seed):
    """keep_scale (0 or 1 / (1 - p)) of every element of a [rows, 128] array: a function of (seed, flat element index), read back
    through eg_bn_act_fwd on ones, as the other train tests do."""
    one, zero = torch.ones(128, device=DEV), torch.zeros(128, device=DEV)
    return ops.bn_act_fwd(torch.ones(rows, 128, device=DEV), one, zero, None, False, p, seed)


class _Table:
    """err = |hip - fp64|, ref_err = |torch fp32 - fp64| (max over the elements), tol = FACTOR x ref_err + 8 ulp x scale."""

    def __init__(self, part, title):
        self.part, self.title, self.rows = part, title, []

    def add(self, name, hip, ref32, ref64, scale=None):
        assert hip.shape == ref64.shape == ref32.shape, (name, hip.shape, ref32.shape, ref64.shape)
        r64 = ref64.double()
        err = float((hip.double() - r64).abs().max())
        ref_err = float((ref32.double() - r64).abs().max())
        scale = float(r64.abs().max()) if scale is None else scale
        self.rows.append((name, err, ref_err, FACTOR * ref_err + 8 * ULP * scale))

    def add_tail(self, name, hip, ref32, ref64, rows=128):
        """The whole array, and its last rows on their own (where a wrapped offset lands)."""
        self.add(name, hip, ref32, ref64)
        self.add(f"{name} [last {rows} rows]", hip[-rows:], ref32[-rows:], ref64[-rows:])

    def check(self, capsys):
        worst = max(e / t for _, e, _, t in self.rows)
        WORST[self.part] = max(WORST.get(self.part, 0.0), worst)
        with capsys.disabled():
            print(f"\n  {self.title}: worst err / tol = {worst:.3f}   (part {self.part} so far: {WORST[self.part]:.3f})")
            for name, err, ref_err, tol in self.rows:
                print(f"    {name:46s} |hip-fp64| {err:.3e}   |torch32-fp64| {ref_err:.3e}   ratio {err / max(ref_err, 1e-300):8.2f}   "
                      f"tol {tol:.3e}   err/tol {err / tol:.3f}")
        bad = [(n, e, t) for n, e, _, t in self.rows if not e <= t]
        assert not bad, bad


# =====================================================================================================================================
# 1. the flat operators at the crossing
# =====================================================================================================================================
@_big(20)
def test_flat_reductions_at_the_crossing(capsys):
    """eg_colsum128, eg_bn_stats, eg_dweight128 over 4,200,037 rows (2.15 GB) against fp64; the last 128 rows on their own as well: the
    same operators on arrays that are zero everywhere else must return those rows' sums."""
    R = R_HI
    x, g = _rows(R, 1, 2.0, 0.5), _rows(R, 2, 1.0, 0.1)
    x64, g64 = x.double(), g.double()
    t = _Table(1, f"colsum128 / bn_stats / dweight128 at {R} rows")
    t.add("colsum128", ops.colsum128(x), x.sum(0), x64.sum(0))
    mean, var = ops.bn_stats(x)
    t.add("bn_stats mean", mean, x.mean(0), x64.mean(0))
    t.add("bn_stats var", var, x.var(0, unbiased=False), x64.var(0, unbiased=False))
    again = ops.bn_stats(x)
    assert torch.equal(again[0], mean) and torch.equal(again[1], var)
    t.add("dweight128", ops.dweight128(g, x), g.t() @ x, g64.t() @ x64)
    # everything but the last 128 rows zero
    x2, g2 = torch.zeros_like(x), torch.zeros_like(g)
    x2[-128:] = x[-128:]
    g2[-128:] = g[-128:]
    t.add("colsum128, last 128 rows only", ops.colsum128(x2), x[-128:].sum(0), x64[-128:].sum(0))
    t.add("bn_stats mean, last 128 rows only", ops.bn_stats(x2)[0], x[-128:].sum(0) / R, x64[-128:].sum(0) / R)
    want = g64[-128:].t() @ x64[-128:]
    t.add("dweight128, last 128 rows of g only", ops.dweight128(g2, x), g[-128:].t() @ x[-128:], want)
    t.add("dweight128, last 128 rows of x only", ops.dweight128(g, x2), g[-128:].t() @ x[-128:], want)
    t.check(capsys)


@pytest.mark.parametrize("relu,p", [(False, 0.0), (True, 0.0), (False, 0.3), (True, 0.3)])
@_big(28)
def test_bn_act_fwd_at_the_crossing(relu, p, capsys):
    """eg_bn_act_fwd (affine, dropout with the kernel's own mask, ReLU, residual) over 4,200,037 rows against the fp64 formula."""
    R, seed = R_HI, 1234
    z, res = _rows(R, 3, 1.5, 0.2), (_rows(R, 4) if relu else None)         # (with and without a residual)
    scale, shift = (_vec("gamma") * _vec("invstd")).contiguous(), _vec("beta")
    out = ops.bn_act_fwd(z, scale, shift, res, relu, p, seed)
    mask = _kernel_mask(R, p, seed) if p > 0 else None

    def ref(dt):
        v = z.to(dt) * scale.to(dt) + shift.to(dt)
        if mask is not None:
            v = v * mask.to(dt)
        v = torch.relu(v) if relu else v
        return v if res is None else v + res.to(dt)

    t = _Table(1, f"bn_act_fwd at {R} rows, relu {relu}, p {p}")
    t.add_tail("out", out, ref(torch.float32), ref(torch.float64))
    t.check(capsys)
    assert torch.equal(out, ops.bn_act_fwd(z, scale, shift, res, relu, p, seed))


@_big(14)
def test_dropout_mask_past_byte_2_to_the_31(capsys):
    """The mask beyond byte offset 2^31 is still the function of (seed, element index) the forward used
    (test_dropout_mask_statistics_and_consistency at 4,200,037 rows): values, the keep rate of the last 1 M elements, the backward's
    regenerated mask (dbeta == y.sum(0)), a prefix equal to the same rows of a short array, another seed another mask."""
    R, p, seed = R_HI, 0.3, 1234
    one, zero = torch.ones(128, device=DEV), torch.zeros(128, device=DEV)
    ones = torch.ones(R, 128, device=DEV)
    y = ops.bn_act_fwd(ones, one, zero, None, False, p, seed)
    assert torch.all((y == 0) | (y == 1.0 / (1 - p)))
    keep = (y != 0)
    assert abs(keep.float().mean().item() - (1 - p)) < 5e-3
    assert abs(keep.reshape(-1)[-(1 << 20):].float().mean().item() - (1 - p)) < 5e-3               # the last 1 M elements
    assert abs(keep[-8192:].float().mean(0).min().item() - (1 - p)) < 0.02                        # per channel over the last 8192 rows
    assert torch.equal(y, ops.bn_act_fwd(ones, one, zero, None, False, p, seed))
    assert torch.equal(y[:4097], ops.bn_act_fwd(ones[:4097].contiguous(), one, zero, None, False, p, seed))
    other = ops.bn_act_fwd(ones, one, zero, None, False, p, seed + 1)
    assert not torch.equal(y[-128:], other[-128:])
    del other, keep
    dz, dgamma, dbeta = ops.bn_act_bwd(ones, ones, zero, one, one, zero, relu=False, dropout_p=p, seed=seed)
    want = y.sum(0, dtype=torch.float64)
    assert torch.allclose(dbeta.double(), want, rtol=1e-6, atol=0)
    assert torch.allclose(dbeta.double(), y[-128:].sum(0, dtype=torch.float64) + y[:-128].sum(0, dtype=torch.float64), rtol=1e-6, atol=0)


def _bn_bwd_fused(graph, dy, z, x, mean, invstd, gamma, beta, relu, p, seed):
    """eg_launch_bn_bwd's fused form (apply + weight gradient in one kernel: dz is written AND fed to dW = dz^T x) over plain rows:
    eg_gcn_layer_bwd on a handle with that many nodes, dz wanted, no dX launch.  -> (dz, dgamma, dbeta, dW)"""
    from echoglad_amd.ops._core import _seed, _workspace, call
    bn = torch.stack([mean, invstd, gamma * invstd, beta - mean * gamma * invstd]).contiguous()
    dz, dw, small = torch.empty_like(z), torch.empty(128, 128, device=DEV), torch.empty(3, 128, device=DEV)
    call("eg_gcn_layer_bwd", graph._h, 1, dy, z, x, torch.eye(128, device=DEV), gamma, beta, bn, bool(relu), float(p), _seed(seed), False,
         _workspace(z.device), dz, None, dw, small[0], small[1], small[2])
    assert float(small[0].abs().max()) == 0                       # (the bias in front of a train-mode BatchNorm)
    return dz, small[1], small[2], dw


def _push_off_the_relu_kink(z, mean, invstd, gamma, beta, delta=1e-3):
    """The backward is discontinuous where v = xhat * gamma + beta is zero: an fp32 and an fp64 evaluation that put one of the 537 M
    values on different sides differ by a whole term in that element.  The inputs are moved away from it (|v| >= delta / 2, checked in
    fp64): what is compared is arithmetic, not on which side of a tie a rounding error falls."""
    v = (z - mean) * invstd * gamma + beta
    z.add_(torch.where(v.abs() < delta, 2 * delta / (invstd * gamma), torch.zeros((), device=z.device)))
    v64 = (z.double() - mean.double()) * invstd.double() * gamma.double() + beta.double()
    assert float(v64.abs().min()) >= delta / 2
    return z


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("rows", [R_HI, R_EDGE])
@_big(40)
def test_bn_act_bwd_at_the_crossing(rows, fused, capsys):
    """eg_bn_act_bwd (sums pass + k_bn_bwd_apply) and the fused apply + weight-gradient form (k_bn_bwd_apply_dw: at 4,194,303 rows the
    buffer-descriptor form at its upper edge, at 4,200,037 rows the generic form with an empty row map) against the fp64 formulas;
    ReLU on and off, p = 0 and p = 0.3 with the kernel's own mask."""
    seed = 4321
    mean, invstd, gamma, beta = _vec("mean"), _vec("invstd"), _vec("gamma"), _vec("beta")
    dy = _rows(rows, 5, 1.0, 0.05)
    z = _push_off_the_relu_kink(_rows(rows, 6, 1.5, 0.2), mean, invstd, gamma, beta)
    x = _rows(rows, 7, 1.0, 0.3) if fused else None
    graph = ops.Graph.csr(torch.tensor([[0, 1], [1, 0]], dtype=torch.int64, device=DEV), rows) if fused else None
    mask3 = _kernel_mask(rows, 0.3, seed)

    def ref(dt, relu, mask):
        m, i, ga, be = (v.to(dt) for v in (mean, invstd, gamma, beta))
        xhat = (z.to(dt) - m) * i
        g = dy.to(dt) if mask is None else dy.to(dt) * mask.to(dt)
        if relu:
            g = g * (xhat * ga + be > 0)
        dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
        dz = ga * i * (g - dbeta / rows - xhat * (dgamma / rows))
        return dz, dgamma, dbeta, (dz.t() @ x.to(dt) if fused else None)

    for relu, p in ((False, 0.0), (True, 0.0), (False, 0.3), (True, 0.3)):
        if fused:
            got = _bn_bwd_fused(graph, dy, z, x, mean, invstd, gamma, beta, relu, p, seed)
        else:
            got = ops.bn_act_bwd(dy, z, mean, invstd, gamma, beta, relu, p, seed) + (None,)
        mask = mask3 if p > 0 else None
        r32, r64 = ref(torch.float32, relu, mask), ref(torch.float64, relu, mask)
        t = _Table(1, f"bn_act_bwd{' + dW' if fused else ''} at {rows} rows, relu {relu}, p {p}")
        t.add_tail("dz", got[0], r32[0], r64[0])
        t.add("dgamma", got[1], r32[1], r64[1])
        t.add("dbeta", got[2], r32[2], r64[2])
        if fused:
            t.add("dW", got[3], r32[3], r64[3])
        del r32, r64
        t.check(capsys)
        del got


# =====================================================================================================================================
# 2. the heads: both forms of the first-layers kernel
# =====================================================================================================================================
HEAD_SHAPES = [(72020, 0, 72020, 59),            # batch 59 at 224 / 7 without coordinate rows: flat
               (72024, 0, 72020, 59),            # ... with the 4 coordinate rows filtered out: flat, dh's dropped rows exact zeros
               (2096127, 0, 2096127, 2),         # 2,146,434,048 B: the largest size the buffer-descriptor form admits
               (2096128, 0, 2096128, 2)]         # the first flat one


@pytest.mark.parametrize("n,row_lo,n_valid,B", HEAD_SHAPES)
@_big(64)
def test_heads_train_kernels_across_2_gib(n, row_lo, n_valid, B, capsys):
    """eg_classifier_train_fwd, eg_classifier_train_fwd_act, eg_classifier_bwd and eg_classifier_bwd_sums against the four heads
    written with torch modules (test_gpu_train._torch_heads) in fp64 and fp32 on the device, with the kernels' own masks: logits,
    dh, the 40 parameter gradients, the running statistics, the layer's BatchNorm-backward sums.  The route predicates say which
    body of the first-layers kernel ran; asking for recompute= where it does not exist raises before anything is launched."""
    from echoglad_amd.nn import _MLP_NAMES, _seq_params, _stack_head_params, _unstack_head_grads
    from echoglad_amd.ops._core import _cls_workspace
    from test_gpu_train import _torch_heads
    R = B * n_valid
    direct = (n, B) == (2096127, 2)
    assert ops.classifier_recompute_h_supported(B, n, n_valid) == direct
    assert ops.classifier_layer_sums_supported(B, n, n_valid)
    hip, _ = model_pair(16, 3, 1, seed=n % 1000 + B)
    hip.train()
    # The backward is discontinuous where a hidden pre-activation v = xhat * gamma + beta is zero: an fp32 and an fp64 evaluation that put
    # it on different sides differ by a whole term in every sum it enters (the small train tests pick a seed without such
    # a value).  Among the 816 M hidden values of these shapes a seed cannot avoid them -- with trained-like betas about one per head
    # and layer flips, in the torch fp32 run as often as in the kernels, and the rule below compares the two.  So the heads' BatchNorm
    # biases put the kink 5 standard deviations away from every channel's mean, alternately above (the channel's ReLU is open but
    # for a few dozen values) and below (closed): both gate states in every head and layer, no value within rounding of the kink.
    with torch.no_grad():
        for hd in hip.node_classifiers:
            for j in (1, 5):
                sign = 1.0 - 2.0 * (torch.arange(hd[j].num_features, device=DEV) % 2)
                hd[j].bias.copy_(5.0 * hd[j].weight.abs() * sign)
    ref32 = copy.deepcopy(hip).train()
    ref64 = copy.deepcopy(hip).double().train()
    cfg, params, _ = hip._classifier_train_cfg()
    P = _stack_head_params([q.detach() for q in params], cfg)
    P.update(seed1=11, seed2=12)
    p1, p2 = P["p1"], P["p2"]
    assert p1 == 0.5 and p2 == 0.5
    running0 = {k: P[k].clone() for k in P if k.startswith("running")}
    # the layer in front of the heads: z, its BatchNorm vectors, the residual; ReLU and dropout on
    lrelu, lp, lseed = True, 0.3, 777
    lmean, linvstd, lgamma, lbeta = _vec("mean"), _vec("invstd"), _vec("gamma"), _vec("beta")
    z, res = _push_off_the_relu_kink(_rows(B * n, 11, 1.5, 0.2), lmean, linvstd, lgamma, lbeta), _rows(B * n, 12)     # (the layer's sums gate on it)
    bn = torch.stack([lmean, linvstd, lgamma * linvstd, lbeta - lmean * lgamma * linvstd]).contiguous()
    # ---- forward, both entry points: the same bits (row_lo = 0: the statistics too)
    h, logits, z1, z2, cbn = ops.classifier_train_fwd_act(z, bn, res, lrelu, lp, lseed, B, n, row_lo, n_valid, P, False)
    after = {k: P[k].clone() for k in running0}
    for k, v in running0.items():
        P[k].copy_(v)
    h0 = ops.bn_act_fwd(z, bn[2].contiguous(), bn[3].contiguous(), res, lrelu, lp, lseed)
    l0, z10, z20, cb0 = ops.classifier_train_fwd(h0, B, n, row_lo, n_valid, P, False)
    assert torch.equal(h0, h) and torch.equal(z10, z1) and torch.equal(z20, z2) and torch.equal(cb0, cbn) and torch.equal(l0, logits)
    for k in running0:
        assert torch.equal(after[k], P[k]), k
    del h0, l0, z10, z20, cb0
    # ---- backward, with the layer's sums and without: the same dh and head gradients bit for bit
    w = _rows(R, 13, cols=4)
    layer = (z, bn, lgamma, lbeta, lrelu, lp, lseed)
    dh, grads, sums = ops.classifier_bwd(w, h, B, n, row_lo, n_valid, P, z1, z2, cbn, True, layer=layer)
    dh_plain, grads_plain = ops.classifier_bwd(w, h, B, n, row_lo, n_valid, P, z1, z2, cbn, True)
    assert sums is not None and torch.equal(dh, dh_plain) and torch.equal(grads, grads_plain)
    del dh_plain, grads_plain
    # ---- recompute=: the buffer-descriptor form only
    if direct:
        for k, v in running0.items():
            P[k].copy_(v)
        hs, ls, z1s, z2s, cbs = ops.classifier_train_fwd_act(z, bn, res, lrelu, lp, lseed, B, n, row_lo, n_valid, P, False, h_sparse=True)
        assert torch.equal(ls, logits) and torch.equal(z1s, z1) and torch.equal(z2s, z2) and torch.equal(cbs, cbn)
        hs.view(B, n, 128)[:, row_lo:row_lo + n_valid, :] = float("nan")            # (never written: whatever the memory holds)
        dh2, grads2, sums2 = ops.classifier_bwd(w, hs, B, n, row_lo, n_valid, P, z1, z2, cbn, True, layer=layer, recompute=(res,))
        assert torch.equal(dh2, dh) and torch.equal(grads2, grads) and torch.equal(sums2, sums)
        del hs, ls, z1s, z2s, cbs, dh2, grads2, sums2
    else:
        ws = _cls_workspace(torch.device(DEV))
        ws.fill_(0x5A)                                                   # (every launch of the heads' backward starts by writing partials here)
        before = ws.clone()
        with pytest.raises(RuntimeError, match="recompute_h needs arrays below 2 GB"):
            ops.classifier_bwd(w, h, B, n, row_lo, n_valid, P, z1, z2, cbn, True, layer=layer, recompute=(res,))
        torch.cuda.synchronize()
        assert torch.equal(ws, before), "nothing may be launched"
        del before
    # ---- the references: torch modules, fp32 and fp64, the kernels' masks
    m1 = _kernel_mask(R, p1, 11)
    m2 = _kernel_mask(R // 2, p2, 12).view(R, 64)
    lmask = _kernel_mask(B * n, lp, lseed).view(B, n, 128)[:, row_lo:row_lo + n_valid, :].reshape(R, 128)
    hv = h.view(B, n, 128)[:, row_lo:row_lo + n_valid, :].reshape(R, 128)
    zv = z.view(B, n, 128)[:, row_lo:row_lo + n_valid, :].reshape(R, 128)
    results = {}
    for name, model, dt in (("fp32", ref32, torch.float32), ("fp64", ref64, torch.float64)):
        hr = hv.detach().to(dt).clone().requires_grad_(True)
        want = _torch_heads(model, hr, m1.to(dt), m2.to(dt))
        (want * w.to(dt)).sum().backward()
        xhat = (zv.to(dt) - lmean.to(dt)) * linvstd.to(dt)
        g = hr.grad * lmask.to(dt) * (xhat * lgamma.to(dt) + lbeta.to(dt) > 0)
        heads = list(model.node_classifiers)
        stats = torch.cat([hd[1].running_mean for hd in heads] + [hd[1].running_var for hd in heads] +
                          [hd[5].running_mean for hd in heads] + [hd[5].running_var for hd in heads])
        results[name] = (want.detach(), hr.grad, [q.grad for hd in heads for q in _seq_params(hd)], stats,
                         torch.cat([g.sum(0), (g * xhat).sum(0)]))
        del hr, want, xhat, g
    a, b = results["fp32"], results["fp64"]
    t = _Table(2, f"heads at (n, row_lo, n_valid, B) = {(n, row_lo, n_valid, B)}: {'buffer-descriptor' if direct else 'flat'} form")
    t.add_tail("logits", logits, a[0], b[0])
    t.add_tail("dh [valid rows]", dh.view(B, n, 128)[:, row_lo:row_lo + n_valid, :].reshape(R, 128), a[1], b[1])
    if n_valid < n:                                        # rows the node-type filter drops get an exactly-zero gradient
        drop = torch.ones(n, dtype=torch.bool, device=DEV)
        drop[row_lo:row_lo + n_valid] = False
        assert (dh.view(B, n, 128)[:, drop, :] == 0).all()
    for i, got in enumerate(_unstack_head_grads(grads)):
        k, j = divmod(i, 10)
        if j in (1, 5):                                    # a bias in front of a train-mode BatchNorm: exact zeros
            assert float(got.abs().max()) == 0
            continue
        t.add(f"head {k} d{_MLP_NAMES[j]}", got, a[2][i].reshape(got.shape), b[2][i].reshape(got.shape))
    got_stats = torch.cat([after[k] for k in ("running_mean1", "running_var1", "running_mean2", "running_var2")])
    for name, sl in (("running_mean1", slice(0, 128)), ("running_var1", slice(128, 256)), ("running_mean2", slice(256, 320)),
                     ("running_var2", slice(320, 384))):
        t.add(name, got_stats[sl], a[3][sl], b[3][sl])
    t.add("layer sums: sum g", sums[:128], a[4][:128], b[4][:128])
    t.add("layer sums: sum g xhat", sums[128:], a[4][128:], b[4][128:])
    t.check(capsys)


# =====================================================================================================================================
# 3. the layer kernels, the eval stack and the node-feature packing at batch 59
# =====================================================================================================================================
FAR_FRAMES = (0, 57, 58)        # frame 58 of 59 is the one whose rows straddle byte 2^31 (58 x 72,020 x 512 B < 2^31 < 59 x ...)


@_big(28)
def test_eval_stack_at_batch_59(capsys):
    """test_gpu_model._full_size_properties at (224, 7, 59): aggregation linearity and symmetry, frames 0, 57 and 58 bit-equal to their
    run alone, frame 58 against the CPU oracle, HIP-graph replay equal to eager -- and the same frames through the model with the
    coordinate graph (the coordinate update's taps at the far frames)."""
    from test_gpu_model import _full_size_properties
    _full_size_properties(224, 7, 59, f=58, alone=(0, 57), coord=True, device_inputs=True)


@_big(32)
def test_layer_train_forward_at_batch_59(capsys):
    """eg_gcn_layer_train_fwd at batch 59 (224 / 7): z and agg of frames 0, 57 and 58 bit-equal to the frame at batch 1; the batch
    statistics and the updated running statistics against fp64 column statistics of z; out against the fp64 formula on z (the
    kernel's own mask); the activation pass in tile order (child sums wanted) writes the same out."""
    import numpy as np
    B, eps, mom, relu, p, seed = 59, 1e-5, 0.1, True, 0.3, 99
    g = ops.Graph.topo(224, 7)
    n = g.num_nodes
    assert (B - 1) * n * 512 < 2 ** 31 < B * n * 512
    rs = np.random.RandomState(224)
    W = torch.from_numpy(rs.uniform(-0.15, 0.15, (128, 128)).astype(np.float32)).to(DEV)
    bias = torch.from_numpy(rs.standard_normal(128).astype(np.float32) * 0.1).to(DEV)
    gamma, beta = _vec("gamma"), _vec("beta")
    x = _rows(B * n, 21)
    rm0, rv0 = _vec("mean"), (1.0 + 0.5 * _vec("beta")).contiguous()
    rm, rv = rm0.clone(), rv0.clone()
    out, z, agg, bn = ops.gcn_layer_train_fwd(g, B, x, W, bias, gamma, beta, rm, rv, mom, eps, relu, p, seed, True)
    for k in FAR_FRAMES:
        _, z1, agg1, _ = ops.gcn_layer_train_fwd(g, 1, x[k * n:(k + 1) * n].contiguous(), W, bias, gamma, beta, None, None, None, eps,
                                                 relu, p, seed, True)
        assert torch.equal(z1, z[k * n:(k + 1) * n]) and torch.equal(agg1, agg[k * n:(k + 1) * n]), k
    ka = ops.new_kidsum(g, B)
    out_t = ops.gcn_layer_train_fwd(g, B, x, W, bias, gamma, beta, None, None, None, eps, relu, p, seed, True, kidsum_out=ka)[0]
    assert torch.equal(out_t, out)
    del out_t, ka, agg
    mask = _kernel_mask(B * n, p, seed)
    rows = B * n

    def ref(dt):
        zz = z.to(dt)
        mean, var = zz.mean(0), zz.var(0, unbiased=False)
        invstd = 1.0 / torch.sqrt(var + eps)
        v = torch.relu((zz - mean) * invstd * gamma.to(dt) + beta.to(dt)) if not p else \
            torch.relu(((zz - mean) * invstd * gamma.to(dt) + beta.to(dt)) * mask.to(dt))
        return (mean, invstd, (1 - mom) * rm0.to(dt) + mom * mean, (1 - mom) * rv0.to(dt) + mom * var * (rows / (rows - 1.0)),
                v + x.to(dt))

    r32, r64 = ref(torch.float32), ref(torch.float64)
    t = _Table(3, f"gcn_layer_train_fwd at batch {B} (224 / 7)")
    t.add("batch mean", bn[0], r32[0], r64[0])
    t.add("batch invstd", bn[1], r32[1], r64[1])
    t.add("running_mean", rm, r32[2], r64[2])
    t.add("running_var", rv, r32[3], r64[3])
    t.add_tail("out", out, r32[4], r64[4])
    for k in FAR_FRAMES:
        t.add(f"out, frame {k}", out[k * n:(k + 1) * n], r32[4][k * n:(k + 1) * n], r64[4][k * n:(k + 1) * n])
    del r32, r64
    t.check(capsys)


@_big(20)
def test_pack_levels_at_batch_59(capsys):
    """eg_pack_levels, sides 2 .. 224, batch 59 (2.17 GB of node rows): the reference's permute / cat, bit for bit, and its gradient."""
    from test_gpu_pack import _reference_pack
    sides, B = [2, 4, 8, 16, 32, 64, 128, 224], 59
    g = torch.Generator(DEV)
    g.manual_seed(59)
    maps = [torch.randn(B, 128, s, s, generator=g, device=DEV).requires_grad_(True) for s in sides]
    n_rows = sum(s * s for s in sides)
    assert B * n_rows * 512 > 2 ** 31
    got = ops.pack_levels(maps, B, n_rows, 0)
    want = _reference_pack(maps, B, n_rows, 0)
    assert torch.equal(got, want)
    assert torch.equal(got[-128:], want[-128:])
    gr = torch.randn(B * n_rows, 128, generator=g, device=DEV)
    for a, b in zip(torch.autograd.grad(got, maps, gr), torch.autograd.grad(want, maps, gr)):
        assert torch.equal(a, b)


@_big(8)
def test_create_node_pixels_at_batch_59(monkeypatch, capsys):
    """create_node_pixels through the fused pyramid (eg_avg_pool_pyramid_* + eg_pack_levels, coordinate rows sampled on top) at batch
    59 against the per-level torch pools (EG_POOL_PYRAMID=0) on frames 0, 57 and 58 alone: 2e-6, the bound of
    test_create_node_pixels_with_the_fused_pyramid_equals_the_torch_pools."""
    import numpy as np
    from fixtures_util import initial_coords
    frame, naux, B = 224, 7, 59
    hip, _ = model_pair(frame, naux, 2, coord=True, seed=3)
    g = torch.Generator(DEV)
    g.manual_seed(9)
    frames = torch.randn(B, 128, frame, frame, generator=g, device=DEV)
    jitter = torch.from_numpy(np.random.RandomState(9).uniform(-20, 20, (B * 4, 2)).astype(np.float32))
    coords = (initial_coords(B, frame) + jitter).clamp(0, frame - 1).to(DEV).reshape(B, 4, 2)
    with torch.no_grad():
        monkeypatch.setenv("EG_POOL_PYRAMID", "1")
        feats = hip.create_node_pixels(frames, B, coords).clone()
        n = feats.shape[0] // B
        assert feats.shape[0] * 512 > 2 ** 31
        monkeypatch.setenv("EG_POOL_PYRAMID", "0")
        for k in FAR_FRAMES:
            want = hip.create_node_pixels(frames[k:k + 1].contiguous(), 1, coords[k:k + 1].contiguous())
            assert want.shape == (n, 128)
            assert float((feats[k * n:(k + 1) * n] - want).abs().max()) < 2e-6, k


# =====================================================================================================================================
# 4. one whole training step at batch 60 = 2 x the batch-30 inputs
# =====================================================================================================================================
@_big(40)
def test_train_step_at_batch_60_is_the_batch_30_step_repeated(monkeypatch, capsys):
    """224 / 7 + coordinate graph, three layers, the criteria of test_cfg4_train_full_batch_32_properties; the second half of the batch
    repeats the first (features and initial coordinates).  With dropout off doubling the batch leaves every BatchNorm mean and biased
    variance, the mean-type loss and every parameter gradient unchanged up to the order and length of the sums -- the same kind of
    perturbation as that test's frame permutation, hence its bounds: loss 1e-5 relative, logits of frame b and b + 30 within 2e-4 of
    the largest logit, coordinates 1e-3, parameter gradients 2e-3 x max + 1e-7, running statistics rtol 1e-4 / atol 1e-5 (with the
    unbiased-variance factor N / (N - 1) of the batch-30 value taken to the batch-60 one).  The batch-30 step takes the recompute route (h written sparsely), the batch-60 step does
    not: the last layer's output is written in full, the heads' backward takes the layer's sums in the flat form and reads h.
    With dropout 0.5 the batch-60 step run twice is bit-identical and finite."""
    import numpy as np
    from fixtures_util import initial_coords
    from gpu_util import graph_tensors
    frame, naux, half = 224, 7, 30
    hip, _ = model_pair(frame, naux, 3, coord=True, seed=17)
    topo = graph_tensors(frame, naux, 1, coord=True)[0]
    n, nv = topo.num_nodes, topo.num_valid_nodes
    assert ops.classifier_recompute_h_supported(half, n, nv) and not ops.classifier_recompute_h_supported(2 * half, n, nv)
    assert ops.classifier_layer_sums_supported(2 * half, n, nv)
    ei1 = torch.from_numpy(topo.edge_index()).to(DEV)
    x30 = _rows(half * n, 31)
    jitter = torch.from_numpy(np.random.RandomState(9).uniform(-20, 20, (half * 4, 2)).astype(np.float32))
    c30 = (initial_coords(half, frame) + jitter).clamp(0, frame - 1).to(DEV)
    routes = []
    fwd_act, bwd = ops.classifier_train_fwd_act, ops.classifier_bwd

    def spy_fwd(*a, **kw):
        routes.append(("fwd", bool(kw.get("h_sparse", False))))
        return fwd_act(*a, **kw)

    def spy_bwd(*a, **kw):
        rec = kw.get("recompute", False)
        routes.append(("bwd", kw.get("layer") is not None, rec is not False and rec is not None))
        return bwd(*a, **kw)
    monkeypatch.setattr(ops, "classifier_train_fwd_act", spy_fwd)
    monkeypatch.setattr(ops, "classifier_bwd", spy_bwd)

    def step(B, feats, coords, seed):
        eid = (ei1[:, None, :] + (torch.arange(B, device=DEV) * n)[None, :, None]).reshape(2, -1).contiguous()
        hip.zero_grad(set_to_none=True)
        torch.manual_seed(seed)
        routes.clear()
        logits, c = hip.forward_nodes(feats, eid, B, coords.clone())
        loss = (logits ** 2).mean() + (c ** 2).mean() * 1e-3
        loss.backward()
        return (logits.detach(), c.detach(), {k: q.grad.detach().clone() for k, q in hip.named_parameters()}, float(loss.detach()),
                {k: v.detach().clone() for k, v in hip.named_buffers() if "running" in k}, list(routes))

    hip.train()
    state = copy.deepcopy(hip.state_dict())
    x60, c60 = torch.cat([x30, x30]), torch.cat([c30, c30])
    # ---- dropout 0.5: the batch-60 step twice
    l1, c1, g1, loss1, _, r1 = step(2 * half, x60, c60, 5)
    hip.load_state_dict(state)
    l2, c2, g2, loss2, _, _ = step(2 * half, x60, c60, 5)
    assert torch.equal(l1, l2) and torch.equal(c1, c2) and loss1 == loss2
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    assert torch.isfinite(l1).all() and torch.isfinite(c1).all() and all(torch.isfinite(v).all() for v in g1.values())
    assert r1 == [("fwd", False), ("bwd", True, False)], r1          # h in full; the layer's sums from the heads' backward; h read, not rebuilt
    del l1, l2, c1, c2, g1, g2
    # ---- dropout off: batch 30 against batch 60
    for m in hip.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    hip.load_state_dict(state)
    la, ca, ga, lossa, sa, ra = step(half, x30, c30, 1)
    hip.load_state_dict(state)
    lb, cb, gb, lossb, sb, rb = step(2 * half, x60, c60, 1)
    assert ra == [("fwd", True), ("bwd", True, True)], ra             # the recompute route
    assert rb == [("fwd", False), ("bwd", True, False)], rb
    assert abs(lossa - lossb) < 1e-5 * abs(lossa)
    lmax = la.abs().max()
    cmax, worst_g = 0.0, 0.0
    for h2 in (0, 1):
        assert (lb.view(2, half * nv, 4)[h2] - la).abs().max() < 2e-4 * lmax
        assert (cb.view(2, half * 4, 2)[h2] - ca).abs().max() < 1e-3
        cmax = max(cmax, float((cb.view(2, half * 4, 2)[h2] - ca).abs().max()))
    for k in ga:
        gm = ga[k].abs().max().item()
        err = (ga[k] - gb[k]).abs().max().item()
        assert err < 2e-3 * gm + 1e-7, (k, err, gm)
        worst_g = max(worst_g, err / (2e-3 * gm + 1e-7))
    # running statistics: the means as they are; a running variance takes the UNBIASED batch variance, whose factor N / (N - 1) is not the
    # same for N and 2 N rows -- 1 / (2 N) apart: nothing for the layers and heads (N = 2.2 M), 4e-3 for the landmark MLPs, whose
    # BatchNorms see 4 rows per frame (N = 120) -- so the batch-30 value is first taken to the batch-60 factor, exactly:
    # rv = (1 - m) rv0 + m var N / (N - 1)
    rows30 = {"gnn_layers": half * n, "node_classifiers": half * nv, "node_coordinate_mlp": 4 * half}
    mods = dict(hip.named_modules())
    for k in sa:
        want = sa[k]
        if k.endswith("running_var"):
            N, m = rows30[k.split(".")[0]], mods[k.rsplit(".", 1)[0]].momentum
            want = (1 - m) * state[k] + (sa[k] - (1 - m) * state[k]) * ((N - 1.0) / N) * (2.0 * N / (2.0 * N - 1.0))
        assert torch.allclose(want, sb[k], rtol=1e-4, atol=1e-5), k
    with capsys.disabled():
        print(f"\n  batch 60 vs batch 30: loss {lossa:.8g} / {lossb:.8g}, logits {float((lb.view(2, half * nv, 4) - la).abs().max() / lmax):.2e} of the "
              f"largest, coordinates {cmax:.2e}, worst gradient err / bound {worst_g:.3f}")
