"""CPU reference of the no-GNN baselines' path behind the UNet decoder (eg_conv1x1_relu_heads_fwd; reference src/core/models.py:707-710,
:726-756, :791-797): relu(Conv2d(C_l, 128, 1)(map_l)) of every level in the requested dtype, the rows of a frame level after level
(h, w row-major), then eval_reference.heads_eval on all of them.  Restated from the formulas; nothing of the library in it."""
import numpy as np
import torch

import eval_reference as E

C = 128
F64, F32 = torch.float64, torch.float32


def tail_rows(feats, weights, biases, B, dtype=F64):
    """-> (rows [B * sum p_l^2, 128] in `dtype`, their scales in float64: the same sums on absolute values)."""
    rows, scales = [], []
    for f, w, b in zip(feats, weights, biases):
        f64, w64 = f.detach().cpu().to(F64).reshape(B, f.shape[1], -1), w.detach().cpu().to(F64).reshape(C, -1)
        fd, wd = f64.to(dtype), w64.to(dtype)
        y = torch.einsum("oc,bcp->bpo", wd, fd)
        s = torch.einsum("oc,bcp->bpo", w64.abs(), f64.abs())
        if b is not None:
            y = y + b.detach().cpu().to(dtype)
            s = s + b.detach().cpu().to(F64).abs()
        rows.append(torch.relu(y))
        scales.append(s)
    return torch.cat(rows, dim=1).reshape(-1, C).contiguous(), torch.cat(scales, dim=1).reshape(-1, C).contiguous()


def tail_heads(feats, weights, biases, B, packed, sigmoid=False, dtype=F64):
    """-> (logits or sigmoid(logits) [B * sum p_l^2, 4] in `dtype`, scale in float64)."""
    rows, scale = tail_rows(feats, weights, biases, B, dtype)
    n = rows.shape[0] // B
    return E.heads_eval(packed, rows, B, n, 0, n, sigmoid, dtype, h_scale=scale)


def level_inputs(sides, chans, B, seed, bias=True):
    """Decoder maps ~ N(0, 1), Glorot-uniform 1 x 1 weights, biases ~ 0.1 N(0, 1): float32, CPU."""
    rs = np.random.RandomState(seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    feats = [t(rs.standard_normal((B, c, p, p))) for p, c in zip(sides, chans)]
    weights = [t(rs.uniform(-1, 1, (C, c)) * np.sqrt(6.0 / (c + C))) for c in chans]
    biases = [t(0.1 * rs.standard_normal(C)) if bias else None for _ in chans]
    return feats, weights, biases


# ---------------------------------------------------------------------------
# one training step of the no-GNN model, restated with the model's own torch modules
# ---------------------------------------------------------------------------
def train_restatement(model, x, B, dlogits, dtype=F64, maps=None):
    """models.py:759-799 in training mode on a CPU copy of `model` in `dtype`: decoder_maps (its torch modules), F.relu(linears[i](.)),
    permute / cat per frame, node_classifiers[c], loss = sum(logits * dlogits).  maps: the decoder's maps, given (x is not read then: the
    step behind the decoder, whose inputs are the same numbers on every host).  -> dict with
      logits, grads {name: gradient} of linears.* and node_classifiers.*, unused: the names of parameters without a gradient,
      pre: every tensor a ReLU is applied to (decoder convolutions, the tail's 1 x 1 convolutions, the heads' BatchNorm outputs),
      logits_scale / scales {name: ...}: the LAST reduction of each quantity on absolute values (|A| |W|^T + |b| for the logits,
      |dZ|^T |A| for a weight, sum |dZ| for a bias or beta, sum |dZ| |xhat| for gamma), the scale Report.check takes."""
    import copy
    import torch.nn.functional as Fn
    m = copy.deepcopy(model).cpu().to(dtype).train()
    m.hip_frontend = m.hip_frontend_train = m.hip_tail = False
    for mod in m.modules():
        if isinstance(mod, torch.nn.ReLU):
            mod.inplace = False
    pre, seen = [], {}

    def watch(name, mod, relu_follows):
        def hook(_, inp, out):
            if relu_follows:
                pre.append(out.detach().clone())
            if name is not None:
                rec = seen[name] = {"in": inp[0].detach(), "mod": mod}
                out.register_hook(lambda g: rec.__setitem__("g", g.detach()))
        mod.register_forward_hook(hook)
    for blk in list(m.down_convs) + list(m.up_convs):
        watch(None, blk.conv1, True)
        watch(None, blk.conv2, True)
    for i, lin in enumerate(m.linears):
        watch(f"linears.{i}", lin, True)
    for c, clf in enumerate(m.node_classifiers):
        for k in (0, 1, 4, 5, 8):
            watch(f"node_classifiers.{c}.{k}", clf[k], k in (1, 5))
    feats = m.decoder_maps(x.detach().cpu().to(dtype)) if maps is None else [f.detach().cpu().to(dtype) for f in maps]
    maps = [Fn.relu(lin(f)) for lin, f in zip(m.linears, feats)]
    rows = torch.cat([mp[i].permute(1, 2, 0).reshape(-1, C) for i in range(B) for mp in maps], dim=0)
    logits = torch.cat([clf(rows) for clf in m.node_classifiers], dim=1)
    (logits * dlogits.detach().cpu().to(dtype)).sum().backward()
    named = dict(m.named_parameters())
    grads = {n: p.grad for n, p in named.items() if p.grad is not None and n.startswith(("linears.", "node_classifiers."))}
    scales, last = {}, []
    for name, rec in seen.items():
        a, g, mod = rec["in"].to(F64).abs(), rec["g"].to(F64).abs(), rec["mod"]
        if isinstance(mod, torch.nn.Conv2d):
            scales[name + ".weight"] = torch.einsum("bop,bcp->oc", g.flatten(2), a.flatten(2)).reshape(mod.weight.shape)
            scales[name + ".bias"] = g.sum(dim=(0, 2, 3))
        elif isinstance(mod, torch.nn.Linear):
            scales[name + ".weight"] = g.t() @ a
            scales[name + ".bias"] = g.sum(0)
            if name.endswith(".8"):
                last.append(a @ mod.weight.detach().to(F64).abs().t() + mod.bias.detach().to(F64).abs())
        else:
            z = rec["in"].to(F64)
            xhat = (z - z.mean(0)) / torch.sqrt(z.var(0, unbiased=False) + mod.eps)
            scales[name + ".weight"] = (g * xhat.abs()).sum(0)
            scales[name + ".bias"] = g.sum(0)
    return {"logits": logits.detach(), "grads": grads, "unused": sorted(n for n, p in named.items() if p.grad is None), "pre": pre,
            "logits_scale": torch.cat(last, dim=1), "scales": scales}
