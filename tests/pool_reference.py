"""A plain reference of the average-pool pyramid (csrc/pool.hip) and of the node packing with and without the 1 x 1 convolution
(csrc/pack.hip): torch on the CPU, no kernels.  Every function takes ``dtype``: float64 is the truth, the same code in float32 a
yardstick.  The kernels' float32 inputs convert to double exactly.

adaptive_avg_pool2d of an F x F plane to p x p is  P X P^T  with the p x F matrix P whose row i holds 1 / len on
[floor(i F / p), ceil((i + 1) F / p)); its gradient is  P^T G P.  The rounding error of such a sum, taken in any order, is bounded
by a multiple of the same expression on the magnitudes (`*_scale`): that is the per-output scale of coord_reference.Report.check."""
import torch

C = 128
F64 = torch.float64
LDS_FLOATS = 8192                      # PP_LDS_FLOATS of csrc/pool.hip


# ---------------------------------------------------------------------------
# the pooling matrix
# ---------------------------------------------------------------------------
def window(F: int, p: int, i: int):
    """[start, end) of window i of p over F."""
    return i * F // p, -((-(i + 1) * F) // p)


def pool_matrix(F: int, p: int, dtype=F64) -> torch.Tensor:
    """[p, F]: row i holds 1 / len on [floor(i F / p), ceil((i + 1) F / p))."""
    assert 1 <= p <= F
    m = torch.zeros(p, F, dtype=dtype)
    for i in range(p):
        s, e = window(F, p, i)
        m[i, s:e] = 1.0 / (e - s)
    return m


def pool_fwd(x: torch.Tensor, sides, dtype=F64):
    """[P_p X P_p^T for p in sides] of x [..., F, F]."""
    x = x.detach().to(dtype)
    F = x.shape[-1]
    out = []
    for p in sides:
        m = pool_matrix(F, p, dtype)
        out.append(m @ x @ m.t())
    return out


def pool_fwd_scale(x: torch.Tensor, sides):
    """P |X| P^T in float64: the sum of the magnitudes of every output's summands."""
    return pool_fwd(x.detach().to(F64).abs(), sides, F64)


def pool_bwd(grads, frame_grad, sides, shape, dtype=F64) -> torch.Tensor:
    """dx = g_frame + sum_l P_l^T G_l P_l of the level gradients [..., p_l, p_l] (None: the level is skipped) and the frame's own
    gradient [..., F, F] (None: nothing is added), the result of `shape` [..., F, F]."""
    F = shape[-1]
    dx = torch.zeros(tuple(shape), dtype=dtype) if frame_grad is None else frame_grad.detach().to(dtype).reshape(tuple(shape)).clone()
    for g, p in zip(grads, sides):
        if g is None:
            continue
        m = pool_matrix(F, p, dtype)
        dx = dx + m.t() @ g.detach().to(dtype) @ m
    return dx


def pool_bwd_scale(grads, frame_grad, sides, shape) -> torch.Tensor:
    """|g_frame| + sum_l P_l^T |G_l| P_l in float64."""
    return pool_bwd([None if g is None else g.detach().to(F64).abs() for g in grads],
                    None if frame_grad is None else frame_grad.detach().to(F64).abs(), sides, shape, F64)


# ---------------------------------------------------------------------------
# which route a level takes
# ---------------------------------------------------------------------------
def plan(F: int, sides):
    """For the strictly ascending `sides` of one eg_avg_pool_pyramid_fwd call, per level FINE TO COARSE, one tuple:
    (side, "direct") -- summed from the plane by k_pool_direct -- or (side, "derived", source, kept): the mean of 2 x 2 values of
    the level in front of it (k_pool_derived), read from `source` = "lds" or "global", and `kept` in LDS for the next level.

    The host rule, csrc/pool.hip, eg_avg_pool_pyramid_fwd ("the finer level's windows tile the plane exactly and pair up"):
        derive[l] = l > 0 && side[l - 1] == 2 * side[l] && frame % side[l - 1] == 0
    and in k_pool_derived
        keep = l + 1 < n_levels && derive[l + 1] && p * p <= PP_LDS_FLOATS;   have = keep (of the level before; a direct level
    in between resets it: `if (!a.derive[l]) { have = false; continue; }`)."""
    s = [int(p) for p in sides][::-1]
    assert all(a > b for a, b in zip(s, s[1:])) and s[0] <= F and s[-1] >= 1
    derive = [l > 0 and s[l - 1] == 2 * s[l] and F % s[l - 1] == 0 for l in range(len(s))]
    out, have = [], False
    for l, p in enumerate(s):
        if not derive[l]:
            out.append((p, "direct"))
            have = False
            continue
        keep = l + 1 < len(s) and derive[l + 1] and p * p <= LDS_FLOATS
        out.append((p, "derived", "lds" if have else "global", keep))
        have = keep
    return out


# ---------------------------------------------------------------------------
# packing: the reference's permute / cat
# ---------------------------------------------------------------------------
def pack_rows(maps, batch: int, n_rows: int, row_offset: int) -> torch.Tensor:
    """models.py:511-537 / :726-756: per frame, map[i].permute(1, 2, 0).reshape(-1, 128) of every level [batch, 128, p, p],
    concatenated, at rows row_offset.. of the frame's n_rows; every other row zero -> [batch * n_rows, 128]."""
    out = torch.zeros(batch, n_rows, C, dtype=maps[0].dtype, device=maps[0].device)
    for i in range(batch):
        x = torch.cat([m[i].permute(1, 2, 0).reshape(-1, C) for m in maps], dim=0)
        out[i, row_offset:row_offset + x.shape[0]] = x
    return out.reshape(batch * n_rows, C)


def unpack_rows(nodes: torch.Tensor, sides, batch: int, n_rows: int, row_offset: int):
    """The inverse: [batch * n_rows, 128] -> the level maps [batch, 128, p, p] of `sides`."""
    v = nodes.reshape(batch, n_rows, C)
    maps, row = [], row_offset
    for p in sides:
        maps.append(v[:, row:row + p * p].reshape(batch, p, p, C).permute(0, 3, 1, 2).contiguous())
        row += p * p
    return maps


# ---------------------------------------------------------------------------
# 1 x 1 convolution + ReLU in front of the packing
# ---------------------------------------------------------------------------
def conv_pack64(feats, weights, biases, batch: int, n_rows: int, row_offset: int, dnodes=None, dtype=F64):
    """relu(W_l x + b_l) of every level (feats[l] [batch, c_l, p, p], weights[l] [128, c_l], biases[l] [128] or None), packed like
    pack_rows -> {"out" [batch * n_rows, 128], "s": the pre-activations per level [batch, 128, p, p], "scale": |W||x| + |b| packed}.
    With an upstream gradient dnodes [batch * n_rows, 128] also "dfeat", "dw", "db" (None where there is no bias), lists per level,
    and "dfeat_scale", "dw_scale", "db_scale": the sums of the magnitudes of the products each entry is summed from."""
    sides = [int(f.shape[2]) for f in feats]
    xs = [f.detach().to(dtype) for f in feats]
    ws = [w.detach().to(dtype).reshape(C, -1) for w in weights]
    bs = [None if b is None else b.detach().to(dtype).reshape(C) for b in biases]
    s = [torch.einsum("oc,bcij->boij", w, x) + (0 if b is None else b.view(1, C, 1, 1)) for x, w, b in zip(xs, ws, bs)]
    scale = [torch.einsum("oc,bcij->boij", w.to(F64).abs(), x.to(F64).abs()) + (0 if b is None else b.to(F64).abs().view(1, C, 1, 1))
             for x, w, b in zip(xs, ws, bs)]
    res = dict(out=pack_rows([torch.relu(t) for t in s], batch, n_rows, row_offset), s=s, scale=pack_rows(scale, batch, n_rows, row_offset))
    if dnodes is None:
        return res
    g = unpack_rows(dnodes.detach().to(dtype), sides, batch, n_rows, row_offset)
    dz = [gl * (t > 0).to(dtype) for gl, t in zip(g, s)]
    res["dfeat"] = [torch.einsum("oc,boij->bcij", w, d) for w, d in zip(ws, dz)]
    res["dw"] = [torch.einsum("boij,bcij->oc", d, x) for d, x in zip(dz, xs)]
    res["db"] = [None if b is None else d.sum((0, 2, 3)) for b, d in zip(bs, dz)]
    a = [d.to(F64).abs() for d in dz]
    res["dfeat_scale"] = [torch.einsum("oc,boij->bcij", w.to(F64).abs(), d) for w, d in zip(ws, a)]
    res["dw_scale"] = [torch.einsum("boij,bcij->oc", d, x.to(F64).abs()) for d, x in zip(a, xs)]
    res["db_scale"] = [None if b is None else d.sum((0, 2, 3)) for b, d in zip(bs, a)]
    return res


def relu_margin(s64, s32):
    """(the float32 mask is the float64 mask, min|s64| / max|s32 - s64|) over the pre-activations of all levels: what decides
    whether two float32 evaluations can put a pre-activation on different sides of the ReLU's kink."""
    same = all(torch.equal(a > 0, b > 0) for a, b in zip(s64, s32))
    lo = min(float(a.abs().min()) for a in s64)
    err = max(float((b.to(F64) - a).abs().max()) for a, b in zip(s64, s32))
    return same, lo / max(err, 1e-300)


# ---------------------------------------------------------------------------
# the conv-pack cases: inputs, torch's own float32 result, and the seeds under which the ReLU's mask is safe
# ---------------------------------------------------------------------------
BIAS_MODES = ("all", "none", "mixed")          # mixed: the even levels have a bias
MARGIN = 64


def conv_fixture(sides, chans, batch, front, back, bias, seed):
    """float32 CPU inputs of one conv-pack case: standard normal features, weights N(0, 1 / c_l), biases N(0, 1 / 4), an upstream
    gradient for every node row."""
    import numpy as np
    rs = np.random.RandomState(seed)
    f32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.float32))
    feats = [f32(rs.standard_normal((batch, c, p, p))) for p, c in zip(sides, chans)]
    weights = [f32(rs.standard_normal((C, c)) / np.sqrt(c)) for c in chans]
    drawn = [f32(0.5 * rs.standard_normal(C)) for _ in chans]
    biases = [b if bias == "all" or (bias == "mixed" and l % 2 == 0) else None for l, b in enumerate(drawn)]
    n_rows = front + sum(p * p for p in sides) + back
    return dict(feats=feats, weights=weights, biases=biases, batch=batch, n_rows=n_rows, row_offset=front, sides=list(sides),
                dnodes=f32(rs.standard_normal((batch * n_rows, C))))


def conv_torch32(fx, device="cpu", dtype=torch.float32):
    """What the kernel replaces: relu(conv2d) per level and the reference's permute / cat, with torch's autograd, in float32 on the
    CPU -> the keys of conv_pack64 (without the scales)."""
    leaf = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype).requires_grad_(True)
    feats, ws, bs = [leaf(t) for t in fx["feats"]], [leaf(t) for t in fx["weights"]], [leaf(t) for t in fx["biases"]]
    s = [torch.nn.functional.conv2d(f, w.view(C, -1, 1, 1), b) for f, w, b in zip(feats, ws, bs)]
    out = pack_rows([torch.relu(t) for t in s], fx["batch"], fx["n_rows"], fx["row_offset"])
    ins = feats + ws + [b for b in bs if b is not None]
    grads = list(torch.autograd.grad(out, ins, fx["dnodes"].to(device=device, dtype=dtype)))
    n = len(feats)
    db = iter(grads[2 * n:])
    return dict(out=out.detach(), s=[t.detach() for t in s], dfeat=grads[:n], dw=grads[n:2 * n], db=[None if b is None else next(db) for b in bs])


def conv_margin(fx):
    """(float32 mask == float64 mask, min|s64| / max|s32 - s64|) of a fixture, on the references alone."""
    r64 = conv_pack64(fx["feats"], fx["weights"], fx["biases"], fx["batch"], fx["n_rows"], fx["row_offset"])
    return relu_margin(r64["s"], conv_torch32(fx)["s"])


# (sides, chans, batch, front, back) of tests/test_gpu_pool_pack_fp64.py and of tests/test_gpu_pack.py's small cases
CONV_CASES = [((2, 3, 8), (32, 31, 64), 2, 0, 0), ((1, 4, 17), (1, 33, 5), 1, 2, 3), ((6,), (512,), 2, 0, 1)]
CONV_CASES_PACK = [((2, 4, 30), (40, 7, 3), 2, 4, 4), ((17,), (1,), 2, 0, 0), ((1, 3, 65), (33, 64, 5), 1, 2, 0)]
