"""A plain reference of the coordinate-graph path (resampling, tap sums, landmark MLP, the fused update): torch on the CPU, float64
by default, no kernels.  The kernels' fp32 inputs are converted to double (exactly), so every floor / kink / clamp decision is taken
on the kernels' own numbers.  Every function takes ``dtype``: the same code in float32 is "what the oracle would compute", the
yardstick of the tolerance rule below (tests/test_gpu_train.py::test_cfg4_train_step_error_against_fp64_is_the_references_own).

Tolerance rule (`Report.check`):  |kernel - fp64| <= FACTOR * max|ref32 - fp64| + 8 * 2^-23 * scale, with
  scale = the largest magnitude of the quantity                       (elementwise quantities: samples, d h, d lm, new), or
  scale = the sum of the absolute values of the summands, per output  (reductions: d coords, tap sums, parameter gradients, statistics).
The rounding error of a sum taken in any order is bounded by a multiple of the second number; a small result that comes from
cancellation must not tighten the tolerance."""
import copy

import numpy as np
import torch

from oracle import gnn_oracle as O

C = 128
ULP = 2.0 ** -23
FACTOR = 4.0
F64 = torch.float64


# ---------------------------------------------------------------------------
# inputs: positions where the resampling can go wrong
# ---------------------------------------------------------------------------
def hand_positions(F: int):
    """Groups of (h, w) positions in a frame of side F; the positions of one group belong into ONE frame (they collide).
    Corners, edge midpoints, integer and half-integer positions, -0.0, a bit-identical pair, two in one cell, pairs in
    horizontally / vertically / diagonally adjacent cells (two, two and one shared tap rows), just inside and just outside each border,
    one coordinate inside and the other outside."""
    f32 = np.float32
    e = float(F - 1)
    u, v = float(f32(e * 0.37)), float(f32(e * 0.61))
    i, j = float(np.floor(u)), float(np.floor(v))
    groups = [[(0.0, 0.0)], [(0.0, e)], [(e, 0.0)], [(e, e)],
              [(0.0, e / 2)], [(e / 2, 0.0)], [(e, e / 2)], [(e / 2, e)],
              [(float(F // 2), float(F // 3))], [(F // 2 + 0.5, F // 3 + 0.5)],
              [(-0.0, -0.0)], [(-0.0, min(1.0, e))],
              [(u, v), (u, v)],
              [(i + 0.2, j + 0.3), (i + 0.7, j + 0.6)],
              [(i + 0.4, j + 0.5), (i + 0.6, j + 1.5)],
              [(i + 0.4, j + 0.5), (i + 1.6, j + 0.3)],
              [(i + 0.4, j + 0.5), (i + 1.5, j + 1.5)]]
    for b in (-1.0, float(np.nextafter(f32(-1), f32(0))), -0.5, e, F - 0.5, float(F), F + 3.0):
        groups += [[(b, u)], [(v, b)]]
    groups += [[(-2.5, v)], [(u, F + 7.25)]]
    return groups


def position_rounds(F: int, points: int, B: int, seed: int):
    """float32 arrays [B, points, 2], as many as it takes to hold every group of hand_positions(F) once, the rest of every array
    a seeded random fill on (-1.5, F + 0.5).  A group larger than `points` is split (with one point per frame nothing collides)."""
    frames, cur = [], []
    for g in hand_positions(F):
        g = list(g)
        while g:
            if len(cur) + min(len(g), points) > points:
                frames.append(cur)
                cur = []
            take = g[:points - len(cur)] if len(g) > points else g
            cur += take
            g = g[len(take):]
    if cur:
        frames.append(cur)
    rs = np.random.RandomState(seed)
    rounds = []
    for k in range(0, len(frames), B):
        c = rs.uniform(-1.5, F + 0.5, (B, points, 2)).astype(np.float32)
        for b, fr in enumerate(frames[k:k + B]):
            # hand-placed positions go to the END of a frame's points in the odd rounds: the forwarding meets them in both orders
            at = points - len(fr) if (k // B) % 2 else 0
            c[b, at:at + len(fr)] = np.asarray(fr, dtype=np.float32)
        rounds.append(c)
    return rounds


# ---------------------------------------------------------------------------
# the dropout mask of the kernels (train_common.h): a pure function of (seed, element index)
# ---------------------------------------------------------------------------
def hash_mask(rows: int, width: int, p: float, seed: int) -> torch.Tensor:
    """The keep mask [rows, width] float32 (0 or 1 / (1 - p)) of element index row * width + column, from the hash written out in
    numpy: element e keeps iff the 16-bit field (e & 3) of splitmix64(seed + (e >> 2) * golden) is >= floor(65536 p)."""
    n = rows * width
    if p <= 0:
        return torch.ones(rows, width)
    with np.errstate(over="ignore"):
        e = np.arange(n, dtype=np.uint64)
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (e >> np.uint64(2)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    field = (z >> (np.uint64(16) * (e & np.uint64(3)))) & np.uint64(0xFFFF)
    thr = np.uint64(int(np.float32(p) * np.float32(65536.0)))
    ik = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return torch.from_numpy(np.where(field >= thr, ik, np.float32(0)).astype(np.float32)).view(rows, width)


def kernel_mask(rows: int, width: int, p: float, seed: int) -> torch.Tensor:
    """The same mask read back from the kernels (eg_bn_act_fwd on an all-ones input, rows * width elements in rows of 128), on
    the CPU.  Needs the GPU."""
    from echoglad_amd import ops
    n = rows * width
    one, zero = torch.ones(C, device="cuda:0"), torch.zeros(C, device="cuda:0")
    m = ops.bn_act_fwd(torch.ones((n + C - 1) // C, C, device="cuda:0"), one, zero, None, False, p, seed)
    return m.reshape(-1)[:n].view(rows, width).cpu()


# ---------------------------------------------------------------------------
# resampling
# ---------------------------------------------------------------------------
def _main_maps(h, B, n, main_base, F):
    return h.view(B, n, C)[:, main_base:main_base + F * F, :].permute(0, 2, 1).reshape(B, C, F, F)


def sample64(h, coords, B, n, main_base, F, points, dout=None, dtype=F64):
    """The dense hat-weight formula (oracle.gnn_oracle.bilinear_interpolation_dense) on the main grid of every frame of h [B * n, 128]
    at coords [B * points, 2] -> {"out" [B * points, 128]}; with an upstream gradient dout [B * points, 128] also "dh" [B * n, 128]
    (zero outside the main grid), "dcoords" [B * points, 2], and the scales: "dcoords_scale" = the sum of the absolute values of the
    summands of every d coords, "add_abs" [B, F * F, 128] = the same for the increments of dh (the tap sums' summands)."""
    want = dout is not None
    h = h.detach().to(dtype).clone().requires_grad_(want)
    c = torch.as_tensor(coords).detach().to(dtype).reshape(B * points, 2).clone().requires_grad_(want)
    main = _main_maps(h, B, n, main_base, F)
    out = torch.cat([O.bilinear_interpolation_dense(c[points * b:points * (b + 1)], main[b]) for b in range(B)])
    res = {"out": out.detach()}
    if not want:
        return res
    g = dout.detach().to(dtype).reshape(B * points, C)
    dh, dc = torch.autograd.grad(out, (h, c), g)
    res.update(dh=dh, dcoords=dc)
    with torch.no_grad():
        d = c.detach()[:, :, None] - torch.arange(F, dtype=dtype)                # [P, 2, F]
        w = torch.relu(1 - d.abs())
        a = ((d.abs() < 1) & (d != 0)).to(dtype)                                  # |d w / d c|
        mp = main.detach().abs().repeat_interleave(points, 0)                     # [P, C, F, F]
        gm = torch.einsum("pc,pcij->pij", g.abs(), mp)
        res["dcoords_scale"] = torch.stack([torch.einsum("pij,pi,pj->p", gm, a[:, 0], w[:, 1]),
                                            torch.einsum("pij,pi,pj->p", gm, w[:, 0], a[:, 1])], 1)
        wt = (w[:, 0, :, None] * w[:, 1, None, :]).reshape(B, points, F * F)
        res["add_abs"] = torch.einsum("bpc,bpk->bkc", g.abs().view(B, points, C), wt)
    return res


def tap_sums64(add, z, mean, invstd, scale, shift, relu, keep, dtype=F64, absolute=False):
    """What the increments `add` [B, rows, 128] of a dy add to its BatchNorm-backward sums, per frame and channel -> [B, 2, 128]:
    s1 = sum add keep gate, s2 = sum add keep gate (z - mean) invstd, gate = (z scale + shift > 0) with relu, else 1.
    z, keep [B, rows, 128]; mean, invstd, scale, shift [128].  absolute: the sums of the summands' magnitudes (the scale)."""
    add, z, keep = add.to(dtype), z.to(dtype), keep.to(dtype)
    mean, invstd, scale, shift = (t.to(dtype) for t in (mean, invstd, scale, shift))
    t = add * keep
    if relu:
        t = t * (z * scale + shift > 0).to(dtype)
    xh = (z - mean) * invstd
    if absolute:
        t, xh = t.abs(), xh.abs()
    return torch.stack([t.sum(1), (t * xh).sum(1)], 1)


# ---------------------------------------------------------------------------
# the landmark MLP
# ---------------------------------------------------------------------------
def mlp_params(m):
    """The 10 parameters of a 136-32-16-2 head in the order of the packed gradients (include/echoglad_hip.h)."""
    return [m[0].weight, m[0].bias, m[1].weight, m[1].bias, m[4].weight, m[4].bias, m[5].weight, m[5].bias, m[8].weight, m[8].bias]


PARAM_NAMES = ("w1", "b1", "gamma1", "beta1", "w2", "b2", "gamma2", "beta2", "w3", "b3")


def mlp64(mlp, lm, coords, B, F, mask1=None, mask2=None, dtype=F64):
    """models.py:441-453 with the oracle's _mlp_head modules (a copy, in `dtype`, train mode), the keep masks [4B,32] / [4B,16]
    (0 or 1 / (1 - p)) in place of Dropout: pairwise offsets, the head, coords + delta, clamp to [0, F - 1].  Everything stays on the
    autograd graph; `mlp_backward` takes the gradients.  The copy's BatchNorm modules hold the updated running statistics."""
    m = copy.deepcopy(mlp).to(dtype).train()
    R = 4 * B
    lm_ = lm.detach().to(dtype).reshape(R, C).clone().requires_grad_(True)
    c_ = torch.as_tensor(coords).detach().to(dtype).reshape(B, 4, 2).clone().requires_grad_(True)
    sf = (c_.unsqueeze(1) - c_.unsqueeze(2)).reshape(R, 8)
    x = torch.cat((lm_, sf), 1)
    z1 = m[0](x)
    y1 = m[1](z1)
    h1 = torch.relu(y1)
    if mask1 is not None:
        h1 = h1 * mask1.to(dtype)
    z2 = m[4](h1)
    y2 = m[5](z2)
    h2 = torch.relu(y2)
    if mask2 is not None:
        h2 = h2 * mask2.to(dtype)
    pre = (c_ + m[8](h2).view(B, 4, 2)).view(R, 2)
    new = torch.clamp(pre, min=0, max=F - 1)
    return dict(module=m, lm=lm_, coords=c_, x=x, z1=z1, y1=y1, h1=h1, z2=z2, y2=y2, h2=h2, pre=pre, new=new, F=F)


def input_condition(fw):
    """(smallest BatchNorm output magnitude of both hidden layers, smallest distance of a pre-clamp value to 0 or F - 1, share of
    clamped coordinates): what decides whether two evaluations can take different sides of a kink."""
    pre, e = fw["pre"].detach(), fw["F"] - 1
    return (min(float(fw["y1"].detach().abs().min()), float(fw["y2"].detach().abs().min())),
            float(torch.minimum(pre.abs(), (pre - e).abs()).min()), float(((pre < 0) | (pre > e)).double().mean()))


def _xhat(z, bn):
    return (z - z.mean(0)) / torch.sqrt(z.var(0, unbiased=False) + bn.eps)


def mlp_backward(fw, dnew, dnew_abs=None):
    """Every gradient of mlp64's `new` under the upstream gradient dnew [4B,2] -> {"dlm", "dcoords", "grads" [5042] packed,
    "dd" = d pre} and the reductions' scales {"dcoords_scale", "grads_scale" [5042]}.  dnew_abs: the sum of the magnitudes of dnew's own
    summands where dnew is itself a sum (the fused update: dnew + d_bil)."""
    m, dtype = fw["module"], fw["new"].dtype
    R = fw["new"].shape[0]
    params = mlp_params(m)
    inter = [fw["z1"], fw["y1"], fw["z2"], fw["y2"], fw["pre"]]
    dnew = dnew.detach().to(dtype).reshape(R, 2)
    g = torch.autograd.grad(fw["new"], [fw["lm"], fw["coords"]] + params + inter, dnew, retain_graph=True)
    dlm, dc, pg = g[0], g[1].reshape(R, 2), g[2:12]
    dz1, dy1, dz2, dy2, dd = (t.detach() for t in g[12:])
    res = dict(dlm=dlm, dcoords=dc, grads=torch.cat([t.reshape(-1) for t in pg]), dd=dd)
    with torch.no_grad():
        pre, e = fw["pre"].detach(), fw["F"] - 1
        dd_abs = (dnew.abs() if dnew_abs is None else dnew_abs.to(dtype).reshape(R, 2)) * ((pre >= 0) & (pre <= e)).to(dtype)
        x, h1, h2 = fw["x"].detach().abs(), fw["h1"].detach().abs(), fw["h2"].detach().abs()
        xh1, xh2 = _xhat(fw["z1"].detach(), m[1]), _xhat(fw["z2"].detach(), m[5])
        zero1, zero2 = torch.zeros(32, dtype=dtype), torch.zeros(16, dtype=dtype)
        scales = [dz1.abs().t() @ x, zero1, (dy1 * xh1).abs().sum(0), dy1.abs().sum(0),
                  dz2.abs().t() @ h1, zero2, (dy2 * xh2).abs().sum(0), dy2.abs().sum(0),
                  dd_abs.t() @ h2, dd_abs.sum(0)]
        res["grads_scale"] = torch.cat([t.reshape(-1) for t in scales])
        S = (dz1.abs() @ m[0].weight.detach()[:, C:].abs()).view(R // 4, 4, 4, 2)            # [f, row j, other k, d]
        # d coords[(f, m), d] = dd + sum_j dsf[(f, j), (m, d)] - sum_k dsf[(f, m), (k, d)]
        res["dcoords_scale"] = (dd_abs.view(R // 4, 4, 2) + S.sum(1) + S.sum(2)).reshape(R, 2)
    return res


def running_stats(fw):
    """The four running statistics after the forward and the scales of their sums: (values, scales), each a list of
    running_mean1, running_var1, running_mean2, running_var2."""
    m = fw["module"]
    vals, scales = [], []
    for bn, z in ((m[1], fw["z1"].detach()), (m[5], fw["z2"].detach())):
        mom = bn.momentum
        vals += [bn.running_mean.detach().clone(), bn.running_var.detach().clone()]
        # (new = (1 - mom) old + mom stat: the old value is recovered from the new one, the module has been updated in place)
        scales += [(bn.running_mean - mom * z.mean(0)).abs() + mom * z.abs().mean(0), bn.running_var.detach().abs()]
    return vals, scales


# ---------------------------------------------------------------------------
# the fused update (eg_coord_update_fwd / _bwd)
# ---------------------------------------------------------------------------
def update64(mlp, h, coords, B, n, coord_base, main_base, F, mask1=None, mask2=None, dx=None, dnew=None, lower=None, dtype=F64):
    """Forward: mlp64 on the 4 coordinate rows of every frame of h [B * n, 128], then those rows overwritten with the main grid sampled
    at the new positions -> "h" (after), "new", "fw" (mlp64's record).
    Backward (dx [B * n, 128] = the gradient w.r.t. the tensor after the update; dnew [4B,2] | None from downstream): the main-grid rows
    gain the taps, d new = dnew + d_bil, the coordinate rows leave as d lm -> "dx" (w.r.t. the tensor before), "dcoords", "grads" [5042],
    "dbil", "add" [B, F * F, 128] = what the main-grid rows gained; with lower = (z [B * n, 128], bn [4,128] = mean, invstd, scale, shift,
    relu, keep [B * n, 128]) also "taps" [B,2,128]; and the scales "dcoords_scale", "grads_scale", "dbil_scale", "add_abs", "taps_scale"."""
    hv = h.detach().to(dtype)
    rows = hv.view(B, n, C)[:, coord_base:coord_base + 4, :].reshape(4 * B, C)
    fw = mlp64(mlp, rows, coords, B, F, mask1, mask2, dtype)
    new = fw["new"].detach()
    dout = None if dx is None else dx.detach().to(dtype).view(B, n, C)[:, coord_base:coord_base + 4, :].reshape(4 * B, C)
    s = sample64(hv, new, B, n, main_base, F, 4, dout=dout, dtype=dtype)
    after = hv.clone()
    after.view(B, n, C)[:, coord_base:coord_base + 4, :] = s["out"].view(B, 4, C)
    res = dict(h=after, new=new, fw=fw)
    if dx is None:
        return res
    dbil = s["dcoords"]
    total = dbil if dnew is None else dbil + dnew.detach().to(dtype).reshape(4 * B, 2)
    total_abs = s["dcoords_scale"] if dnew is None else s["dcoords_scale"] + dnew.detach().to(dtype).reshape(4 * B, 2).abs()
    bw = mlp_backward(fw, total, total_abs)
    dxo = dx.detach().to(dtype) + s["dh"]
    dxo.view(B, n, C)[:, coord_base:coord_base + 4, :] = bw["dlm"].view(B, 4, C)
    sl = slice(main_base, main_base + F * F)
    res.update(dx=dxo, dcoords=bw["dcoords"], grads=bw["grads"], dbil=dbil, dcoords_scale=bw["dcoords_scale"],
               grads_scale=bw["grads_scale"], dbil_scale=s["dcoords_scale"], add=s["dh"].view(B, n, C)[:, sl], add_abs=s["add_abs"])
    if lower is not None:
        z, bn, relu, keep = lower
        bn = bn.reshape(4, C)
        args = (z.view(B, n, C)[:, sl], bn[0], bn[1], bn[2], bn[3], relu, keep.view(B, n, C)[:, sl])
        res["taps"] = tap_sums64(s["dh"].view(B, n, C)[:, sl], *args, dtype=dtype)
        res["taps_scale"] = tap_sums64(s["add_abs"], *args, dtype=F64, absolute=True)
    return res


# ---------------------------------------------------------------------------
# the tolerance rule
# ---------------------------------------------------------------------------
class Report:
    """Collects (name, worst |kernel - fp64| / tolerance) and says at the end whether every quantity met the rule."""

    def __init__(self):
        self.rows = {}

    def check(self, name, got, ref64, ref32, scale):
        """scale: a number or a tensor of ref64's shape (per-output scales of a reduction)."""
        ref64 = ref64.detach().to(F64)
        err = (got.detach().cpu().to(F64).reshape(ref64.shape) - ref64).abs()
        ref_err = float((ref32.detach().to(F64).reshape(ref64.shape) - ref64).abs().max()) if ref64.numel() else 0.0
        scale = torch.as_tensor(scale, dtype=F64)
        tol = FACTOR * ref_err + 8 * ULP * scale.expand_as(err) if scale.dim() else torch.full_like(err, FACTOR * ref_err + 8 * ULP * float(scale))
        ratio = torch.where(err <= tol, err / tol.clamp_min(1e-300), torch.full_like(err, float("inf")))
        ratio = torch.where(err == 0, torch.zeros_like(err), ratio)
        worst = float(ratio.max()) if err.numel() else 0.0
        if worst == float("inf"):                      # report by how much the rule was missed
            bad = err > tol
            worst = float((err[bad] / tol[bad].clamp_min(1e-300)).max())
        old = self.rows.get(name, (0.0, 0.0, 0.0))
        self.rows[name] = (max(old[0], worst), max(old[1], float(err.max()) if err.numel() else 0.0), max(old[2], ref_err))
        return worst <= 1.0

    def failed(self):
        return {k: v for k, v in self.rows.items() if not v[0] <= 1.0}

    def table(self, title):
        lines = [f"\n  {title}: |kernel - fp64| / (FACTOR {FACTOR:g} x max|ref32 - fp64| + 8 ulp x scale), worst per quantity"]
        for k, (ratio, err, ref_err) in self.rows.items():
            lines.append(f"    {k:28s} ratio {ratio:9.3e}   max|kernel-fp64| {err:.3e}   max|ref32-fp64| {ref_err:.3e}")
        return "\n".join(lines)


# ---------------------------------------------------------------------------
# the general case of the landmark update: trained-like weights, inputs chosen so that no decision sits within rounding of its kink
# ---------------------------------------------------------------------------
SEED1, SEED2 = 101, 202                     # the dropout seeds of the two hidden layers in every test
# input seed of (B, F, p) where RandomState(11 + B) misses the condition below (found on the CPU, margins as they are)
INPUT_SEED = {(4, 16, 0.0): 100, (4, 16, 0.5): 100}      # (11 + 4 clamps nothing at F = 16)
GENERAL_CASES = [(B, F, p) for B in (1, 4, 16, 17) for F in (5, 16) for p in (0.0, 0.5)]
MARGIN = 1e-5


def oracle_mlp(weight_seed: int):
    """node_coordinate_mlp[0] of the oracle model gpu_util.model_pair(16, 3, 1, coord=True, seed=weight_seed) builds (the same
    constructor arguments, the same fill), without the HIP model next to it."""
    from fixtures_util import fill_state_dict
    ref = O.OracleHierarchicalPatchModel(frame_size=16, gnn_dropout_p=0.5, classifier_dropout_p=0.5, node_embedding_dim=128,
                                         node_hidden_dim=128, num_output_channels=4, num_gnn_layers=1, num_aux_graphs=3,
                                         classifier_hidden_dim=32, use_coordinate_graph=True, output_activation="logit",
                                         use_main_graph_only=False)
    fill_state_dict(ref, weight_seed)
    return ref.node_coordinate_mlp[0]


def general_inputs(B: int, F: int, p: float):
    """(lm [4B,128], coords [4B,2]) float32: standard normal rows, coordinates uniform on (-0.5, F - 0.5) -- some get clamped."""
    rs = np.random.RandomState(INPUT_SEED.get((B, F, p), 11 + B))
    lm = torch.from_numpy(rs.standard_normal((4 * B, C)).astype(np.float32))
    c = torch.from_numpy(rs.uniform(-0.5, F - 0.5, (B, 4, 2)).astype(np.float32)).reshape(4 * B, 2)
    return lm, c


def assert_input_condition(fw):
    """On the fp64 reference alone: every BatchNorm output of both hidden layers at least MARGIN in magnitude, every pre-clamp value
    at least MARGIN away from both bounds, some coordinates clamped and some not.  Then two fp32 evaluations take every decision alike."""
    bn, clamp, share = input_condition(fw)
    assert bn >= MARGIN and clamp >= MARGIN and 0.0 < share < 1.0, (bn, clamp, share)
    return bn, clamp, share
