"""The CNN-pyramid block in training mode on the CPU in any dtype, from F.conv2d and F.batch_norm(training=True) -- the reference of
tests/test_pyramid_train_host.py and tests/test_gpu_pyramid_train.py (a helper, not a test file):

    z = b3 + conv3x3(x, w3);  y = BatchNorm_train(z);  v = y + x;  m, idx = AdaptiveMaxPool2d(side_out)(v);  out = relu(m) * keep

The pool's argmax and the ReLU's gate are discontinuous, so they can be INJECTED: with `idx` the pool is a gather at idx, with `gate`
(0 / 1, pooled size) the ReLU is a multiplication by that constant, with `keep` [B * 128] the plane mask is applied.  Without them
the block pools and rectifies by itself."""
from __future__ import annotations

import torch
import torch.nn.functional as F

EPS, MOMENTUM = 1e-5, 0.1


def pooled_dout(fx, side_out):
    """The fixture's dout is full size: the pooled block takes its top-left corner."""
    return fx["dout"][:, :, :side_out, :side_out].contiguous()


def pyramid_block_reference(fx, dtype, side_out, idx=None, gate=None, keep=None):
    """-> dict: v (the pre-pool map), m (pooled v), idx (int64, offsets inside a plane), out, rm, rv, dz, and the gradients dx, dw3,
    db3, dgamma, dbeta of sum(out * dout)."""
    B, C, side = fx["B"], fx["c_out"], fx["side"]
    leaf = lambda k: fx[k].detach().to(dtype).clone().requires_grad_()
    x, w3, b3, gamma, beta = leaf("x"), leaf("w3"), leaf("b3"), leaf("gamma"), leaf("beta")
    rm, rv = fx["rm"].to(dtype).clone(), fx["rv"].to(dtype).clone()
    z = F.conv2d(x, w3, b3, padding=1)
    z.retain_grad()
    y = F.batch_norm(z, rm, rv, gamma, beta, True, MOMENTUM, EPS)
    v = y + x
    if idx is None:
        m, used = F.adaptive_max_pool2d(v, side_out, return_indices=True)
    else:
        used = idx.to(torch.int64).cpu()
        m = v.flatten(2).gather(2, used.flatten(2)).view(B, C, side_out, side_out)
    out = torch.relu(m) if gate is None else m * gate.to(dtype).cpu()
    if keep is not None:
        out = out * keep.to(dtype).cpu().view(B, C, 1, 1)
    (out * pooled_dout(fx, side_out).to(dtype)).sum().backward()
    return dict(v=v.detach(), m=m.detach(), idx=used, out=out.detach(), rm=rm, rv=rv, dz=z.grad, dx=x.grad, dw3=w3.grad, db3=b3.grad,
                dgamma=gamma.grad, dbeta=beta.grad)


def window_max(v, side_out):
    """The largest value of every window of v."""
    return F.adaptive_max_pool2d(v, side_out)


def window_gap(v, side_out):
    """Per window: the largest value minus the second largest (inf for a window of one pixel)."""
    B, C, side, _ = v.shape
    gaps = torch.full((B, C, side_out, side_out), float("inf"), dtype=v.dtype)
    for i in range(side_out):
        y0, y1 = (i * side) // side_out, -((-(i + 1) * side) // side_out)
        for j in range(side_out):
            x0, x1 = (j * side) // side_out, -((-(j + 1) * side) // side_out)
            w = v[:, :, y0:y1, x0:x1].flatten(2)
            if w.shape[2] > 1:
                top = w.topk(2, dim=2).values
                gaps[:, :, i, j] = top[:, :, 0] - top[:, :, 1]
    return gaps
