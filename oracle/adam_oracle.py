"""TEST INFRASTRUCTURE ONLY -- Adam (amsgrad off) in plain numpy, one function per step, written from the formulas of
torch.optim.Adam's documentation.  Nothing under echoglad_amd/ may import this file.

    g = -grad if maximize else grad
    g = g + weight_decay * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)            t = number of updates of THIS tensor, this one included

``dtype=np.float64`` is the reference.  ``dtype=np.float32`` is the yardstick of what single precision costs: the same formulas, the
hyper-parameters and every elementwise operation rounded to fp32, the two bias corrections (``lr / (1 - b1^t)`` and
``sqrt(1 - b2^t)``) evaluated in fp64 and rounded once, as the header of csrc/adam.hip describes its arithmetic.  It is not a second
reference: ``bound`` turns its distance from the fp64 form into the tolerance of a comparison.

The hyper-parameters reach ``eg_adam_step`` as C floats.  ``as_float32`` gives the value the kernel receives; the GPU tests hand that
value to the fp64 form as well, so that the comparison measures the arithmetic and not the rounding of 0.999 (``1 - float32(0.999)``
is 1.3e-5 off ``1 - 0.999`` in relative terms, and exp_avg_sq with it: tests/test_oracle.py pins that figure)."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np


def as_float32(x: float) -> float:
    """x as a C float holds it, as a Python float."""
    return float(np.float32(x))


def adam_step(p, g, m, v, t, *, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False, dtype=np.float64):
    """One update of one tensor: (p, m, v) after update number ``t`` (1 for the first).  Inputs are left unchanged."""
    f = np.dtype(dtype).type
    p, g, m, v = (np.asarray(a).astype(dtype) for a in (p, g, m, v))
    b1, b2 = f(betas[0]), f(betas[1])
    lr, eps, wd = f(lr), f(eps), f(weight_decay)
    with np.errstate(all="ignore"):                                     # (non-finite gradients, eps = 0 on v = 0: IEEE results are wanted)
        if maximize:
            g = -g
        if wd != 0:
            g = g + wd * p
        m = b1 * m + (f(1) - b1) * g
        v = b2 * v + (f(1) - b2) * g * g
        step_size = f(np.float64(lr) / (1.0 - np.float64(b1) ** np.float64(t)))
        bc2_sqrt = f(np.sqrt(1.0 - np.float64(b2) ** np.float64(t)))
        p = p - step_size * m / (np.sqrt(v) / bc2_sqrt + eps)
    assert p.dtype == m.dtype == v.dtype == np.dtype(dtype)
    return p, m, v


class AdamOracle:
    """A list of tensors with torch's per-tensor state (``t[k]`` updates so far); ``step(grads, **hyper)`` updates every tensor whose
    gradient is not None and leaves the others, their count included, alone."""

    def __init__(self, params: Sequence[np.ndarray], dtype=np.float64):
        self.dtype = dtype
        self.p: List[np.ndarray] = [np.asarray(a).astype(dtype) for a in params]
        self.m: List[np.ndarray] = [np.zeros_like(a) for a in self.p]
        self.v: List[np.ndarray] = [np.zeros_like(a) for a in self.p]
        self.t: List[int] = [0] * len(self.p)

    def add(self, params: Sequence[np.ndarray]) -> None:
        """More tensors (a parameter group added later): zero moments, no update so far."""
        new = [np.asarray(a).astype(self.dtype) for a in params]
        self.p += new
        self.m += [np.zeros_like(a) for a in new]
        self.v += [np.zeros_like(a) for a in new]
        self.t += [0] * len(new)

    def step(self, grads: Sequence[Optional[np.ndarray]], only: Optional[Sequence[int]] = None, **hyper) -> None:
        for k in (range(len(self.p)) if only is None else only):
            if grads[k] is None:
                continue
            self.t[k] += 1
            self.p[k], self.m[k], self.v[k] = adam_step(self.p[k], grads[k], self.m[k], self.v[k], self.t[k], dtype=self.dtype, **hyper)


def ulp32(x: float) -> float:
    """The spacing of fp32 at |x|."""
    return float(np.spacing(np.float32(abs(x))))


def bound(o32: np.ndarray, o64: np.ndarray, factor: float = 4.0) -> float:
    """The tolerance of ``max|device - o64|`` for one tensor: ``factor`` times what the fp32 form of the oracle is away from the fp64
    form, and at least ``factor`` ulps of the largest value.  Non-finite elements are compared separately and left out here."""
    return factor * unit(o32, o64)


def unit(o32: np.ndarray, o64: np.ndarray) -> float:
    """max(e32, ulp32(max|o64|)) over the finite elements: the unit error ratios are reported in."""
    ok = np.isfinite(o64)
    if not ok.any():
        return 0.0
    e32 = float(np.abs(o32.astype(np.float64)[ok] - o64[ok]).max())
    return max(e32, ulp32(float(np.abs(o64[ok]).max())))
