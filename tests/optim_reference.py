"""TEST INFRASTRUCTURE ONLY -- SGD and RMSprop in plain numpy, one function per step, written from the formulas of torch.optim.SGD's
and torch.optim.RMSprop's documentation, with a step count per tensor.  Nothing under echoglad_amd/ may import this file.

    SGD      g = -grad if maximize else grad;   g = g + weight_decay * p
             momentum != 0:  buf = g (the tensor's first update: a copy, no dampening)  else  momentum * buf + (1 - dampening) * g
                             g = g + momentum * buf (nesterov)  else  buf
             p = p - lr * g
    RMSprop  g as above;   sq = alpha * sq + (1 - alpha) * g * g
             centered:  ga = ga + (1 - alpha) * (g - ga);  avg = sqrt(sq - ga * ga) + eps     else  avg = sqrt(sq) + eps
             momentum > 0:  buf = momentum * buf + g / avg;  p = p - lr * buf                  else  p = p - lr * g / avg

``dtype=np.float64`` is the reference (tests/test_optim_reference.py holds it against torch's own classes in double).
``dtype=np.float32`` is the yardstick of what single precision costs, as in oracle/adam_oracle.py: the same formulas with the
hyper-parameters and every elementwise operation rounded to fp32.  ``unit`` / ``ulp32`` / ``as_float32`` are that file's.

The inputs of the GPU comparisons (tests/test_gpu_sgd_rmsprop.py) live here too -- ``SHAPES``, ``SCALES``, ``Inputs``, ``SGD_CASES``,
``RMSPROP_CASES`` -- so that the CPU suite can show on the very same numbers that the GPU tests' bound separates a right kernel from
one with a seeded mistake."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from oracle.adam_oracle import as_float32, ulp32, unit  # noqa: F401  (re-exported)

SCALES = (1.0, 0.3, 2.0, 0.7, 3.0, 1.5)                  # gradients scaled differently per step (tests/test_gpu_adam.py's)
SHAPES = [(1500,), (33, 7), (300,)]                      # two workgroups, two partly filled workgroups; >= 231 elements each
K_BOUND = 4.0                                            # max|device - oracle64| <= K_BOUND * unit(oracle32, oracle64)

SGD_DEFAULTS = dict(lr=1e-2, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False)
RMSPROP_DEFAULTS = dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False, maximize=False)

# name -> what differs from the defaults (the arithmetic cases of the GPU tests; "lr=0" and "eps=0" have a test of their own there)
SGD_CASES = {
    "plain": dict(),
    "weight_decay": dict(weight_decay=0.01),
    "maximize": dict(maximize=True),
    "momentum": dict(momentum=0.9),
    "momentum+dampening": dict(momentum=0.9, dampening=0.1),
    "nesterov": dict(momentum=0.9, nesterov=True),
    "momentum+weight_decay+maximize": dict(momentum=0.9, weight_decay=0.01, maximize=True),
    "lr=0": dict(lr=0.0, momentum=0.9),
}
RMSPROP_CASES = {
    "default": dict(),
    "centered": dict(centered=True),
    "momentum": dict(momentum=0.9),
    "centered+momentum+weight_decay": dict(centered=True, momentum=0.9, weight_decay=0.01),
    "maximize": dict(maximize=True),
    "alpha=0": dict(alpha=0.0),
    "eps=1e-3": dict(eps=1e-3),
    "eps=0": dict(eps=0.0),                              # gradients kept away from zero (Inputs.random_grads(away_from_zero=True))
}


def sgd_hyper(case: str) -> dict:
    return dict(SGD_DEFAULTS, **SGD_CASES[case])


def rmsprop_hyper(case: str) -> dict:
    return dict(RMSPROP_DEFAULTS, **RMSPROP_CASES[case])


def c_floats(hyper: dict) -> dict:
    """The hyper-parameters as the entry points receive them (C floats), for the oracles."""
    out = dict(hyper)
    for k in ("lr", "momentum", "dampening", "weight_decay", "alpha", "eps"):
        if k in out:
            out[k] = as_float32(float(out[k]))
    return out


class Inputs:
    """Seeded initial values and per-step gradients: the draws of tests/test_gpu_adam.py's ``Run``, without a device."""

    def __init__(self, shapes, seed=0, init=None):
        self.rs = np.random.RandomState(seed)
        self.init = [self.rs.standard_normal(s).astype(np.float32) for s in shapes] if init is None else init
        self.shapes = [a.shape for a in self.init]

    def more(self, shapes):
        new = [self.rs.standard_normal(s).astype(np.float32) for s in shapes]
        self.init += new
        self.shapes += [a.shape for a in new]
        return new

    def random_grads(self, scale=1.0, away_from_zero=False):
        gs = [self.rs.standard_normal(s) * scale for s in self.shapes]
        if away_from_zero:
            gs = [np.sign(g) * (0.5 + np.abs(g)) for g in gs]
        return [g.astype(np.float32) for g in gs]


def arithmetic_grads(case: str, seed: int = 1, steps: int = 6):
    """(initial values, [gradients of step 1, ...]) of the GPU tests' arithmetic comparison of ``case``."""
    inp = Inputs(SHAPES, seed=seed)
    return inp.init, [inp.random_grads(SCALES[it], away_from_zero=case == "eps=0") for it in range(steps)]


def sgd_step(p, g, buf, t, *, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False, dtype=np.float64):
    """One update of one tensor that has had ``t`` updates so far: (p, buf) after it; ``buf`` is None without a momentum.  Inputs are
    left unchanged."""
    f = np.dtype(dtype).type
    p, g = np.asarray(p).astype(dtype), np.asarray(g).astype(dtype)
    lr, mom, damp, wd = f(lr), f(momentum), f(dampening), f(weight_decay)
    with np.errstate(all="ignore"):
        if maximize:
            g = -g
        if wd != 0:
            g = g + wd * p
        if mom != 0:
            buf = g.copy() if t == 0 or buf is None else mom * np.asarray(buf).astype(dtype) + (f(1) - damp) * g
            g = g + mom * buf if nesterov else buf
        else:
            buf = None
        p = p - lr * g
    assert p.dtype == np.dtype(dtype) and (buf is None or buf.dtype == np.dtype(dtype))
    return p, buf


def rmsprop_step(p, g, sq, ga, buf, *, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False, maximize=False,
                 dtype=np.float64):
    """One update of one tensor: (p, sq, ga, buf) after it; ``ga`` / ``buf`` stay None unless centered / momentum > 0 (zeros when they
    are needed and not there yet)."""
    f = np.dtype(dtype).type
    p, g, sq = (np.asarray(a).astype(dtype) for a in (p, g, sq))
    lr, alpha, eps, wd, mom = f(lr), f(alpha), f(eps), f(weight_decay), f(momentum)
    with np.errstate(all="ignore"):
        if maximize:
            g = -g
        if wd != 0:
            g = g + wd * p
        sq = alpha * sq + (f(1) - alpha) * g * g
        if centered:
            ga = np.zeros_like(p) if ga is None else np.asarray(ga).astype(dtype)
            ga = ga + (f(1) - alpha) * (g - ga)
            avg = np.sqrt(sq - ga * ga) + eps
        else:
            avg = np.sqrt(sq) + eps
        if mom > 0:
            buf = np.zeros_like(p) if buf is None else np.asarray(buf).astype(dtype)
            buf = mom * buf + g / avg
            p = p - lr * buf
        else:
            p = p - lr * g / avg
    assert p.dtype == sq.dtype == np.dtype(dtype)
    return p, sq, ga, buf


class _Oracle:
    """A list of tensors with a per-tensor state (``t[k]`` updates so far); ``step(grads, **hyper)`` updates every tensor whose
    gradient is not None and leaves the others, their count included, alone.  ``s[name][k]``: state array ``name`` of tensor k, None
    while it does not exist."""
    NAMES: Sequence[str] = ()

    def __init__(self, params: Sequence[np.ndarray], dtype=np.float64):
        self.dtype = dtype
        self.p: List[np.ndarray] = []
        self.t: List[int] = []
        self.s: Dict[str, List[Optional[np.ndarray]]] = {n: [] for n in self.NAMES}
        self.add(params)

    def add(self, params: Sequence[np.ndarray]) -> None:
        new = [np.asarray(a).astype(self.dtype) for a in params]
        self.p += new
        self.t += [0] * len(new)
        for n in self.NAMES:
            self.s[n] += [None] * len(new)

    def set(self, name: str, k: int, value) -> None:
        self.s[name][k] = None if value is None else np.asarray(value).astype(self.dtype)

    def clear(self, k: int) -> None:
        self.t[k] = 0
        for n in self.NAMES:
            self.s[n][k] = None

    def step(self, grads, only=None, step_fn=None, **hyper) -> None:
        for k in (range(len(self.p)) if only is None else only):
            if grads[k] is None:
                continue
            self._update(k, grads[k], step_fn, hyper)
            self.t[k] += 1


class SGDOracle(_Oracle):
    NAMES = ("momentum_buffer",)

    def _update(self, k, g, step_fn, hyper):
        b = self.s["momentum_buffer"]
        self.p[k], b[k] = (step_fn or sgd_step)(self.p[k], g, b[k], self.t[k], dtype=self.dtype, **hyper)


class RMSpropOracle(_Oracle):
    NAMES = ("square_avg", "grad_avg", "momentum_buffer")

    def _update(self, k, g, step_fn, hyper):
        s = self.s
        sq = np.zeros_like(self.p[k]) if s["square_avg"][k] is None else s["square_avg"][k]
        self.p[k], s["square_avg"][k], s["grad_avg"][k], s["momentum_buffer"][k] = (step_fn or rmsprop_step)(
            self.p[k], g, sq, s["grad_avg"][k], s["momentum_buffer"][k], dtype=self.dtype, **hyper)
