"""CPU: tests/optim_reference.py -- the fp64 SGD / RMSprop oracles against torch's own classes in double, and how hard the bound of the
GPU comparisons (tests/test_gpu_sgd_rmsprop.py) bites on those tests' very inputs: every seeded mistake a kernel could plausibly
carry lands at least 100 bounds away from the fp64 oracle, the fp32 oracle itself a quarter of a bound."""
import numpy as np
import pytest
import torch

import optim_reference as R

# the flag combinations of the captured-step tests, beside the arithmetic cases
EXTRA_SGD = {"captured: momentum+dampening": dict(momentum=0.9, dampening=0.1), "captured: nesterov": dict(momentum=0.9, nesterov=True)}
EXTRA_RMSPROP = {"captured: centered+momentum": dict(centered=True, momentum=0.9)}


def _against_torch(torch_cls, oracle_cls, hyper, case):
    """6 steps on the GPU tests' inputs plus a short tensor that sits out step 3 and one that gets its first gradient in step 3 (its
    first update -- SGD's buffer copy -- comes when its neighbours' buffers are two steps old)."""
    init, steps = R.arithmetic_grads(case if case in ("eps=0",) else "")
    init = init + [init[0][:40] * 2, init[0][40:90] * 0.5]
    tp = [torch.nn.Parameter(torch.from_numpy(a.astype(np.float64))) for a in init]
    opt = torch_cls(tp, foreach=False, **hyper)
    o = oracle_cls(init)
    for k, gs in enumerate(steps):
        gs = gs + [None if k == 2 else gs[0][:40] * 0.5, None if k < 2 else gs[0][40:90] * 2]
        for t, g in zip(tp, gs):
            t.grad = None if g is None else torch.from_numpy(g.astype(np.float64))
        opt.step()
        o.step(gs, **hyper)
    assert o.t == [6, 6, 6, 5, 4]
    worst = 0.0
    for k, t in enumerate(tp):
        pairs = [(o.p[k], t.detach())]
        for name in o.NAMES:
            want = opt.state[t].get(name)
            if torch.is_tensor(want) and (name != "grad_avg" or hyper.get("centered")) and (name != "momentum_buffer" or hyper.get("momentum", 0) > 0):
                assert o.s[name][k] is not None, (name, k)
                pairs.append((o.s[name][k], want))
            else:
                assert o.s[name][k] is None, (name, k)
        if "step" in opt.state[t]:
            assert int(opt.state[t]["step"]) == o.t[k]
        for got, want in pairs:
            want = want.numpy()
            err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
            worst = max(worst, err)
            assert err <= 1e-13, (k, err)
    return worst


@pytest.mark.parametrize("case", list(R.SGD_CASES) + list(EXTRA_SGD))
def test_sgd_oracle_fp64_is_torch_sgd_in_double(case):
    hyper = dict(R.SGD_DEFAULTS, **(R.SGD_CASES[case] if case in R.SGD_CASES else EXTRA_SGD[case]))
    _against_torch(torch.optim.SGD, R.SGDOracle, hyper, case)


@pytest.mark.parametrize("case", list(R.RMSPROP_CASES) + list(EXTRA_RMSPROP))
def test_rmsprop_oracle_fp64_is_torch_rmsprop_in_double(case):
    hyper = dict(R.RMSPROP_DEFAULTS, **(R.RMSPROP_CASES[case] if case in R.RMSPROP_CASES else EXTRA_RMSPROP[case]))
    _against_torch(torch.optim.RMSprop, R.RMSpropOracle, hyper, case)


# ---- the centered inputs stay away from the cancellation ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c, h in R.RMSPROP_CASES.items() if h.get("centered")])
def test_centered_inputs_keep_the_square_root_away_from_cancellation(case):
    """sqrt(sq - ga^2): with gradients of one value sq -> ga^2 and the difference is rounding noise no fp32 kernel can be held to.
    Random gradients of changing scale keep sq - ga^2 >= 1e-3 sq for every element at every step."""
    hyper = R.c_floats(R.rmsprop_hyper(case))
    init, steps = R.arithmetic_grads(case)
    o = R.RMSpropOracle(init)
    low = np.inf
    for gs in steps:
        o.step(gs, **hyper)
        for sq, ga in zip(o.s["square_avg"], o.s["grad_avg"]):
            low = min(low, float(((sq - ga * ga) / sq).min()))
    print(f"{case}: min (sq - ga^2) / sq = {low:.4f}")
    assert low >= 1e-3


# ---- seeded mistakes ----------------------------------------------------------------------------------------------------------------
def _wrong_sgd(mistake):
    def step(p, g, buf, t, *, lr, momentum, dampening, weight_decay, nesterov, maximize, dtype):
        f = np.dtype(dtype).type
        p, g = np.asarray(p).astype(dtype), np.asarray(g).astype(dtype)
        lr, mom, damp, wd = f(lr), f(momentum), f(dampening), f(weight_decay)
        if maximize and mistake != "maximize sign lost":
            g = -g
        if wd != 0 and mistake != "weight decay dropped":
            g = g + wd * p
        if mom != 0:
            first = t == 0
            if mistake == "count behind by one on the first step":
                first = t - 1 == 0
            if mistake == "first buffer taken as zeros with dampening applied":
                first = False
            old = np.zeros_like(p) if buf is None else np.asarray(buf).astype(dtype)
            w = f(1) if mistake == "dampening ignored" else f(1) - damp
            buf = g.copy() if first else mom * old + w * g
            g = buf if (not nesterov or mistake == "nesterov term dropped") else g + mom * buf
        return p - lr * g, buf
    return step


def _wrong_rmsprop(mistake):
    def step(p, g, sq, ga, buf, *, lr, alpha, eps, weight_decay, momentum, centered, maximize, dtype):
        f = np.dtype(dtype).type
        p, g, sq = (np.asarray(a).astype(dtype) for a in (p, g, sq))
        lr, alpha, eps, wd, mom = f(lr), f(alpha), f(eps), f(weight_decay), f(momentum)
        if maximize and mistake != "maximize sign lost":
            g = -g
        if wd != 0 and mistake != "weight decay dropped":
            g = g + wd * p
        sq = alpha * sq + (f(1) - alpha) * g * g
        inner = sq
        if centered:
            ga = np.zeros_like(p) if ga is None else np.asarray(ga).astype(dtype)
            ga = ga + (f(1) - alpha) * (g - ga)
            if mistake != "the centered term dropped":
                inner = sq - ga * ga
        avg = np.sqrt(inner + eps) if mistake == "eps added inside the square root" else np.sqrt(inner) + eps
        if mom > 0:
            buf = np.zeros_like(p) if buf is None else np.asarray(buf).astype(dtype)
            buf = mom * buf + (lr * g / avg if mistake == "RMSprop buffer scaled by lr twice" else g / avg)
            return p - lr * buf, sq, ga, buf
        return p - lr * g / avg, sq, ga, buf
    return step


# (mistake, algorithm, the GPU case whose inputs and hyper-parameters show it)
MISTAKES = [
    ("first buffer taken as zeros with dampening applied", "sgd", "momentum+dampening"),
    ("nesterov term dropped", "sgd", "nesterov"),
    ("dampening ignored", "sgd", "momentum+dampening"),
    ("eps added inside the square root", "rmsprop", "eps=1e-3"),
    ("the centered term dropped", "rmsprop", "centered"),
    ("the centered term dropped", "rmsprop", "centered+momentum+weight_decay"),
    ("RMSprop buffer scaled by lr twice", "rmsprop", "momentum"),
    ("weight decay dropped", "sgd", "weight_decay"),
    ("weight decay dropped", "rmsprop", "centered+momentum+weight_decay"),
    ("maximize sign lost", "sgd", "maximize"),
    ("maximize sign lost", "rmsprop", "maximize"),
    ("count behind by one on the first step", "sgd", "momentum"),
    ("count behind by one on the first step", "sgd", "momentum+dampening"),
]


def _arrays(o):
    return [("p", o.p)] + [(n, o.s[n]) for n in o.NAMES if o.s[n][0] is not None]


@pytest.mark.parametrize("mistake,algo,case", MISTAKES, ids=[f"{m} [{a}: {c}]" for m, a, c in MISTAKES])
def test_gpu_bound_separates_seeded_mistakes(mistake, algo, case):
    """The mistake, evaluated in fp32 on the inputs of the GPU test's ``case``, against that test's bound K * max(e32, ulp32): at
    least 100 bounds away in the parameters of some tensor; the fp32 oracle itself is 1 / K of a bound away by construction."""
    cls, hyper, wrong = ((R.SGDOracle, R.sgd_hyper(case), _wrong_sgd(mistake)) if algo == "sgd" else
                         (R.RMSpropOracle, R.rmsprop_hyper(case), _wrong_rmsprop(mistake)))
    hyper = R.c_floats(hyper)
    init, steps = R.arithmetic_grads(case)
    o64, o32, bad = cls(init, np.float64), cls(init, np.float32), cls(init, np.float32)
    for gs in steps:
        o64.step(gs, **hyper)
        o32.step(gs, **hyper)
        bad.step(gs, step_fn=wrong, **hyper)
    ratios = {}
    for (name, w64), (_, w32), (_, got) in zip(_arrays(o64), _arrays(o32), _arrays(bad)):
        per_tensor = []
        for a64, a32, g in zip(w64, w32, got):
            bound = 8.0 * R.unit(a32, a64)                                       # (K may rise to 8 at the most: held even there)
            per_tensor.append(float(np.abs(g.astype(np.float64) - a64).max()) / bound)
            assert float(np.abs(a32.astype(np.float64) - a64).max()) <= bound / 8.0 + 1e-300
        ratios[name] = min(per_tensor)                                           # every tensor shows it
    print(f"{mistake} [{algo}: {case}]: bounds away (K = 8), worst tensor: " + ", ".join(f"{n} {r:.0f}" for n, r in ratios.items()))
    assert ratios["p"] >= 100.0, ratios
