"""-m gpu: echoglad_amd.optim.SGD / RMSprop (eg_sgd_step / eg_rmsprop_step, csrc/optim.hip: one launch per 120 / 84 tensors, step
counts on the device) against tests/optim_reference.py, plain fp64 SGD and RMSprop in numpy with a step count per tensor.

Built like tests/test_gpu_adam.py.  Inputs are fp32 values, the oracle gets the same values cast up; the hyper-parameters are handed
to the oracle as the C floats the entry points receive.  Tolerance of every oracle comparison, per tensor and per array (p and every
state array):

    max|device - oracle64|  <=  4 * max(e32, ulp32(max|oracle64|)),        e32 = max|oracle32 - oracle64|

oracle32 being the same formulas with every operation rounded to fp32.  4 is the project's figure for Adam: FMA contraction and
another order of the operations in the device code against numpy, over about as many rounded operations per element and step.
tests/test_optim_reference.py shows on these tests' inputs that a first buffer taken as zeros, a dropped nesterov or centered term,
an ignored dampening, eps inside the square root, a buffer scaled by lr twice, a dropped weight decay, a lost maximize sign and a
count behind by one are each more than 100 of these bounds away (even with 8 in place of 4).

Every check prints its figures before it asserts (``pytest tests/test_gpu_sgd_rmsprop.py -s``: one ``OPTIM_RATIO <class> <case>: p,
<state arrays>`` line per check).  Largest measured err / max(e32, ulp) on an MI355X, worst over the 6 steps and 3 tensors of each
arithmetic case (the bound is 4):

    SGD      case                              p     momentum_buffer
             plain                             1.00
             weight_decay                      1.00
             maximize                          1.00
             momentum                          1.00  1.00
             momentum+dampening                1.00  1.00
             nesterov                          1.00  1.00
             momentum+weight_decay+maximize    1.00  1.00
             lr=0                              0.00  0.98
    RMSprop  case                              p     square_avg  grad_avg  momentum_buffer
             default                           1.00  1.00
             centered                          1.00  1.00        1.01
             momentum                          1.00  1.00                  1.00
             centered+momentum+weight_decay    1.00  1.00        1.00      1.16
             maximize                          1.00  1.00
             alpha=0                           0.58  0.50
             eps=1e-3                          1.00  1.00
             eps=0                             1.00  1.00

(1.00: the device's error is the fp32 oracle's own, or an ulp of the largest value.)  Over the other tests of this file the largest
ratios are 1.32 (SGD: p, stale cache with 130 tensors) and 1.81 (RMSprop: p, same test; grad_avg 1.46 after a replaced step count,
momentum_buffer 1.35); the chunk-edge test stays at 1.03.  K stays 4."""
import numpy as np
import pytest
import torch

import optim_reference as R
from gpu_util import DEV
from echoglad_amd import engine, ops, optim
from echoglad_amd.optim import SGD, RMSprop

pytestmark = pytest.mark.gpu

SCALES, SHAPES = R.SCALES, R.SHAPES
CHUNK = 1024                                             # elements per workgroup: 256 threads x 4
KINDS = {"sgd": (SGD, R.SGDOracle, R.SGD_DEFAULTS), "rmsprop": (RMSprop, R.RMSpropOracle, R.RMSPROP_DEFAULTS)}
# the configuration that uses every state array of a class (cache, state, gradient-form and edge tests)
FULL = {"sgd": dict(momentum=0.9, dampening=0.1), "rmsprop": dict(centered=True, momentum=0.9)}


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _hyper(kind, **changes):
    return dict(KINDS[kind][2], **changes)


def _used(hyper):
    """The state arrays an update with ``hyper`` reads and writes."""
    if "alpha" in hyper:
        return ("square_avg",) + (("grad_avg",) if hyper["centered"] else ()) + (("momentum_buffer",) if hyper["momentum"] > 0 else ())
    return ("momentum_buffer",) if hyper["momentum"] != 0 else ()


class Run(R.Inputs):
    """Device parameters (gradients allocated once and written in place, so their addresses never change) and the two oracles on the
    same values.  ``groups``: [(indices, hyper-parameters)] -- what the oracle applies to which tensors."""

    def __init__(self, kind, shapes, seed=0, init=None):
        super().__init__(shapes, seed, init)
        self.kind = kind
        self.params = [torch.nn.Parameter(_dev(a)) for a in self.init]
        for p in self.params:
            p.grad = torch.zeros_like(p)
        self.parked = {}
        oracle = KINDS[kind][1]
        self.o64, self.o32 = oracle(self.init, np.float64), oracle(self.init, np.float32)
        self.worst = {}

    def add(self, shapes):
        init = self.more(shapes)
        new = [torch.nn.Parameter(_dev(a)) for a in init]
        for p in new:
            p.grad = torch.zeros_like(p)
        self.params += new
        for o in (self.o64, self.o32):
            o.add(init)
        return new

    def oracle_step(self, grads, groups):
        for idx, hyper in groups:
            for o in (self.o64, self.o32):
                o.step(grads, only=idx, **R.c_floats(hyper))

    def step(self, opt, grads, groups):
        """One step of the optimizer and of both oracles with ``grads`` (None: this parameter has no gradient in this step)."""
        for k, (p, g) in enumerate(zip(self.params, grads)):
            if g is None:
                if p.grad is not None:
                    self.parked[k], p.grad = p.grad, None
            else:
                if p.grad is None:
                    p.grad = self.parked.pop(k)
                p.grad.copy_(_dev(g))
        opt.step()
        self.oracle_step(grads, groups)

    def check(self, opt, case):
        """Counts exact; p and every state array of every tensor within the bound of the fp64 oracle (non-finite elements: in the same
        places).  Prints the figures before it asserts."""
        torch.cuda.synchronize()
        fails = []
        for k, p in enumerate(self.params):
            st = opt.state.get(p, {})
            t = float(st["step"]) if "step" in st else 0.0
            if t != float(self.o64.t[k]):
                fails.append(f"tensor {k}: step count {t}, oracle {self.o64.t[k]}")
            arrays = [("p", _np(p), self.o32.p[k], self.o64.p[k])]
            for name in self.o64.NAMES:
                if self.o64.s[name][k] is None:
                    continue
                if not torch.is_tensor(st.get(name)):
                    fails.append(f"tensor {k}: no {name} in the state after {self.o64.t[k]} updates")
                    continue
                arrays.append((name, _np(st[name]), self.o32.s[name][k], self.o64.s[name][k]))
            for name, got, w32, w64 in arrays:
                got, w64 = got.reshape(w64.shape), np.asarray(w64)
                ok = np.isfinite(w64)
                if not np.array_equal(np.isfinite(got), ok):
                    fails.append(f"tensor {k} {name}: non-finite elements at {np.flatnonzero(~np.isfinite(got))[:8]}, oracle at {np.flatnonzero(~ok)[:8]}")
                    continue
                if not ok.any():
                    continue
                err, unit = float(np.abs(got[ok] - w64[ok]).max()), R.unit(w32, w64)
                self.worst[name] = max(self.worst.get(name, 0.0), err / unit)
                if err > R.K_BOUND * unit:
                    fails.append(f"tensor {k} {name}: err {err:.3e} = {err / unit:.2f} x max(e32, ulp) = {unit:.3e}")
        print(f"OPTIM_RATIO {self.kind} {case}: " + "  ".join(f"{n} {r:.2f}" for n, r in self.worst.items()))
        assert not fails, (case, fails[:10], len(fails))


# ---- kernel arithmetic against fp64 ---------------------------------------------------------------------------------------------
ARITHMETIC = [("sgd", c) for c in R.SGD_CASES if c != "lr=0"] + [("rmsprop", c) for c in R.RMSPROP_CASES]


@pytest.mark.parametrize("kind,case", ARITHMETIC, ids=[f"{k}: {c}" for k, c in ARITHMETIC])
def test_arithmetic_against_fp64(kind, case):
    hyper = R.sgd_hyper(case) if kind == "sgd" else R.rmsprop_hyper(case)
    run = Run(kind, SHAPES, seed=1)
    opt = KINDS[kind][0](run.params, **hyper)
    for it in range(6):
        run.step(opt, run.random_grads(SCALES[it], away_from_zero=case == "eps=0"), [(None, hyper)])
        run.check(opt, case)
    for p in run.params:
        assert set(opt.state[p]) == set(_used(hyper)) | {"step"}                 # torch's keys, nothing else


def test_sgd_lr_zero_moves_buffer_and_counts_only():
    hyper = R.sgd_hyper("lr=0")
    run = Run("sgd", SHAPES, seed=1)
    before = [p.detach().clone() for p in run.params]
    opt = SGD(run.params, **hyper)
    for it in range(6):
        run.step(opt, run.random_grads(SCALES[it]), [(None, hyper)])
    run.check(opt, "lr=0")
    for p, q in zip(run.params, before):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))             # bit-unchanged
        assert float(opt.state[p]["step"]) == 6.0 and float(opt.state[p]["momentum_buffer"].abs().max()) > 0


@pytest.mark.parametrize("kind", list(KINDS))
def test_lr_as_a_device_scalar_filled_between_steps(kind):
    lr = torch.tensor(1e-3, device=DEV)
    hyper = _hyper(kind, weight_decay=0.01, **FULL[kind])
    run = Run(kind, SHAPES, seed=4)
    opt = KINDS[kind][0](run.params, **dict(hyper, lr=lr))
    for it, value in enumerate([1e-3, 1e-3, 5e-4, 5e-4, 2e-3, 1e-4]):
        lr.fill_(value)
        run.step(opt, run.random_grads(SCALES[it]), [(None, dict(hyper, lr=value))])
        run.check(opt, "tensor lr")
    assert opt.param_groups[0]["lr"] is lr


@pytest.mark.parametrize("kind", list(KINDS))
def test_two_param_groups_in_one_optimizer(kind):
    run = Run(kind, SHAPES + [(2049,), (257,)], seed=5)
    ha = _hyper(kind, lr=1e-3)                                                   # (no momentum: SGD's launch without buffers)
    hb = _hyper(kind, lr=3e-2, weight_decay=0.1, **FULL[kind])
    opt = KINDS[kind][0]([dict(params=run.params[:3], **ha), dict(params=run.params[3:], **hb)])
    for it in range(6):
        run.step(opt, run.random_grads(SCALES[it]), [([0, 1, 2], ha), ([3, 4], hb)])
        run.check(opt, "two groups")
    assert "momentum_buffer" not in opt.state[run.params[0]] and "momentum_buffer" in opt.state[run.params[3]]


# ---- first-update semantics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_first_update_of_a_late_parameter_and_of_an_added_group(kind):
    """The third parameter has no gradient in steps 1 - 2: its first update (SGD: the buffer becomes a copy of g, no dampening) is step
    3, when its neighbours' buffers are two steps old -- ONE launch holds tensors on both sides of their first update.  Then the same
    with a group added after step 4."""
    hyper = _hyper(kind, weight_decay=0.01, **FULL[kind])
    run = Run(kind, SHAPES, seed=21)
    opt = KINDS[kind][0](run.params, **hyper)
    groups = [([0, 1, 2], hyper)]
    for it in range(4):
        grads = run.random_grads(SCALES[it])
        if it < 2:
            grads[2] = None
        run.step(opt, grads, groups)
        run.check(opt, "late parameter")
        if it == 1:
            assert run.params[2] not in opt.state                                # never had a gradient: no state
    assert [float(opt.state[p]["step"]) for p in run.params] == [4.0, 4.0, 2.0]
    hb = _hyper(kind, lr=3e-2, **FULL[kind])
    opt.add_param_group(dict(params=run.add([(1025,), (260,)]), **hb))
    groups.append(([3, 4], hb))
    for it in range(4, 6):
        run.step(opt, run.random_grads(SCALES[it]), groups)
        run.check(opt, "add_param_group")
    assert [float(opt.state[p]["step"]) for p in run.params] == [6.0, 6.0, 4.0, 2.0, 2.0]


def test_sgd_loaded_buffer_without_a_step_is_used_not_overwritten():
    """A torch.optim.SGD state (momentum_buffer, no step) loaded: the next update continues the buffer."""
    hyper = _hyper("sgd", **FULL["sgd"])
    run = Run("sgd", SHAPES, seed=22)
    opt = SGD(run.params, **hyper)
    sd = opt.state_dict()
    for k, s in enumerate(run.shapes):
        b0 = (run.rs.standard_normal(s) * 0.3).astype(np.float32)
        sd["state"][k] = {"momentum_buffer": torch.from_numpy(b0.copy())}
        for o in (run.o64, run.o32):
            o.set("momentum_buffer", k, b0)
            o.t[k] = 1
    opt.load_state_dict(sd)
    for it in range(3):
        run.step(opt, run.random_grads(SCALES[it]), [(None, hyper)])
        run.check(opt, "loaded buffer")
    assert [float(opt.state[p]["step"]) for p in run.params] == [4.0] * 3


# ---- chunk edges and bounds ---------------------------------------------------------------------------------------------------------
SENTINEL = -7.25e10
EDGE_NUMELS = (1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
ALL_STATE = {"sgd": ("momentum_buffer",), "rmsprop": ("square_avg", "grad_avg", "momentum_buffer")}


def _guarded(n, first, fill):
    """(buffer, the slice [first, first + n) of it): 64 sentinels on both sides, the slice 4-byte but not 16-byte aligned."""
    buf = torch.full((first + n + 64,), SENTINEL, device=DEV)
    assert first >= 64 and buf.data_ptr() % 16 == 0 and first % 4 != 0
    view = buf[first:first + n]
    if fill is not None:
        view.copy_(fill)
    assert view.data_ptr() % 16 != 0 and view.data_ptr() % 4 == 0 and view.is_contiguous()
    return buf, view


@pytest.mark.parametrize("kind,used", [("sgd", True), ("sgd", False), ("rmsprop", True), ("rmsprop", False)],
                         ids=["sgd", "sgd, buffer unused", "rmsprop", "rmsprop, grad_avg and buffer unused"])
def test_chunk_edges_unaligned_slices_and_sentinels(kind, used):
    """Every array a slice of a larger buffer, 4-byte but not 16-byte aligned, sentinels around it.  The sizes go down to one element,
    where e32 is no yardstick (see tests/test_gpu_adam.py), so nothing cancels: the gradients keep their sign per element over the 3
    steps, |g| in scale * [0.5, 1.5], and that sign is the opposite of the parameter's, so buffers and parameters only grow in
    magnitude and every rounding is a fraction of an ulp of the result.  ``used`` False: momentum 0 / not centered, and the slots of
    the unused state arrays sit in the state all the same, sentinels INSIDE as well -- not one word of them may change."""
    hyper = _hyper(kind, lr=1e-3, weight_decay=0.01, **(FULL[kind] if used else {}))
    names = _used(hyper)
    rs = np.random.RandomState(8)
    init = [rs.standard_normal(n).astype(np.float32) for n in EDGE_NUMELS]
    run = Run(kind, None, seed=8, init=init)
    buffers, params = [], []
    for k, n in enumerate(EDGE_NUMELS):
        first = [65 + (k + j) % 3 for j in range(5)]    # 65, 66 or 67 floats into a 16-byte aligned buffer, another one per array
        pb, pv = _guarded(n, first[0], _dev(init[k]))
        gb, gv = _guarded(n, first[1], torch.zeros(n, device=DEV))
        p = torch.nn.Parameter(pv)
        assert p.data_ptr() == pv.data_ptr()
        p.grad = gv
        slots = {}
        for j, name in enumerate(ALL_STATE[kind]):
            sb, sv = _guarded(n, first[2 + j], torch.zeros(n, device=DEV) if name in names else None)
            slots[name] = (sb, sv, first[2 + j])
        buffers.append((n, [("p", pb, first[0]), ("grad", gb, first[1])] + [(nm, sb, lo) for nm, (sb, _, lo) in slots.items()]))
        params.append((p, slots))
    run.params = [p for p, _ in params]
    opt = KINDS[kind][0](run.params, **hyper)
    for p, slots in params:                              # installed before the first step: the slices are what the kernel writes
        for name, (_, sv, _) in slots.items():
            opt.state[p][name] = sv
        opt.state[p]["step"] = torch.zeros((), device=DEV)       # (a buffer without a count would be one update old)
    signs = [-np.sign(a).astype(np.float64) for a in init]
    for it in range(3):
        grads = [(s * (0.5 + rs.random_sample(s.shape)) * SCALES[it]).astype(np.float32) for s in signs]
        run.step(opt, grads, [(None, hyper)])
        for p, slots in params:
            assert all(opt.state[p][name] is sv for name, (_, sv, _) in slots.items()) and p.grad.data_ptr() % 16 != 0
    run.check(opt, "chunk edges" + ("" if used else ", unused slots"))
    assert [float(opt.state[p]["step"]) for p in run.params] == [3.0] * len(EDGE_NUMELS)
    for n, bufs in buffers:
        for name, buf, lo in bufs:
            bits, want = buf.view(torch.int32), torch.full_like(buf, SENTINEL).view(torch.int32)
            assert lo >= 64 and buf.numel() == lo + n + 64
            assert torch.equal(bits[:lo], want[:lo]) and torch.equal(bits[lo + n:], want[lo + n:]), (n, name)
            if name in ALL_STATE[kind] and name not in names:
                assert torch.equal(bits, want), (n, name, "an unused slot was written")
            elif name != "grad":
                assert not torch.equal(bits[lo:lo + n], want[lo:lo + n]), (n, name)


# ---- workgroup -> (tensor, chunk) look-up -------------------------------------------------------------------------------------------
def _lookup_numels(count, where):
    """count tensors with 1, 2 or 5 chunks mixed (some ending on a chunk boundary, some before it) and ONE of 17 chunks."""
    chunks = [(1, 2, 5)[(k * 7 + k // 3) % 3] for k in range(count)]
    chunks[{"first": 0, "middle": count // 2, "last": count - 1}[where]] = 17
    return [c * CHUNK - (0, 1, 5, 1023)[k % 4] for k, c in enumerate(chunks)]


LOOKUPS = [(kind, count, where) for kind, cap in (("sgd", 120), ("rmsprop", 84)) for count in (cap, cap + 1, 2 * cap, 2 * cap + 1)
           for where in ("first", "middle", "last")]


@pytest.mark.parametrize("kind,count,where", LOOKUPS, ids=[f"{k}-{c}-{w}" for k, c, w in LOOKUPS])
def test_workgroup_lookup_one_optimizer_equals_one_optimizer_per_tensor(kind, count, where):
    """Every workgroup must find its own (tensor, chunk): the list under ONE optimizer (launches of the per-launch maximum) is
    bit-equal to every tensor under an optimizer of its own (one tensor per launch: the look-up is trivial)."""
    cls = KINDS[kind][0]
    assert cls._MAX == (120 if kind == "sgd" else 84)
    hyper = _hyper(kind, weight_decay=0.01, **FULL[kind])
    numels = _lookup_numels(count, where)
    assert {-(-n // CHUNK) for n in numels} == {1, 2, 5, 17}
    gen = torch.Generator(device=DEV).manual_seed(9)
    a = [torch.nn.Parameter(torch.randn(n, device=DEV, generator=gen)) for n in numels]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    one, each = cls(a, **hyper), [cls([q], **hyper) for q in b]
    for it in range(3):
        for p, q in zip(a, b):
            p.grad = torch.randn(p.numel(), device=DEV, generator=gen) * SCALES[it]
            q.grad = p.grad.clone()
        one.step()
        for o in each:
            o.step()
    torch.cuda.synchronize()
    for k, (p, q, o) in enumerate(zip(a, b, each)):
        assert torch.equal(p, q), (k, numels[k])
        for name in _used(hyper):
            assert torch.equal(one.state[p][name], o.state[q][name]), (k, numels[k], name)
        assert float(one.state[p]["step"]) == float(o.state[q]["step"]) == 3.0
        assert bool((one.state[p]["momentum_buffer"] != 0).any())


# ---- the stale prepared launch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shapes,skipped", [(SHAPES, 1), ([(1100,)] + [(300,)] * 128 + [(2049,)], 5)], ids=["3 tensors", "130 tensors"])
def test_stale_cache_a_step_without_one_gradient_in_between(kind, shapes, skipped):
    """A: every parameter.  B: one parameter's gradient is None.  C: every parameter again, the gradients where they were in A -- the
    key of A's prepared launches, whose count array stood still during B.  (130 tensors: the skipped one is in the first launch, so
    the split into launches is shifted in B.)"""
    hyper = _hyper(kind, **FULL[kind])
    run = Run(kind, shapes, seed=14)
    opt = KINDS[kind][0](run.params, **hyper)
    addresses = [p.grad.data_ptr() for p in run.params]
    for it, name in enumerate("ABCD"):
        grads = run.random_grads(SCALES[it])
        if name == "B":
            grads[skipped] = None
        run.step(opt, grads, [(None, hyper)])
        if name != "B":
            assert [p.grad.data_ptr() for p in run.params] == addresses
        if name == "C":
            torch.cuda.synchronize()
            counts = [float(opt.state[p]["step"]) for p in run.params]
            assert counts == [2.0 if k == skipped else 3.0 for k in range(len(shapes))]
        if name in "CD":
            run.check(opt, f"stale cache, {len(shapes)} tensors, after {name}")


# ---- state edited between steps -----------------------------------------------------------------------------------------------------
def _replace_buffer(run, opt, k):
    new = (run.rs.standard_normal(run.shapes[k]) * 0.3).astype(np.float32)
    t = _dev(new)
    opt.state[run.params[k]]["momentum_buffer"] = t
    for o in (run.o64, run.o32):
        o.set("momentum_buffer", k, new)
    return lambda: opt.state[run.params[k]]["momentum_buffer"] is t


def _replace_step(run, opt, k):
    opt.state[run.params[k]]["step"] = torch.tensor(10.0, device=DEV)
    run.o64.t[k] = run.o32.t[k] = 10
    return lambda: True


def _replace_step_cpu(run, opt, k):
    opt.state[run.params[k]]["step"] = torch.tensor(10.0)
    run.o64.t[k] = run.o32.t[k] = 10
    return lambda: True


def _clear_state(run, opt, k):
    opt.state[run.params[k]].clear()
    for o in (run.o64, run.o32):
        o.clear(k)
    return lambda: True


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("edit", [_replace_buffer, _replace_step, _replace_step_cpu, _clear_state],
                         ids=["buffer replaced", "step replaced", "step replaced (cpu)", "state cleared"])
def test_state_edited_between_steps(kind, edit):
    """torch's optimizers read ``state`` in every step, so an edit between two steps counts.  Gradient addresses stay fixed (the key of
    the prepared launches does not change); the oracle gets the same edit.  (SGD after ``state cleared``: the next update is a buffer
    copy again.)"""
    hyper = _hyper(kind, **FULL[kind])
    run = Run(kind, SHAPES, seed=15)
    opt = KINDS[kind][0](run.params, **hyper)
    for it in range(2):
        run.step(opt, run.random_grads(SCALES[it]), [(None, hyper)])
    run.check(opt, f"{edit.__name__}, before")
    torch.cuda.synchronize()
    still = edit(run, opt, 0)
    for it in range(2, 4):
        run.step(opt, run.random_grads(SCALES[it]), [(None, hyper)])
        run.check(opt, edit.__name__)
        assert still()


# ---- gradient forms -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("form", ["expanded", "transposed"])
def test_noncontiguous_gradient_assigned_every_step(kind, form):
    """A strided view as the gradient, the SAME view assigned before every step and its memory rewritten in between: the same result
    as with its contiguous copy, and as the oracle."""
    cls = KINDS[kind][0]
    hyper = _hyper(kind, **FULL[kind])
    run = Run(kind, [(48, 40), (300,)], seed=17)
    twin = [torch.nn.Parameter(p.detach().clone()) for p in run.params]
    opt, ref = cls(run.params, **hyper), cls(twin, **hyper)
    base = torch.zeros((1, 40) if form == "expanded" else (40, 48), device=DEV)
    view = base.expand(48, 40) if form == "expanded" else base.t()
    assert not view.is_contiguous() and view.shape == (48, 40)
    for it in range(4):
        grads = run.random_grads(SCALES[it])
        src = grads[0][:1] if form == "expanded" else np.ascontiguousarray(grads[0].T)
        base.copy_(_dev(src))
        grads[0] = _np(view).astype(np.float32)
        run.params[0].grad = view
        run.params[1].grad.copy_(_dev(grads[1]))
        for q, g in zip(twin, grads):
            q.grad = _dev(g)
        opt.step()
        ref.step()
        run.oracle_step(grads, [(None, hyper)])
        torch.cuda.synchronize()
        for p, q in zip(run.params, twin):
            assert torch.equal(p, q), it
            for name in _used(hyper):
                assert torch.equal(opt.state[p][name], ref.state[q][name]), (it, name)
        run.check(opt, f"{form} gradient")


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("set_to_none", [True, False])
def test_zero_grad_loops(kind, set_to_none):
    hyper = _hyper(kind, weight_decay=0.01, **FULL[kind])
    run = Run(kind, SHAPES, seed=18)
    opt = KINDS[kind][0](run.params, **hyper)
    for it in range(6):
        opt.zero_grad(set_to_none=set_to_none)
        grads = run.random_grads(SCALES[it])
        for p, g in zip(run.params, grads):
            if set_to_none:
                assert p.grad is None
                p.grad = _dev(g)                         # a fresh tensor, as autograd allocates one
            else:
                assert not bool(p.grad.any())
                p.grad.add_(_dev(g))                     # accumulated into the zeroed one
        opt.step()
        run.oracle_step(grads, [(None, hyper)])
        run.check(opt, f"zero_grad(set_to_none={set_to_none})")


@pytest.mark.parametrize("kind", list(KINDS))
def test_empty_parameter_passes_through(kind):
    cls = KINDS[kind][0]
    hyper = _hyper(kind, **FULL[kind])
    run = Run(kind, [(300,), (257,)], seed=19)
    empty = torch.nn.Parameter(torch.zeros(0, 4, device=DEV))
    empty.grad = torch.zeros_like(empty)
    opt = cls([run.params[0], empty, run.params[1]], **hyper)
    for it in range(3):
        run.step(opt, run.random_grads(SCALES[it]), [(None, hyper)])
    run.check(opt, "empty parameter")
    assert empty.shape == (0, 4)
    alone = cls([empty], **hyper)
    alone.step()
    torch.cuda.synchronize()


# ---- non-finite isolation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_nonfinite_gradient_elements_stay_where_they_are(kind):
    hyper = _hyper(kind, **FULL[kind])
    run = Run(kind, [(1500,), (300,)], seed=20)
    opt = KINDS[kind][0](run.params, **hyper)
    for it in range(3):
        grads = run.random_grads(SCALES[it])
        if it == 1:
            grads[0][7], grads[0][1300] = np.inf, np.nan
        run.step(opt, grads, [(None, hyper)])
    run.check(opt, "non-finite")                       # (finite elements within the bound, the others in the oracle's places)
    st = opt.state[run.params[0]]
    for t in [run.params[0]] + [st[name] for name in _used(hyper)]:
        assert (~torch.isfinite(t.detach())).nonzero().flatten().tolist() == [7, 1300]
    st = opt.state[run.params[1]]
    for t in [run.params[1]] + [st[name] for name in _used(hyper)]:
        assert bool(torch.isfinite(t.detach()).all())


# ---- the captured step ------------------------------------------------------------------------------------------------------------------
CAPTURED = [("sgd", dict(momentum=0.9, dampening=0.1)), ("sgd", dict(momentum=0.9, nesterov=True)), ("rmsprop", dict(centered=True, momentum=0.9))]


@pytest.mark.parametrize("kind,flags", CAPTURED, ids=["sgd momentum+dampening", "sgd nesterov", "rmsprop centered+momentum"])
def test_graphed_train_step_equals_eager_steps_of_the_same_class(kind, flags):
    """engine.GraphedTrainStep (1 warm-up step -- SGD's buffer copy -- and 5 replays of ONE captured launch, the tensor lr filled to a
    tenth before replay 2) is bit-equal to 6 eager steps on a twin: the captured arguments serve every step, the counts read 6."""
    cls = KINDS[kind][0]
    w = torch.nn.Parameter(torch.ones(64, 64, device=DEV))
    twin = torch.nn.Parameter(w.detach().clone())
    x = torch.randn(8, 64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(23))
    lr, lr_twin = torch.tensor(1e-2, device=DEV), torch.tensor(1e-2, device=DEV)
    opt, ref = cls([w], lr=lr, **flags), cls([twin], lr=lr_twin, **flags)
    # the graph's first node bumps the device's dropout epoch word, which is allocated at its first use -- never inside a capture, and
    # this toy has no dropout layer whose warm-up forward would have been there
    ops.dropout_epoch_add(0)
    step = engine.GraphedTrainStep(lambda: ((x @ w) ** 2).mean(), opt, warmup=1)
    for k in range(5):
        if k == 2:
            lr.fill_(1e-3)
        step()
    for k in range(6):
        if k == 3:                                       # (1 warm-up step + replays 0, 1 at 1e-2; replays 2 - 4 at 1e-3)
            lr_twin.fill_(1e-3)
        ref.zero_grad()
        ((x @ twin) ** 2).mean().backward()
        ref.step()
    torch.cuda.synchronize()
    assert float(opt.state[w]["step"]) == float(ref.state[twin]["step"]) == 6.0
    assert torch.equal(w, twin) and not torch.equal(w, torch.ones_like(w))
    for name in _used(dict(KINDS[kind][2], **flags)):
        assert torch.equal(opt.state[w][name], ref.state[twin][name]), name


def test_eval_after_graphed_sgd_training_sees_the_trained_state():
    """Three replayed steps with the SGD of ``optim.build`` (tensor lr) on the frame-16 / 3-aux-level model; eval-mode inference must
    equal a fresh model loaded with the trained state: the kernel's writes invalidate the caches of folded inference parameters."""
    from gpu_util import model_pair
    from echoglad_amd import data, losses

    def _setup(frame, naux, coord, seed):                # (tests/test_gpu_engine.py's)
        hip, _ = model_pair(frame, naux, 2, coord=coord, seed=seed)
        torch.manual_seed(seed)
        emb = torch.nn.Conv2d(1, 128, kernel_size=1).to(DEV)
        np.random.seed(seed)
        ds = data.SyntheticEchoDataset(num_aux_graphs=naux, frame_size=frame, use_coordinate_graph=coord)
        return hip, None, emb, None, ds
    frame, naux, B = 16, 3, 2
    hip, _, emb, _, ds = _setup(frame, naux, True, 5)
    batch = data.to_device(data.collate([ds[i] for i in range(B)], ds.topology), DEV)
    crit = {"bce": losses.WeightedBCEWithLogitsLoss("none", 9000, 1), "elm": losses.ExpectedLandmarkMSE(10, B, frame, naux), "coordinate": engine.MSE(1)}
    for q in emb.parameters():
        q.requires_grad_(False)
    model = {"embedder": emb, "landmark": hip}

    def infer(m):
        m.eval()
        with torch.no_grad():
            return [t.clone() for t in engine.forward_batch({"embedder": emb, "landmark": m}, batch, True)]

    first = infer(hip)                                   # (fills the caches of folded parameters / the inference graph)
    hip.train()
    config = {"name": "sgd", "lr": 1e-3, "momentum": 0.9}
    opt = optim.build(config, model, device_lr=True)
    assert type(opt) is SGD and config == {"name": "sgd", "lr": 1e-3, "momentum": 0.9}
    lr = opt.param_groups[0]["lr"]
    assert torch.is_tensor(lr) and lr.is_cuda and lr.dtype == torch.float32 and lr.dim() == 0

    def loss_fn():
        preds, cp = engine.forward_batch(model, batch, True)
        return engine.total_loss(engine.compute_loss(crit, preds, batch.y, cp, batch.node_coord_y, batch.valid_labels, B))
    step = engine.GraphedTrainStep(loss_fn, opt, warmup=2)
    for _ in range(3):
        step()
    got = infer(hip)
    assert not torch.equal(got[0], first[0])             # five steps moved it
    assert all(float(opt.state[p]["step"]) == 5.0 for p in hip.parameters() if p in opt.state) and len(opt.state) > 0
    fresh, _, _, _, _ = _setup(frame, naux, True, 6)
    fresh.load_state_dict({k: v.clone() for k, v in hip.state_dict().items()})
    want = infer(fresh)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
