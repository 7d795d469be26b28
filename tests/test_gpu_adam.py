"""-m gpu: echoglad_amd.optim.Adam (eg_adam_step, csrc/adam.hip: one launch per 96 tensors, step counts on the device) against
oracle/adam_oracle.py, a plain fp64 Adam in numpy that carries the step count per tensor.

Inputs are fp32 values, the oracle gets the same values cast up; the hyper-parameters are handed to the oracle as the C floats
eg_adam_step receives (tests/test_oracle.py says what that leaves out).  Tolerance of every oracle comparison, per tensor and per
array (p, exp_avg, exp_avg_sq):

    max|device - oracle64|  <=  4 * max(e32, ulp32(max|oracle64|)),        e32 = max|oracle32 - oracle64|

oracle32 being the same formulas with every operation rounded to fp32.  4: FMA contraction and another order of the operations in
the device code (exp_avg as m + (1 - b1)(g - m)) against numpy, over about eight rounded operations per element and step.
tests/test_oracle.py shows that a step count behind by one, a misplaced eps or a dropped weight decay are > 1000 of these bounds away.

Largest measured err / max(e32, ulp) per case on an MI355X (the bound is 4): NOT MEASURED YET -- this module has not run on a GPU.
Every check prints its figures before it asserts (``pytest tests/test_gpu_adam.py -s``: one ``ADAM_RATIO <case>: p, exp_avg,
exp_avg_sq`` line per check); the table belongs here.  With optim.py's real host logic and eg_adam_step replaced by a numpy stand-in
of the kernel's formulas on host memory (no FMA contraction), the largest ratios were 1.17 (p), 3.55 (exp_avg), 1.00 (exp_avg_sq).

Against the optim.py before the fix of the prepared-launch cache (same stand-in) these fail: test_stale_cache_* (every count 2 after
step C, where 3 and 2 are due), test_state_edited_between_steps[*], test_noncontiguous_gradient_assigned_every_step (a table kept
under the address of a strided view pointed at a copy that was gone) and test_empty_parameter_passes_through."""
import numpy as np
import pytest
import torch

from gpu_util import DEV
from oracle import adam_oracle as AO
from echoglad_amd.optim import Adam

pytestmark = pytest.mark.gpu

SCALES = (1.0, 0.3, 2.0, 0.7, 3.0, 1.5)                  # gradients scaled differently per step
CHUNK = 1024                                             # elements per workgroup: 256 threads x 4


def _c_floats(hyper):
    """The hyper-parameters as eg_adam_step receives them (C floats), for the oracle."""
    out = dict(hyper)
    for k in ("lr", "eps", "weight_decay"):
        if k in out:
            out[k] = AO.as_float32(float(out[k]))
    if "betas" in out:
        out["betas"] = tuple(AO.as_float32(b) for b in out["betas"])
    return out


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


class Run:
    """Device parameters (gradients allocated once and written in place, so their addresses never change) and the two oracles on the
    same values.  ``groups``: [(indices, hyper-parameters)] -- what the oracle applies to which tensors."""

    def __init__(self, shapes, seed=0, init=None):
        self.rs = np.random.RandomState(seed)
        init = [self.rs.standard_normal(s).astype(np.float32) for s in shapes] if init is None else init
        self.shapes = [a.shape for a in init]
        self.params = [torch.nn.Parameter(_dev(a)) for a in init]
        for p in self.params:
            p.grad = torch.zeros_like(p)
        self.parked = {}
        self.o64, self.o32 = AO.AdamOracle(init, np.float64), AO.AdamOracle(init, np.float32)
        self.worst = [0.0, 0.0, 0.0]

    def add(self, shapes):
        init = [self.rs.standard_normal(s).astype(np.float32) for s in shapes]
        new = [torch.nn.Parameter(_dev(a)) for a in init]
        for p in new:
            p.grad = torch.zeros_like(p)
        self.params += new
        self.shapes += [a.shape for a in init]
        for o in (self.o64, self.o32):
            o.add(init)
        return new

    def random_grads(self, scale=1.0, away_from_zero=False):
        gs = [self.rs.standard_normal(s) * scale for s in self.shapes]
        if away_from_zero:
            gs = [np.sign(g) * (0.5 + np.abs(g)) for g in gs]
        return [g.astype(np.float32) for g in gs]

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
        for idx, hyper in groups:
            for o in (self.o64, self.o32):
                o.step(grads, only=idx, **_c_floats(hyper))

    def check(self, opt, case):
        """Counts exact; p, exp_avg, exp_avg_sq of every tensor within the bound of the fp64 oracle (non-finite elements: in the same
        places).  Prints the figures before it asserts."""
        torch.cuda.synchronize()
        fails = []
        for k, p in enumerate(self.params):
            st = opt.state.get(p, {})
            t = float(st["step"]) if "step" in st else 0.0
            if t != float(self.o64.t[k]):
                fails.append(f"tensor {k}: step count {t}, oracle {self.o64.t[k]}")
            arrays = [(0, "p", _np(p), self.o32.p[k], self.o64.p[k])]
            if "exp_avg" in st:
                arrays += [(1, "exp_avg", _np(st["exp_avg"]), self.o32.m[k], self.o64.m[k]),
                           (2, "exp_avg_sq", _np(st["exp_avg_sq"]), self.o32.v[k], self.o64.v[k])]
            elif self.o64.t[k] != 0:
                fails.append(f"tensor {k}: no moments in the state after {self.o64.t[k]} updates")
            for j, name, got, w32, w64 in arrays:
                got, w64 = got.reshape(w64.shape), np.asarray(w64)
                ok = np.isfinite(w64)
                if not np.array_equal(np.isfinite(got), ok):
                    fails.append(f"tensor {k} {name}: non-finite elements at {np.flatnonzero(~np.isfinite(got))[:8]}, oracle at {np.flatnonzero(~ok)[:8]}")
                    continue
                if not ok.any():
                    continue
                err, unit = float(np.abs(got[ok] - w64[ok]).max()), AO.unit(w32, w64)
                self.worst[j] = max(self.worst[j], err / unit)
                if err > 4.0 * unit:
                    fails.append(f"tensor {k} {name}: err {err:.3e} = {err / unit:.2f} x max(e32, ulp) = {unit:.3e}")
        print(f"ADAM_RATIO {case}: p {self.worst[0]:.2f}  exp_avg {self.worst[1]:.2f}  exp_avg_sq {self.worst[2]:.2f}")
        assert not fails, (case, fails[:10], len(fails))


# Shapes of the oracle comparisons.  e32 is a maximum over the elements of a tensor, and so is the device's error: the two are comparable
# when the tensor has enough elements for the maxima to be typical.  With a handful of elements e32 is a sample of one -- any correct
# fp32 Adam is 4 e32 away from fp64 in one such tensor out of six or so (exp_avg after gradients of changing sign is small against the
# operands whose rounding it carries, so the ulp of the VALUE is no floor either).  So these tensors have >= 231 elements; single
# elements and tails of a few elements are covered by the chunk-edge test (gradients of constant sign per element: see there) and by
# the bit-equality and count tests below.
SHAPES = [(1500,), (33, 7), (300,)]                      # two workgroups, two partly filled workgroups


# ---- kernel arithmetic against fp64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hyper", [
    ("default", dict()),
    ("weight_decay", dict(weight_decay=0.01)),
    ("maximize", dict(maximize=True)),
    ("weight_decay+maximize", dict(weight_decay=0.01, maximize=True)),
    ("beta1=0", dict(betas=(0.0, 0.999))),
    ("beta2=0", dict(betas=(0.9, 0.0))),
    ("eps=1e-3", dict(eps=1e-3)),
    ("eps=0", dict(eps=0.0)),
    ("lr=1e-2", dict(lr=1e-2)),
])
def test_arithmetic_against_fp64(name, hyper):
    hyper = dict(dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False), **hyper)
    run = Run(SHAPES, seed=1)
    opt = Adam(run.params, **hyper)
    for it in range(6):
        run.step(opt, run.random_grads(SCALES[it], away_from_zero=name == "eps=0"), [(None, hyper)])
        run.check(opt, name)


def test_lr_zero_moves_moments_and_counts_only():
    hyper = dict(lr=0.0, betas=(0.9, 0.999), eps=1e-8)
    run = Run(SHAPES, seed=2)
    before = [p.detach().clone() for p in run.params]
    opt = Adam(run.params, **hyper)
    for it in range(6):
        run.step(opt, run.random_grads(SCALES[it]), [(None, hyper)])
    run.check(opt, "lr=0")
    for p, q in zip(run.params, before):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))             # bit-unchanged
        assert float(opt.state[p]["step"]) == 6.0
        assert float(opt.state[p]["exp_avg"].abs().max()) > 0 and float(opt.state[p]["exp_avg_sq"].abs().max()) > 0


def test_zero_gradient_leaves_parameters_alone():
    hyper = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
    run = Run(SHAPES, seed=3)
    before = [p.detach().clone() for p in run.params]
    opt = Adam(run.params, **hyper)
    for it in range(6):
        run.step(opt, [np.zeros(s, np.float32) for s in run.shapes], [(None, hyper)])
    run.check(opt, "zero gradient")
    for p, q in zip(run.params, before):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))
        st = opt.state[p]
        assert float(st["step"]) == 6.0
        assert bool(torch.isfinite(p).all()) and not bool(st["exp_avg"].any()) and not bool(st["exp_avg_sq"].any())


def test_lr_as_a_device_scalar_filled_between_steps():
    lr = torch.tensor(1e-3, device=DEV)
    hyper = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    run = Run(SHAPES, seed=4)
    opt = Adam(run.params, lr=lr, **hyper)
    for it, value in enumerate([1e-3, 1e-3, 5e-4, 5e-4, 2e-3, 1e-4]):
        lr.fill_(value)
        run.step(opt, run.random_grads(SCALES[it]), [(None, dict(hyper, lr=value))])
        run.check(opt, "tensor lr")


def test_two_param_groups_in_one_optimizer():
    run = Run(SHAPES + [(2049,), (257,)], seed=5)
    ha = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    hb = dict(lr=3e-2, betas=(0.5, 0.9), eps=1e-8, weight_decay=0.1)
    opt = Adam([dict(params=run.params[:3], **ha), dict(params=run.params[3:], **hb)])
    for it in range(6):
        run.step(opt, run.random_grads(SCALES[it]), [([0, 1, 2], ha), ([3, 4], hb)])
        run.check(opt, "two groups")


def test_hyper_parameters_changed_between_steps():
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    run = Run(SHAPES, seed=6)
    opt = Adam(run.params, **hyper)
    changes = {2: dict(lr=5e-3), 3: dict(betas=(0.8, 0.99)), 4: dict(weight_decay=0.05)}
    for it in range(6):
        hyper = dict(hyper, **changes.get(it, {}))
        opt.param_groups[0].update(changes.get(it, {}))
        run.step(opt, run.random_grads(SCALES[it]), [(None, hyper)])
        run.check(opt, "hyper-parameters changed")


# ---- late steps: the fp64 pow of the bias corrections ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["cpu tensor", "number"])
@pytest.mark.parametrize("t0", [1000, 100000])
def test_late_steps_from_a_loaded_state(t0, form):
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    run = Run(SHAPES, seed=7)
    opt = Adam(run.params, **hyper)
    sd = opt.state_dict()
    for k, s in enumerate(run.shapes):
        m0 = (run.rs.standard_normal(s) * 0.3).astype(np.float32)
        v0 = (run.rs.standard_normal(s) ** 2 * 0.2).astype(np.float32)
        sd["state"][k] = {"step": torch.tensor(float(t0)) if form == "cpu tensor" else t0,
                          "exp_avg": torch.from_numpy(m0.copy()), "exp_avg_sq": torch.from_numpy(v0.copy())}
        for o in (run.o64, run.o32):
            o.m[k], o.v[k], o.t[k] = m0.astype(o.dtype), v0.astype(o.dtype), t0
    opt.load_state_dict(sd)
    for it in range(3):
        run.step(opt, run.random_grads(SCALES[it]), [(None, hyper)])
        run.check(opt, f"t0={t0}")
    for p in run.params:
        assert float(opt.state[p]["step"]) == float(t0 + 3)
    assert all(float(s["step"]) == float(t0 + 3) for s in opt.state_dict()["state"].values())


# ---- chunk edges and bounds ---------------------------------------------------------------------------------------------------------
SENTINEL = -7.25e10
EDGE_NUMELS = (1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)


def _guarded(n, first, fill):
    """(buffer, the slice [first, first + n) of it): 64 sentinels on both sides, the slice 4-byte but not 16-byte aligned."""
    buf = torch.full((first + n + 64,), SENTINEL, device=DEV)
    assert first >= 64 and buf.data_ptr() % 16 == 0 and first % 4 != 0
    view = buf[first:first + n]
    view.copy_(fill)
    assert view.data_ptr() % 16 != 0 and view.data_ptr() % 4 == 0 and view.is_contiguous()
    return buf, view


def test_chunk_edges_unaligned_slices_and_sentinels():
    """Every tensor a slice of a larger buffer, 4-byte but not 16-byte aligned, sentinels around it.  The sizes go down to one element,
    where e32 is no yardstick (see SHAPES), so the gradients keep their sign per element over the 3 steps, |g| in scale * [0.5, 1.5]:
    exp_avg and exp_avg_sq then grow without cancellation, every rounding is a fraction of an ulp of the result (about 0.9 per step
    for exp_avg, 1.1 for exp_avg_sq, 0.5 for p), and 3 steps stay below 4 ulps of the final value in the worst case, whatever e32 is."""
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    rs = np.random.RandomState(8)
    init = [rs.standard_normal(n).astype(np.float32) for n in EDGE_NUMELS]
    run = Run(None, seed=8, init=init)
    buffers, params = [], []
    for k, n in enumerate(EDGE_NUMELS):
        first = [65 + (k + j) % 3 for j in range(4)]    # 65, 66 or 67 floats into a 16-byte aligned buffer, another one per array
        pb, pv = _guarded(n, first[0], _dev(init[k]))
        gb, gv = _guarded(n, first[1], torch.zeros(n, device=DEV))
        mb, mv = _guarded(n, first[2], torch.zeros(n, device=DEV))
        vb, vv = _guarded(n, first[3], torch.zeros(n, device=DEV))
        p = torch.nn.Parameter(pv)
        assert p.data_ptr() == pv.data_ptr()
        p.grad = gv
        buffers.append(((pb, gb, mb, vb), first, n))
        params.append((p, mv, vv))
    run.params = [p for p, _, _ in params]
    opt = Adam(run.params, **hyper)
    for p, mv, vv in params:                             # moments installed before the first step: the slices are what the kernel writes
        opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"] = mv, vv
    signs = [np.sign(g) for g in run.random_grads()]
    for it in range(3):
        grads = [(s * (0.5 + rs.random_sample(s.shape)) * SCALES[it]).astype(np.float32) for s in signs]
        run.step(opt, grads, [(None, hyper)])
        for p, mv, vv in params:
            assert opt.state[p]["exp_avg"] is mv and opt.state[p]["exp_avg_sq"] is vv and p.grad.data_ptr() % 16 != 0
    run.check(opt, "chunk edges")
    for bufs, first, n in buffers:
        for name, buf, lo in zip(("p", "grad", "exp_avg", "exp_avg_sq"), bufs, first):
            bits, want = buf.view(torch.int32), torch.full_like(buf, SENTINEL).view(torch.int32)
            assert lo >= 64 and buf.numel() == lo + n + 64
            assert torch.equal(bits[:lo], want[:lo]) and torch.equal(bits[lo + n:], want[lo + n:]), (n, name)


# ---- workgroup -> (tensor, chunk) look-up -------------------------------------------------------------------------------------------
def _lookup_numels(count, where):
    """count tensors with 1, 2 or 5 chunks mixed (some ending on a chunk boundary, some before it) and ONE of 17 chunks."""
    chunks = [(1, 2, 5)[(k * 7 + k // 3) % 3] for k in range(count)]
    chunks[{"first": 0, "middle": count // 2, "last": count - 1}[where]] = 17
    return [c * CHUNK - (0, 1, 5, 1023)[k % 4] for k, c in enumerate(chunks)]


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("count", [96, 97, 192, 193])
def test_workgroup_lookup_one_optimizer_equals_one_optimizer_per_tensor(count, where):
    """Every workgroup must find its own (tensor, chunk): the list under ONE optimizer (launches of 96 tensors) is bit-equal to every
    tensor under an optimizer of its own (one tensor per launch: the look-up is trivial)."""
    hyper = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    numels = _lookup_numels(count, where)
    assert {-(-n // CHUNK) for n in numels} == {1, 2, 5, 17}
    gen = torch.Generator(device=DEV).manual_seed(9)
    a = [torch.nn.Parameter(torch.randn(n, device=DEV, generator=gen)) for n in numels]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    one, each = Adam(a, **hyper), [Adam([q], **hyper) for q in b]
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
        assert torch.equal(one.state[p]["exp_avg"], o.state[q]["exp_avg"]), (k, numels[k])
        assert torch.equal(one.state[p]["exp_avg_sq"], o.state[q]["exp_avg_sq"]), (k, numels[k])
        assert float(one.state[p]["step"]) == float(o.state[q]["step"]) == 3.0
        assert bool((one.state[p]["exp_avg_sq"] > 0).any())


# ---- step counts are exact ----------------------------------------------------------------------------------------------------------
COUNT_SHAPES = [(128, 128), (128,), (32, 136), (2, 16), (1,), (4097,)] + [(7,)] * 100       # 106 tensors: launches of 119 and 10 workgroups


def _plain_steps(shapes, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, device=DEV, generator=gen)) for s in shapes]
    for p in ps:
        p.grad = torch.randn(p.shape, device=DEV, generator=gen)
    return ps, Adam(ps, lr=1e-3)


def test_step_counts_after_50_steps_two_launches_per_step():
    ps, opt = _plain_steps(COUNT_SHAPES, 10)
    for _ in range(50):
        opt.step()
    torch.cuda.synchronize()
    assert [float(opt.state[p]["step"]) for p in ps] == [50.0] * len(ps)
    assert [float(s["step"]) for s in opt.state_dict()["state"].values()] == [50.0] * len(ps)


def test_step_counts_after_50_steps_one_workgroup():
    ps, opt = _plain_steps([(5,)], 11)
    for _ in range(50):
        opt.step()
    torch.cuda.synchronize()
    assert float(opt.state[ps[0]]["step"]) == 50.0


def test_step_counts_two_optimizers_on_two_streams():
    """Two optimizers stepped alternately, each on a stream of its own (a ticket word per stream): counts exact, and the parameters
    bit-equal to the same two optimizers stepped one after the other on one stream."""
    (pa, oa), (pb, ob) = _plain_steps(COUNT_SHAPES, 12), _plain_steps(COUNT_SHAPES[3:40], 13)
    (qa, ra), (qb, rb) = _plain_steps(COUNT_SHAPES, 12), _plain_steps(COUNT_SHAPES[3:40], 13)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(50):
        with torch.cuda.stream(sa):
            oa.step()
        with torch.cuda.stream(sb):
            ob.step()
    for _ in range(50):
        ra.step()
    for _ in range(50):
        rb.step()
    torch.cuda.synchronize()
    for ps, opt, qs in ((pa, oa, qa), (pb, ob, qb)):
        assert [float(opt.state[p]["step"]) for p in ps] == [50.0] * len(ps)
        for p, q in zip(ps, qs):
            assert torch.equal(p, q)


# ---- the stale prepared launch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes,skipped", [(SHAPES, 1), ([(1100,)] + [(300,)] * 104 + [(2049,)], 5)], ids=["3 tensors", "106 tensors"])
def test_stale_cache_a_step_without_one_gradient_in_between(shapes, skipped):
    """A: every parameter.  B: one parameter's gradient is None.  C: every parameter again, the gradients where they were in A -- the
    key of A's prepared launches, whose count array stood still during B.  (106 tensors: the skipped one is in the first launch, so
    the split into launches of 96 is shifted in B.)"""
    hyper = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
    run = Run(shapes, seed=14)
    opt = Adam(run.params, **hyper)
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
            print(f"ADAM_STALE {len(shapes)} tensors: counts after C {sorted(set(counts))}, of the skipped one {counts[skipped]}")
            assert counts == [2.0 if k == skipped else 3.0 for k in range(len(shapes))]
        if name in "CD":
            run.check(opt, f"stale cache, {len(shapes)} tensors, after {name}")


# ---- state edited between steps -----------------------------------------------------------------------------------------------------
def _replace_exp_avg(run, opt, k):
    new = (run.rs.standard_normal(run.shapes[k]) * 0.3).astype(np.float32)
    t = _dev(new)
    opt.state[run.params[k]]["exp_avg"] = t
    for o in (run.o64, run.o32):
        o.m[k] = new.astype(o.dtype)
    return lambda: opt.state[run.params[k]]["exp_avg"] is t


def _zero_exp_avg_sq(run, opt, k):
    t = torch.zeros_like(run.params[k])
    opt.state[run.params[k]]["exp_avg_sq"] = t
    for o in (run.o64, run.o32):
        o.v[k] = np.zeros_like(o.v[k])
    return lambda: opt.state[run.params[k]]["exp_avg_sq"] is t and bool((t > 0).any())


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
        o.m[k], o.v[k], o.t[k] = np.zeros_like(o.m[k]), np.zeros_like(o.v[k]), 0
    return lambda: True


@pytest.mark.parametrize("edit", [_replace_exp_avg, _zero_exp_avg_sq, _replace_step, _replace_step_cpu, _clear_state],
                         ids=["exp_avg replaced", "exp_avg_sq zeroed", "step replaced", "step replaced (cpu)", "state cleared"])
def test_state_edited_between_steps(edit):
    """torch's optimizers read ``state`` in every step, so an edit between two steps counts.  Gradient addresses stay fixed (the key of
    the prepared launches does not change); the oracle gets the same edit."""
    hyper = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
    run = Run(SHAPES, seed=15)
    opt = Adam(run.params, **hyper)
    for it in range(2):
        run.step(opt, run.random_grads(SCALES[it]), [(None, hyper)])
    run.check(opt, f"{edit.__name__}, before")
    torch.cuda.synchronize()
    still = edit(run, opt, 0)
    for it in range(2, 4):
        run.step(opt, run.random_grads(SCALES[it]), [(None, hyper)])
        run.check(opt, edit.__name__)
        assert still()


def test_add_param_group_after_two_steps():
    ha = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    hb = dict(lr=1e-3, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.01)
    run = Run(SHAPES, seed=16)
    opt = Adam(run.params, **ha)
    groups = [([0, 1, 2], ha)]
    for it in range(4):
        if it == 2:
            opt.add_param_group(dict(params=run.add([(1025,), (260,)]), **hb))
            groups.append(([3, 4], hb))
        run.step(opt, run.random_grads(SCALES[it]), groups)
        run.check(opt, "add_param_group")
    assert [float(opt.state[p]["step"]) for p in run.params] == [4.0, 4.0, 4.0, 2.0, 2.0]


# ---- gradient forms -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["expanded", "transposed"])
def test_noncontiguous_gradient_assigned_every_step(form):
    """A strided view as the gradient, the SAME view assigned before every step and its memory rewritten in between (what a hook or a
    hand-written backward does): the same result as with its contiguous copy, and as the oracle."""
    hyper = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
    run = Run([(48, 40), (300,)], seed=17)
    twin = [torch.nn.Parameter(p.detach().clone()) for p in run.params]
    opt, ref = Adam(run.params, **hyper), Adam(twin, **hyper)
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
        for o in (run.o64, run.o32):
            o.step(grads, **_c_floats(hyper))
        torch.cuda.synchronize()
        for p, q in zip(run.params, twin):
            assert torch.equal(p, q), it
            assert torch.equal(opt.state[p]["exp_avg"], ref.state[q]["exp_avg"]) and torch.equal(opt.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"]), it
        run.check(opt, f"{form} gradient")


@pytest.mark.parametrize("set_to_none", [True, False])
def test_zero_grad_loops(set_to_none):
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    run = Run(SHAPES, seed=18)
    opt = Adam(run.params, **hyper)
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
        for o in (run.o64, run.o32):
            o.step(grads, **_c_floats(hyper))
        run.check(opt, f"zero_grad(set_to_none={set_to_none})")


def test_empty_parameter_passes_through():
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    run = Run([(300,), (257,)], seed=19)
    empty = torch.nn.Parameter(torch.zeros(0, 4, device=DEV))
    empty.grad = torch.zeros_like(empty)
    opt = Adam([run.params[0], empty, run.params[1]], **hyper)
    for it in range(3):
        run.step(opt, run.random_grads(SCALES[it]), [(None, hyper)])
    run.check(opt, "empty parameter")
    assert empty.shape == (0, 4)
    alone = Adam([empty], **hyper)
    alone.step()
    torch.cuda.synchronize()


# ---- non-finite isolation -----------------------------------------------------------------------------------------------------------
def test_nonfinite_gradient_elements_stay_where_they_are():
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    run = Run([(1500,), (300,)], seed=20)
    opt = Adam(run.params, **hyper)
    for it in range(3):
        grads = run.random_grads(SCALES[it])
        if it == 1:
            grads[0][7], grads[0][1300] = np.inf, np.nan
        run.step(opt, grads, [(None, hyper)])
    run.check(opt, "non-finite")                       # (finite elements within the bound, the others in the oracle's places)
    st = opt.state[run.params[0]]
    for t in (run.params[0], st["exp_avg"], st["exp_avg_sq"]):
        assert (~torch.isfinite(t.detach())).nonzero().flatten().tolist() == [7, 1300]
    st = opt.state[run.params[1]]
    for t in (run.params[1], st["exp_avg"], st["exp_avg_sq"]):
        assert bool(torch.isfinite(t.detach()).all())
