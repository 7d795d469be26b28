"""CPU: the host side of the one-launch SGD and RMSprop (csrc/optim.hip, echoglad_amd/optim.py) -- the refusals of eg_sgd_step /
eg_rmsprop_step (and eg_adam_step, csrc/adam.hip: one host function, csrc/multi_tensor.h) that come before any HIP call, the registry and builder, the state-dict round trip with torch's classes and the
prepared-launch cache walked on CPU tensors.  Nothing is launched."""
import copy
import ctypes as ct
import re

import pytest
import torch

from echoglad_amd import _lib, optim
from echoglad_amd.optim import SGD, Adam, RMSprop, _prepared_valid

SGD_MAX, RMSPROP_MAX, ADAM_MAX = 120, 84, 96


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_abi_155():
    text = open(_lib.HEADER_PATH).read()
    flat = re.sub(r"\s+", " ", text)
    assert _lib.ABI_VERSION >= 155 and f"#define EG_ABI_VERSION {_lib.ABI_VERSION}" in text
    assert re.search(r"\* 155: eg_sgd_step, eg_rmsprop_step", flat)
    assert "155: eg_sgd_step, eg_rmsprop_step" in open(_lib.__file__).read()
    assert f"#define EG_SGD_MAX_TENSORS {SGD_MAX}" in text and f"#define EG_RMSPROP_MAX_TENSORS {RMSPROP_MAX}" in text
    assert (optim._SGD_MAX_TENSORS, optim._RMSPROP_MAX_TENSORS, optim._MAX_TENSORS) == (SGD_MAX, RMSPROP_MAX, 96)
    assert f"#define EG_ADAM_MAX_TENSORS {ADAM_MAX}" in text and optim._MAX_TENSORS == ADAM_MAX
    f, p, i = ct.c_float, ct.c_void_p, ct.c_int
    assert _lib.SIGNATURES["eg_sgd_step"] == (i, [p, i, p, f, p, f, f, f, i, i, p])
    assert _lib.SIGNATURES["eg_rmsprop_step"] == (i, [p, i, p, f, p, f, f, f, f, i, i, p])
    assert {"eg_sgd_step", "eg_rmsprop_step"} <= _lib.TAKES_STREAM
    # the ctypes entries follow the header's field order
    for cls, name in ((optim._SGDTensor, "eg_sgd_tensor"), (optim._RMSpropTensor, "eg_rmsprop_tensor"), (optim._AdamTensor, "eg_adam_tensor")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
        assert [n for n, _ in cls._fields_] == re.findall(r"(\w+);", body)
        assert ct.sizeof(cls) == 8 * len(cls._fields_)


# ---- refusals before the first HIP call ------------------------------------------------------------------------------------------------
FAKE = 0x1000                                            # never dereferenced: every call below returns before any launch


def _sgd_table(count, buf=FAKE, numel=8):
    return (optim._SGDTensor * max(count, 1))(*[optim._SGDTensor(FAKE, FAKE, buf, numel) for _ in range(count)])


def _rms_table(count, ga=None, buf=None, numel=8, sq=FAKE):
    return (optim._RMSpropTensor * max(count, 1))(*[optim._RMSpropTensor(FAKE, FAKE, sq, ga, buf, numel) for _ in range(count)])


def _sgd(lib, table, count, steps=FAKE, momentum=0.0, dampening=0.0, wd=0.0, nesterov=0):
    return lib.eg_sgd_step(table, count, steps, 1e-3, None, momentum, dampening, wd, nesterov, 0, None)


def _rms(lib, table, count, steps=FAKE, alpha=0.99, eps=1e-8, wd=0.0, momentum=0.0, centered=0):
    return lib.eg_rmsprop_step(table, count, steps, 1e-2, None, alpha, eps, wd, momentum, centered, 0, None)


def test_sgd_step_refusals(built_lib):
    lib = _lib.load()
    ARG, UNS = _lib.EG_ERR_ARG, _lib.EG_ERR_UNSUPPORTED
    t = _sgd_table(2)
    assert _sgd(lib, None, 2) == ARG and _sgd(lib, t, 2, steps=None) == ARG and _sgd(lib, t, -1) == ARG
    assert _sgd(lib, t, 2, momentum=-0.1) == ARG and "momentum" in _lib.last_error()
    assert _sgd(lib, t, 2, momentum=float("nan")) == ARG
    assert _sgd(lib, t, 2, wd=-1e-3) == ARG and "weight_decay" in _lib.last_error()
    assert _sgd(lib, t, 2, nesterov=1) == ARG and "nesterov" in _lib.last_error()                      # momentum 0
    assert _sgd(lib, t, 2, nesterov=1, momentum=0.9, dampening=0.1) == ARG
    assert _sgd(lib, _sgd_table(2, buf=None), 2, momentum=0.9) == ARG and "buffer" in _lib.last_error()
    assert _sgd(lib, _sgd_table(2, numel=0), 2) == ARG and _sgd(lib, _sgd_table(2, numel=1 << 31), 2) == ARG
    bad = _sgd_table(2)
    bad[1].grad = None
    assert _sgd(lib, bad, 2) == ARG
    assert _sgd(lib, _sgd_table(SGD_MAX + 1), SGD_MAX + 1) == UNS and "split" in _lib.last_error()
    assert _sgd(lib, _sgd_table(SGD_MAX + 1), SGD_MAX + 1, momentum=0.9) == UNS
    assert _sgd(lib, _sgd_table(SGD_MAX + 1), SGD_MAX + 1, momentum=-1.0) == ARG                      # (a bad hyper-parameter first)
    assert _sgd(lib, t, 0) == _lib.EG_OK                                                              # nothing to do, nothing launched


def test_rmsprop_step_refusals(built_lib):
    lib = _lib.load()
    ARG, UNS = _lib.EG_ERR_ARG, _lib.EG_ERR_UNSUPPORTED
    t = _rms_table(2)
    assert _rms(lib, None, 2) == ARG and _rms(lib, t, 2, steps=None) == ARG and _rms(lib, t, -1) == ARG
    for kw in (dict(alpha=-0.1), dict(eps=-1e-8), dict(wd=-1e-3), dict(momentum=-0.5), dict(alpha=float("nan"))):
        assert _rms(lib, t, 2, **kw) == ARG, kw
    # grad_avg exactly when centered, momentum_buffer exactly when momentum > 0
    assert _rms(lib, t, 2, centered=1) == ARG and "grad_avg" in _lib.last_error()
    assert _rms(lib, _rms_table(2, ga=FAKE), 2) == ARG and "grad_avg" in _lib.last_error()
    assert _rms(lib, t, 2, momentum=0.9) == ARG and "momentum_buffer" in _lib.last_error()
    assert _rms(lib, _rms_table(2, buf=FAKE), 2) == ARG and "momentum_buffer" in _lib.last_error()
    assert _rms(lib, _rms_table(2, ga=FAKE, buf=FAKE), 2, centered=1) == ARG
    assert _rms(lib, _rms_table(2, sq=None), 2) == ARG
    assert _rms(lib, _rms_table(2, numel=0), 2) == ARG and _rms(lib, _rms_table(2, numel=1 << 31), 2) == ARG
    assert _rms(lib, _rms_table(RMSPROP_MAX + 1), RMSPROP_MAX + 1) == UNS and "split" in _lib.last_error()
    assert _rms(lib, _rms_table(RMSPROP_MAX + 1, ga=FAKE, buf=FAKE), RMSPROP_MAX + 1, centered=1, momentum=0.9) == UNS
    assert _rms(lib, t, 0) == _lib.EG_OK


def _adam_table(count, m=FAKE, v=FAKE, numel=8):
    return (optim._AdamTensor * max(count, 1))(*[optim._AdamTensor(FAKE, FAKE, m, v, numel) for _ in range(count)])


def _adam(lib, table, count, steps=FAKE, beta1=0.9, beta2=0.999, eps=1e-8):
    return lib.eg_adam_step(table, count, steps, 1e-3, None, beta1, beta2, eps, 0.0, 0, None)


def test_adam_step_refusals(built_lib):
    lib = _lib.load()
    ARG, UNS = _lib.EG_ERR_ARG, _lib.EG_ERR_UNSUPPORTED
    t = _adam_table(2)
    assert _adam(lib, None, 2) == ARG and _adam(lib, t, 2, steps=None) == ARG and _adam(lib, t, -1) == ARG
    for kw in (dict(beta1=-0.1), dict(beta1=1.0), dict(beta2=-0.1), dict(beta2=1.0), dict(beta1=float("nan")), dict(beta2=float("nan")),
               dict(eps=-1e-8)):
        assert _adam(lib, t, 2, **kw) == ARG and "betas" in _lib.last_error(), kw
    assert _adam(lib, _adam_table(2, m=None), 2) == ARG and _adam(lib, _adam_table(2, v=None), 2) == ARG
    assert _adam(lib, _adam_table(2, numel=0), 2) == ARG and _adam(lib, _adam_table(2, numel=1 << 31), 2) == ARG
    bad = _adam_table(2)
    bad[1].grad = None
    assert _adam(lib, bad, 2) == ARG
    assert _adam(lib, _adam_table(ADAM_MAX + 1), ADAM_MAX + 1) == UNS and "split" in _lib.last_error()
    assert _adam(lib, _adam_table(ADAM_MAX + 1), ADAM_MAX + 1, beta1=1.5) == ARG                      # (a bad hyper-parameter first)
    assert _adam(lib, t, 0) == _lib.EG_OK                                                             # nothing to do, nothing launched


def test_constructor_checks_are_torchs():
    p = torch.nn.Parameter(torch.zeros(3))
    for kw in (dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-1.0), dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1)):
        with pytest.raises(ValueError):
            SGD([p], **kw)
        with pytest.raises(ValueError):
            torch.optim.SGD([p], **dict(dict(lr=1e-3), **kw))
    for kw in (dict(lr=-1.0), dict(eps=-1e-8), dict(momentum=-0.1), dict(weight_decay=-1.0), dict(alpha=-0.5)):
        with pytest.raises(ValueError):
            RMSprop([p], **kw)
        with pytest.raises(ValueError):
            torch.optim.RMSprop([p], **kw)
    for opt in (SGD([p]), RMSprop([p])):
        assert opt.param_groups[0]["capturable"] is True                          # (what engine.GraphedTrainStep looks for)
        opt.step()                                                               # no gradient anywhere: nothing launched
        assert p not in opt.state                                                # never had a gradient: no state
    assert SGD([p]).defaults["lr"] == 1e-3 and RMSprop([p]).defaults["lr"] == 1e-2
    p.grad = torch.ones(3)
    for opt in (SGD([p]), RMSprop([p])):
        with pytest.raises(RuntimeError):
            opt.step()                                                           # a CPU parameter: refused before any launch


# ---- registry and builder --------------------------------------------------------------------------------------------------------------
def test_registry_and_builder_give_the_reference_parameter_order():
    assert optim.OPTIMIZERS == {"sgd": SGD, "rmsprop": RMSprop, "adam": Adam}
    models = {"landmark": torch.nn.Linear(3, 2), "embedder": torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 3))}
    want = list(models["embedder"].parameters()) + list(models["landmark"].parameters())

    class Log:
        lines = []

        def infov(self, m):
            self.lines.append(m)
    for cfg, cls in (({"name": "sgd", "lr": 0.1, "momentum": 0.9, "nesterov": True}, SGD),
                     ({"name": "rmsprop", "lr": 0.01, "centered": True}, RMSprop),
                     ({"name": "adam", "lr": 1e-4, "betas": [0.9, 0.99]}, Adam)):
        before = copy.deepcopy(cfg)
        opt = optim.build(cfg, models, Log())
        assert type(opt) is cls and cfg == before                                # name still in the caller's config
        got = [p for g in opt.param_groups for p in g["params"]]
        assert len(got) == len(want) == 6 and all(a is b for a, b in zip(got, want))
        assert opt.param_groups[0]["lr"] == cfg["lr"] and opt.param_groups[0]["capturable"]
    assert len(Log.lines) == 3 and "SGD" in Log.lines[0]
    assert type(optim.build({"name": "sgd"}, models)) is SGD                     # no logger
    with pytest.raises(KeyError, match="rmsprop"):
        optim.build({"name": "adagrad", "lr": 0.1}, models)
    with pytest.raises(RuntimeError):
        optim.build({"name": "sgd"}, models, device_lr=True)                     # (CPU models: no device to put the lr on)


# ---- the prepared launches on CPU tensors ----------------------------------------------------------------------------------------------
KINDS = {
    "sgd": (SGD, dict(momentum=0.9), ("momentum_buffer",)),
    "sgd, no momentum": (SGD, dict(), ()),
    "rmsprop": (RMSprop, dict(), ("square_avg",)),
    "rmsprop, centered + momentum": (RMSprop, dict(centered=True, momentum=0.9), ("square_avg", "grad_avg", "momentum_buffer")),
}


def _on_cpu(kind, n):
    cls, kw, names = KINDS[kind]
    ps = [torch.nn.Parameter(torch.full((3,), float(k))) for k in range(n)]
    for p in ps:
        p.grad = torch.ones(3)
    return cls(ps, **kw), ps, names


def _host_step(opt, ps):
    """step() without the launch: look the prepared launches up, then do to the counts what the kernel does."""
    with_grad = [p for p in ps if p.grad is not None]
    launches = opt._launches_of(0, with_grad, [p.grad for p in with_grad], on_device=False)
    for _part, _table, counts, _views, _tensors in launches:
        counts += 1.0
    return launches


@pytest.mark.parametrize("kind", list(KINDS))
def test_launch_split_at_the_per_launch_maximum(kind):
    cls = KINDS[kind][0]
    cap = SGD_MAX if cls is SGD else RMSPROP_MAX
    assert cls._MAX == cap
    for n, want in ((cap, [cap]), (cap + 1, [cap, 1]), (2 * cap + 1, [cap, cap, 1])):
        opt, ps, names = _on_cpu(kind, n)
        launches = _host_step(opt, ps)
        assert [len(l[0]) for l in launches] == want == [len(l[1]) for l in launches] == [l[2].numel() for l in launches]
        flat = [p for l in launches for p in l[0]]
        assert all(a is b for a, b in zip(flat, ps))
        for l in launches:
            for k, p in enumerate(l[0]):
                e, st = l[1][k], opt.state[p]
                assert (e.param, e.grad, e.numel) == (p.data_ptr(), p.grad.data_ptr(), 3)
                for field in ("momentum_buffer", "square_avg", "grad_avg"):
                    if hasattr(e, field):
                        assert getattr(e, field) == (st[field].data_ptr() if field in names else None), field
                assert set(st) == set(names) | {"step"} and st["step"] is l[3][k] and float(st["step"]) == 1.0


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n,skipped", [(3, 1), (130, 5)])
def test_prepared_launch_is_dropped_when_a_step_in_between_moved_the_counts(kind, n, skipped):
    opt, ps, names = _on_cpu(kind, n)
    a = _host_step(opt, ps)
    assert _prepared_valid(opt.state, a, names) and _host_step(opt, ps) is a     # nothing moved: kept, and used again
    parked, ps[skipped].grad = ps[skipped].grad, None
    b = _host_step(opt, ps)
    assert b is not a and not _prepared_valid(opt.state, a, names) and _prepared_valid(opt.state, b, names)
    ps[skipped].grad = parked
    c = _host_step(opt, ps)
    assert c is not a and _prepared_valid(opt.state, c, names)
    assert [float(opt.state[p]["step"]) for p in ps] == [3.0 if k == skipped else 4.0 for k in range(n)]
    assert _host_step(opt, ps) is c
    for launch in c:                                                             # the table's counts ARE the state's
        for p, view in zip(launch[0], launch[3]):
            assert opt.state[p]["step"] is view


def _edit_buffer(opt, p, names):
    opt.state[p][names[-1]] = torch.full((3,), 0.5)
    return 3.0


def _edit_step(opt, p, names):
    opt.state[p]["step"] = torch.tensor(7.0)
    return 8.0


def _edit_step_number(opt, p, names):
    opt.state[p]["step"] = 7
    return 8.0


def _edit_clear(opt, p, names):
    opt.state[p].clear()
    return 1.0


def _edit_delete(opt, p, names):
    del opt.state[p]
    return 1.0


@pytest.mark.parametrize("kind", ["sgd", "rmsprop", "rmsprop, centered + momentum"])
@pytest.mark.parametrize("edit", [_edit_buffer, _edit_step, _edit_step_number, _edit_clear, _edit_delete])
def test_prepared_launch_is_dropped_when_the_state_was_edited(kind, edit):
    opt, ps, names = _on_cpu(kind, 3)
    a = _host_step(opt, ps)
    assert _host_step(opt, ps) is a
    step_after = edit(opt, ps[1], names)
    installed = {k: v for k, v in opt.state.get(ps[1], {}).items() if torch.is_tensor(v) and k != "step"}
    assert not _prepared_valid(opt.state, a, names)
    b = _host_step(opt, ps)
    assert b is not a and _prepared_valid(opt.state, b, names)
    st = opt.state[ps[1]]
    for k, v in installed.items():                                               # the tensor the user put there is the one in the table
        assert st[k] is v and v.data_ptr() == getattr(b[0][1][1], k)
    assert float(st["step"]) == step_after and float(opt.state[ps[0]]["step"]) == 3.0
    assert all(st[nm].shape == (3,) for nm in names)


@pytest.mark.parametrize("kind", ["sgd", "rmsprop, centered + momentum"])
def test_prepared_launch_survives_what_does_not_move_the_state(kind):
    opt, ps, names = _on_cpu(kind, 3)
    a = _host_step(opt, ps)
    opt.state[ps[0]][names[0]].zero_()
    opt.state[ps[2]]["step"].fill_(11.0)
    ps[0].grad.copy_(torch.full((3,), 4.0))
    opt.param_groups[0]["lr"] = 0.5
    opt.param_groups[0]["weight_decay"] = 0.1
    assert _prepared_valid(opt.state, a, names) and _host_step(opt, ps) is a
    assert float(opt.state[ps[2]]["step"]) == 12.0
    sd = opt.state_dict()
    assert _prepared_valid(opt.state, a, names)
    opt.load_state_dict(sd)
    assert _host_step(opt, ps) is not a                                          # (loading moves everything: new tensors)


def test_switching_the_momentum_on_changes_the_tables_and_restarts_the_count():
    """The state tensors in use are part of the cache key; SGD's count says how many updates the BUFFER has had."""
    opt, ps, _ = _on_cpu("sgd, no momentum", 2)
    a = _host_step(opt, ps)
    assert _host_step(opt, ps) is a and a[0][1][0].momentum_buffer is None and "momentum_buffer" not in opt.state[ps[0]]
    opt.param_groups[0]["momentum"] = 0.9
    b = _host_step(opt, ps)
    assert b is not a and b[0][1][0].momentum_buffer == opt.state[ps[0]]["momentum_buffer"].data_ptr()
    assert [float(opt.state[p]["step"]) for p in ps] == [1.0, 1.0]               # counted from 0: the first one was the copy
    ropt, rps, _ = _on_cpu("rmsprop", 2)
    a = _host_step(ropt, rps)
    ropt.param_groups[0]["centered"] = True
    b = _host_step(ropt, rps)
    assert b is not a and b[0][1][1].grad_avg == ropt.state[rps[1]]["grad_avg"].data_ptr() and float(ropt.state[rps[0]]["step"]) == 2.0


def test_empty_parameter_is_left_out_of_the_launch():
    for cls, kw in ((SGD, dict(momentum=0.9)), (RMSprop, dict())):
        ps = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.zeros(0)), torch.nn.Parameter(torch.ones(1))]
        for p in ps:
            p.grad = torch.ones_like(p)
        opt = cls(ps, **kw)
        launches = opt._launches_of(0, ps, [p.grad for p in ps], on_device=False)
        assert len(launches) == 1 and [id(p) for p in launches[0][0]] == [id(ps[0]), id(ps[2])]
        assert [launches[0][1][k].numel for k in range(2)] == [3, 1] and ps[1] not in opt.state


# ---- state dicts: ours into torch's classes and back -----------------------------------------------------------------------------------
def _twins(n=3):
    ours = [torch.nn.Parameter(torch.arange(4.0) + k) for k in range(n)]
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    for p in ours + theirs:
        p.grad = torch.full((4,), 0.5)
    return ours, theirs


def test_sgd_state_round_trip_with_torch():
    ours, theirs = _twins()
    kw = dict(lr=0.1, momentum=0.9, dampening=0.1)
    # torch -> ours: a state with a momentum_buffer and no step is one update old (the buffer is used, not overwritten)
    topt = torch.optim.SGD(theirs, **kw)
    topt.step()
    sd = topt.state_dict()
    assert all(set(s) == {"momentum_buffer"} for s in sd["state"].values())
    opt = SGD(ours, **kw)
    opt.load_state_dict(copy.deepcopy(sd))
    assert all(g["capturable"] for g in opt.param_groups)
    launches = _host_step(opt, ours)
    for k, p in enumerate(ours):
        st = opt.state[p]
        assert torch.equal(st["momentum_buffer"], topt.state[theirs[k]]["momentum_buffer"])
        assert launches[0][1][k].momentum_buffer == st["momentum_buffer"].data_ptr()
        assert float(st["step"]) == 2.0                                          # 1 from the loaded buffer + the host step's 1
    # ours -> torch: the extra step key is ignored, the buffer is the one torch goes on with
    for p in ours:
        opt.state[p]["momentum_buffer"].fill_(0.25)
    back = torch.optim.SGD(theirs, **kw)
    back.load_state_dict(copy.deepcopy(opt.state_dict()))
    before = [p.detach().clone() for p in theirs]
    back.step()
    for p, q in zip(theirs, before):                                             # buf = 0.9 * 0.25 + 0.9 * 0.5 = 0.675; p -= 0.1 * buf
        assert torch.allclose(p, q - 0.1 * 0.675, rtol=0, atol=1e-6)
        assert torch.allclose(back.state[p]["momentum_buffer"], torch.full((4,), 0.675))
    # a loaded state WITH step keeps it
    opt2 = SGD(ours, **kw)
    sd2 = copy.deepcopy(opt.state_dict())
    assert all(float(s["step"]) == 2.0 for s in sd2["state"].values())
    opt2.load_state_dict(sd2)
    _host_step(opt2, ours)
    assert [float(opt2.state[p]["step"]) for p in ours] == [3.0] * 3


@pytest.mark.parametrize("kw", [dict(), dict(centered=True, momentum=0.9)], ids=["default", "centered+momentum"])
def test_rmsprop_state_round_trip_with_torch(kw):
    ours, theirs = _twins()
    names = ("square_avg",) + (("grad_avg", "momentum_buffer") if kw else ())
    topt = torch.optim.RMSprop(theirs, lr=0.01, **kw)
    topt.step()
    topt.step()
    sd = topt.state_dict()
    assert all(set(s) >= set(names) | {"step"} for s in sd["state"].values())
    opt = RMSprop(ours, lr=0.01, **kw)
    opt.load_state_dict(copy.deepcopy(sd))
    assert all(g["capturable"] for g in opt.param_groups)
    launches = _host_step(opt, ours)
    for k, p in enumerate(ours):
        st = opt.state[p]
        for nm in names:
            assert torch.equal(st[nm], topt.state[theirs[k]][nm]) and getattr(launches[0][1][k], nm) == st[nm].data_ptr()
        assert float(st["step"]) == 3.0
    # ours -> torch: the STATE loads (the groups stay torch's own: ours say capturable=True, which torch's class refuses on CPU tensors)
    back = torch.optim.RMSprop(theirs, lr=0.01, **kw)
    back.load_state_dict({"state": copy.deepcopy(opt.state_dict()["state"]), "param_groups": back.state_dict()["param_groups"]})
    for k, q in enumerate(theirs):
        for nm in names:
            assert torch.equal(back.state[q][nm], opt.state[ours[k]][nm])
    back.step()
    for q in theirs:
        assert float(back.state[q]["step"]) == 4.0 and bool(torch.isfinite(q).all())
    assert set(opt.state_dict()["state"][0]) == set(names) | {"step"}            # torch's keys, nothing else
