"""The optimizer update of the training step as ONE launch per step: ``Adam`` (``eg_adam_step``, csrc/adam.hip), ``SGD`` and ``RMSprop``
(``eg_sgd_step`` / ``eg_rmsprop_step``, csrc/optim.hip) -- the three names of the reference's optimizer registry
(src/builders/optimizer_builder.py), with its builder (``OPTIMIZERS``, ``build``).  All three are one kernel and one host function
(csrc/multi_tensor.h) around a dozen lines of arithmetic each.

The reference trains with ``torch.optim.Adam`` (src/engine.py's optimizer builder).  torch's fused form is a ``_foreach_add_`` on
the step counts plus one multi-tensor launch per ~30 tensors: 4 launches (34 us of a 0.9-ms captured batch-1 step) for the 73
parameter tensors of the GNN stack and heads.  ``Adam`` below runs the same arithmetic (torch's fused Adam, amsgrad off) in one launch
per 96 tensors; the step counts are device floats (one per parameter, as in torch), so the update can be captured into a HIP graph
(``engine.GraphedTrainStep`` asks for ``capturable``: these optimizers always are).  State layout as torch's (``state[p]`` = ``step``,
``exp_avg``, ``exp_avg_sq``), so ``state_dict()`` / ``load_state_dict()`` round-trip and a ``torch.optim.Adam`` state loads.

``torch.optim.SGD`` has no capturable form and ``torch.optim.RMSprop(capturable=True)`` is a chain of ``_foreach_*`` launches; ``SGD``
(one launch per 120 tensors) and ``RMSprop`` (per 84) run torch's ``_single_tensor_sgd`` / ``_single_tensor_rmsprop`` arithmetic with
torch's state keys (``momentum_buffer``; ``step``, ``square_avg``, ``momentum_buffer``, ``grad_avg``).  ``SGD`` keeps a ``step`` as well
(torch.optim.SGD ignores the key): the kernel reads it to decide whether an update is the tensor's first, the one that copies the
gradient into the momentum buffer -- on the device, so a captured launch is right on both sides of that update.

``lr`` may be a CUDA float32 scalar tensor (torch's convention for captured steps: the kernel reads it, so a scheduler's ``fill_`` reaches the
replays); a float lr is frozen into a captured launch.  CUDA float32 parameters with dense gradients only; anything else raises (there
is no CPU path)."""
from __future__ import annotations

import copy
import ctypes as ct
from typing import Iterable

import torch

from . import _lib

_MAX_TENSORS = 96                                       # EG_ADAM_MAX_TENSORS
_SGD_MAX_TENSORS = 120                                  # EG_SGD_MAX_TENSORS
_RMSPROP_MAX_TENSORS = 84                               # EG_RMSPROP_MAX_TENSORS


def _entry_type(name, *state):
    """The table entry of one update (eg_adam_tensor, eg_sgd_tensor, eg_rmsprop_tensor of include/echoglad_hip.h): param, grad, the
    state arrays under torch's state keys, numel."""
    fields = [(f, ct.c_void_p) for f in ("param", "grad") + state] + [("numel", ct.c_int64)]
    return type(name, (ct.Structure,), {"_fields_": fields})


_AdamTensor = _entry_type("_AdamTensor", "exp_avg", "exp_avg_sq")
_SGDTensor = _entry_type("_SGDTensor", "momentum_buffer")
_RMSpropTensor = _entry_type("_RMSpropTensor", "square_avg", "grad_avg", "momentum_buffer")


class _OneLaunch(torch.optim.Optimizer):
    """What the three optimizers share: the step loop, the prepared-launch cache and the per-launch count arrays.  A subclass names
    its table entry (``_ENTRY``: a state array that a group's update does not use is NULL there), its per-launch maximum (``_MAX``),
    the state tensors a group's update uses (``_names``) and the call itself (``_launch``)."""
    _ENTRY = None
    _MAX = 0
    _ALWAYS_CAPTURABLE = True                           # load_state_dict keeps ``capturable`` set, whatever the saved groups say

    def _names(self, group):
        """The keys of the state tensors (beside ``step``) that this group's update reads and writes, in the table's order."""
        raise NotImplementedError

    def _launch(self, lib, group, table, count, counts, lr, lr_dev, stream):
        raise NotImplementedError

    @property
    def _who(self):
        return f"echoglad_amd.optim.{type(self).__name__}"

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib, stream = None, None
        for gi, group in enumerate(self.param_groups):
            ps, grads = [], []
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    ps.append(p)
                    grads.append(g)
            if not ps:
                continue
            if not ps[0].is_cuda:
                raise RuntimeError(f"{self._who}: CUDA float32 parameters with dense float32 gradients only")
            if lib is None:
                lib = _lib.load()
                stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
            launches = self._launches_of(gi, ps, grads)
            lr = group["lr"]
            lr_dev = None
            if torch.is_tensor(lr):                     # (torch's convention for a captured step: schedulers fill_() a tensor lr)
                if not lr.is_cuda or lr.dtype != torch.float32 or lr.numel() != 1:
                    raise RuntimeError(f"{self._who}: a tensor lr must be a CUDA float32 scalar")
                lr_dev, lr = ct.c_void_p(lr.data_ptr()), 0.0
            for part, table, counts, _views, _moments in launches:
                self._launch(lib, group, table, len(part), ct.c_void_p(counts.data_ptr()), float(lr), lr_dev, stream)
                # the kernel wrote the parameters behind autograd's back: tell it (in-place version counters: what saved-tensor checks
                # and the model's caches of folded inference parameters are keyed on)
                torch.autograd.graph.increment_version(part)
        return loss

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self.__dict__.pop("_prepared", None)            # (the moments and counts are new tensors)
        self.__dict__.pop("_count_arrays", None)
        if self._ALWAYS_CAPTURABLE:                     # (groups saved by torch's classes say nothing, or False: not so here)
            for group in self.param_groups:
                group["capturable"] = True

    def _launches_of(self, gi, ps, grads, on_device=True):
        """The prepared launches of group ``gi`` for the parameters ``ps`` (those with a gradient, in order; ``grads``: their
        gradients).  They are kept while nothing moved: the same parameters at the same addresses, contiguous gradients at the same
        addresses (the caching allocator hands a step's gradients the same blocks again), the same state tensors in use (a group's
        ``momentum`` or ``centered`` switched on or off changes them) AND ``self.state`` still holding the very count views and state
        tensors the tables point at (``_prepared_valid``) -- checks and 82 ctypes structs per step were 0.2 ms of a batch-1 step the
        host is the bound of.  ``on_device`` False: CPU tensors pass (the host-logic tests walk the cache without a GPU; nothing is
        launched)."""
        group = self.param_groups[gi]
        names = self._names(group)
        key = (tuple(map(id, ps)), tuple([p.data_ptr() for p in ps]), tuple([g.data_ptr() for g in grads]), names)
        cache = self.__dict__.setdefault("_prepared", {}).setdefault(gi, {})
        hit = cache.get(key)
        if hit is not None and not (_prepared_valid(self.state, hit, names) and all([g.is_contiguous() for g in grads])):
            del cache[key]
            hit = None
        if hit is None:                                 # (the allocator cycles through a few sets of blocks for a step's gradients)
            if len(cache) >= 4:
                cache.clear()
            copied = not all(g.is_contiguous() for g in grads)
            hit = self._prepare(ps, on_device, group, names)
            if not copied:                              # (a gradient copied to a contiguous one is not at the key's address: not kept)
                cache[key] = hit
        return hit

    def _prepare(self, ps, on_device, group, names):
        """[(parameters, table, step counts, their 0-d views, the state tensors per parameter)] -- one entry per launch of up to
        ``_MAX`` parameters.  The views and state tensors are what ``state[p]`` holds at this moment: they keep the memory behind
        the table alive and are what ``_prepared_valid`` compares ``state`` with.  An empty parameter is in no launch (the entry points
        take no empty entry): it is left alone, as torch's optimizers leave it."""
        ps = [p for p in ps if p.numel() > 0]
        for p in ps:
            if (on_device and not p.is_cuda) or p.dtype != torch.float32 or p.grad.is_sparse or p.grad.dtype != torch.float32:
                raise RuntimeError(f"{self._who}: CUDA float32 parameters with dense float32 gradients only")
            if not p.is_contiguous():
                raise RuntimeError(f"{self._who}: parameters must be contiguous")
            if not p.grad.is_contiguous():
                p.grad = p.grad.contiguous()
            st = self.state[p]
            for name in names:
                t = st.get(name)
                if t is None:
                    st[name] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                elif (not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != p.device or t.numel() != p.numel()
                      or not t.is_contiguous()):
                    raise RuntimeError(f"{self._who}: state[p]['{name}'] must be a contiguous float32 tensor of the parameter's size on its device")
        out = []
        fields = [f for f, _ in self._ENTRY._fields_[2:-1]]
        for lo in range(0, len(ps), self._MAX):
            part = ps[lo:lo + self._MAX]
            counts, views = self._counts_of(part)
            table = (self._ENTRY * len(part))()
            moments = []
            for k, p in enumerate(part):
                st = self.state[p]
                tensors = tuple(st[name] for name in names)
                table[k] = self._ENTRY(p.data_ptr(), p.grad.data_ptr(), *[st[f].data_ptr() if f in names else None for f in fields], p.numel())
                moments.append(tensors)
            out.append((part, table, counts, views, moments))
        return out

    def _initial_count(self, st):
        """The count of a parameter whose state has no ``step``."""
        return 0.0

    def _counts_of(self, part):
        """(array, views): the step counts of the parameters of one launch as ONE device array (the kernel takes steps[k]);
        ``state[p]["step"]`` are 0-d views of it.  Kept while the same parameters come in the same order; otherwise (first step, a
        parameter that had no gradient last time, a loaded state) re-assembled from the per-parameter counts -- torch's state layout
        stays the truth."""
        key = tuple(id(p) for p in part)
        hit = self.__dict__.setdefault("_count_arrays", {}).get(key)
        if hit is not None and all(self.state[p].get("step") is v for p, v in zip(part, hit[1])):
            return hit
        dev = part[0].device
        vals = []
        for p in part:
            t = self.state[p].get("step")
            if t is None:
                t = self._initial_count(self.state[p])
            vals.append(t.detach().to(device=dev, dtype=torch.float32).reshape(()) if torch.is_tensor(t) else
                        torch.tensor(float(t), dtype=torch.float32, device=dev))
        counts = torch.stack(vals)
        views = [counts[k] for k in range(len(part))]
        for p, v in zip(part, views):
            self.state[p]["step"] = v
        if len(self._count_arrays) > 8:
            self._count_arrays.clear()
        self._count_arrays[key] = (counts, views)
        return counts, views


class Adam(_OneLaunch):
    _ENTRY = _AdamTensor
    _MAX = _MAX_TENSORS
    _ALWAYS_CAPTURABLE = False                          # (as it always was: the loaded groups stand)

    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 maximize: bool = False):
        if not torch.is_tensor(lr) and not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # (capturable / fused: what engine.GraphedTrainStep and code written for torch.optim.Adam look for)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, maximize=maximize, capturable=True, fused=True)
        super().__init__(params, defaults)

    def _names(self, group):
        return ("exp_avg", "exp_avg_sq")

    def _launch(self, lib, group, table, count, counts, lr, lr_dev, stream):
        b1, b2 = group["betas"]
        _lib.check(lib.eg_adam_step(table, count, counts, lr, lr_dev, float(b1), float(b2), float(group["eps"]),
                                    float(group["weight_decay"]), int(bool(group["maximize"])), stream), "eg_adam_step")


class SGD(_OneLaunch):
    """torch.optim.SGD's update (``_single_tensor_sgd``) in one launch per 120 tensors.  ``state[p]["step"]`` counts the updates the
    momentum buffer has seen: 0 makes the next update the one that copies the gradient into the buffer (torch: ``momentum_buffer is
    None``).  A buffer that comes without a count (a torch.optim.SGD state) is one update old; a buffer that has to be created (first
    update, state cleared, ``momentum`` switched on later) starts the count at 0 again."""
    _ENTRY = _SGDTensor
    _MAX = _SGD_MAX_TENSORS

    def __init__(self, params: Iterable, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                 nesterov: bool = False, maximize: bool = False):
        if not torch.is_tensor(lr) and not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= momentum:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize,
                        capturable=True)
        super().__init__(params, defaults)

    def _names(self, group):
        return ("momentum_buffer",) if group["momentum"] != 0 else ()

    def _initial_count(self, st):
        return 1.0 if torch.is_tensor(st.get("momentum_buffer")) else 0.0

    def _prepare(self, ps, on_device, group, names):
        if names:                                       # a buffer that is about to be created: its first update is a copy
            for p in ps:
                if p.numel() > 0 and self.state[p].get("momentum_buffer") is None:
                    self.state[p]["step"] = 0.0
        return super()._prepare(ps, on_device, group, names)

    def _launch(self, lib, group, table, count, counts, lr, lr_dev, stream):
        _lib.check(lib.eg_sgd_step(table, count, counts, lr, lr_dev, float(group["momentum"]), float(group["dampening"]),
                                   float(group["weight_decay"]), int(bool(group["nesterov"])), int(bool(group["maximize"])), stream),
                   "eg_sgd_step")


class RMSprop(_OneLaunch):
    """torch.optim.RMSprop's update (``_single_tensor_rmsprop``) in one launch per 84 tensors (five pointers per tensor in 4 KB of
    kernel arguments)."""
    _ENTRY = _RMSpropTensor
    _MAX = _RMSPROP_MAX_TENSORS

    def __init__(self, params: Iterable, lr: float = 1e-2, alpha: float = 0.99, eps: float = 1e-8, weight_decay: float = 0.0,
                 momentum: float = 0.0, centered: bool = False, maximize: bool = False):
        if not torch.is_tensor(lr) and not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= momentum:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if not 0.0 <= alpha:
            raise ValueError(f"Invalid alpha value: {alpha}")
        defaults = dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=centered, weight_decay=weight_decay, maximize=maximize,
                        capturable=True)
        super().__init__(params, defaults)

    def _names(self, group):
        return ("square_avg",) + (("grad_avg",) if group["centered"] else ()) + (("momentum_buffer",) if group["momentum"] > 0 else ())

    def _launch(self, lib, group, table, count, counts, lr, lr_dev, stream):
        _lib.check(lib.eg_rmsprop_step(table, count, counts, lr, lr_dev, float(group["alpha"]), float(group["eps"]),
                                       float(group["weight_decay"]), float(group["momentum"]), int(bool(group["centered"])),
                                       int(bool(group["maximize"])), stream), "eg_rmsprop_step")


def _prepared_valid(state, launches, names=("exp_avg", "exp_avg_sq")) -> bool:
    """Whether prepared launches (``_OneLaunch._prepare``) still describe ``state``: for every parameter ``state[p]["step"]`` is the
    cached view of the launch's count array and the state tensors ``names`` (Adam's by default) are the tensors whose addresses sit in
    the table.  Anything else -- a step in between that left a parameter out (its neighbours' counts moved to another array), a moment
    or a count replaced, ``state[p]`` cleared or deleted -- and the launch would advance counts and moments nobody looks at any more.
    Identity checks on plain objects only: this runs in every step.  (In-place edits -- ``zero_()``, ``copy_()``, ``fill_()`` -- write
    the memory the table points at and need no new table.)"""
    get = state.get
    if len(names) == 2:                                 # (Adam, RMSprop with one flag: the loop without an inner loop -- 82 tensors per step)
        n0, n1 = names
        for part, _table, _counts, views, moments in launches:
            if moments and len(moments[0]) != 2:
                return False
            for p, view, (m, v) in zip(part, views, moments):
                st = get(p)
                if st is None or st.get("step") is not view or st.get(n0) is not m or st.get(n1) is not v:
                    return False
        return True
    if len(names) == 1:                                 # (SGD with a momentum, plain RMSprop)
        n0, = names
        for part, _table, _counts, views, moments in launches:
            if moments and len(moments[0]) != 1:
                return False
            for p, view, (m,) in zip(part, views, moments):
                st = get(p)
                if st is None or st.get("step") is not view or st.get(n0) is not m:
                    return False
        return True
    for part, _table, _counts, views, moments in launches:
        for p, view, tensors in zip(part, views, moments):
            st = get(p)
            if st is None or st.get("step") is not view or len(tensors) != len(names):
                return False
            for name, t in zip(names, tensors):
                if st.get(name) is not t:
                    return False
    return True


# ---- the reference's optimizer builder (src/builders/optimizer_builder.py) -----------------------------------------------------------
OPTIMIZERS = {"sgd": SGD, "rmsprop": RMSprop, "adam": Adam}


def build(optim_config, models, logger=None, device_lr=False):
    """The reference's ``optimizer_builder.build``: ``optim_config["name"]`` picks the class, the other keys are its arguments, the
    parameters are the embedder's and then the landmark model's.  The caller's config is left as it is.  An unknown name raises
    ``KeyError`` with the registry's names.  ``device_lr``: ``lr`` becomes a CUDA float32 scalar tensor (on the first parameter's
    device), so that a scheduler's change reaches the replays of a captured step (``engine.GraphedTrainStep``)."""
    config = copy.deepcopy(dict(optim_config))
    name = config.pop("name")
    if name not in OPTIMIZERS:
        raise KeyError(f"unknown optimizer '{name}': specify one of {sorted(OPTIMIZERS)}")
    params = list(models["embedder"].parameters()) + list(models["landmark"].parameters())
    if device_lr:
        cls = OPTIMIZERS[name]
        lr = config.get("lr", 1e-2 if cls is RMSprop else 1e-3)
        if not torch.is_tensor(lr):
            dev = next((p.device for p in params if p.is_cuda), None)
            if dev is None:
                raise RuntimeError("echoglad_amd.optim.build(device_lr=True): the models' parameters are not on a GPU")
            lr = torch.tensor(float(lr), dtype=torch.float32, device=dev)
        config["lr"] = lr
    optimizer = OPTIMIZERS[name](params, **config)
    if logger is not None:
        logger.infov(f"optimizer built: {name.upper()} ({type(optimizer).__module__}.{type(optimizer).__name__})")
    return optimizer
