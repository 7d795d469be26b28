"""The reference's learning-rate schedules (src/builders/scheduler_builder.py, src/core/schedulers.py): ``multi`` and
``reduce_lr_on_plateau`` are torch's own classes, ``custom`` is ``CustomScheduler`` below; ``build`` picks one from a training config.

Under a captured training step (``engine.GraphedTrainStep``) a group's ``lr`` is a CUDA float32 scalar tensor
(``optim.build(..., device_lr=True)``) that the update kernel reads in every replay.  torch's two schedulers ``fill_()`` such a tensor;
``CustomScheduler`` does the same -- it never puts a float in the tensor's place, which the capture would not see."""
from __future__ import annotations

import copy

import torch
from torch.optim import lr_scheduler
from torch.optim.optimizer import Optimizer


def _value(lr) -> float:
    return float(lr.item()) if torch.is_tensor(lr) else float(lr)


class CustomScheduler:
    """Multiply the learning rate by ``gamma`` at the epoch ``milestones[0]``, then drop that milestone while more than one remains
    (the last one stays, so it fires once and never again as the epochs go on).  One learning rate for every group -- the last
    group's at construction, as in the reference.  ``step()`` is called once per epoch; construction takes the step to ``last_epoch``
    (0 when it is -1)."""

    def __init__(self, optimizer, milestones, gamma, last_epoch=-1):
        if not isinstance(optimizer, Optimizer):
            raise TypeError(f"{type(optimizer).__name__} is not an Optimizer")
        self.optimizer = optimizer
        self.milestones = list(milestones)              # (popped from below: the caller's list stays whole)
        self.gamma = gamma
        if last_epoch == -1:
            for group in optimizer.param_groups:
                group.setdefault("initial_lr", _value(group["lr"]))
            last_epoch = 0
        else:
            for i, group in enumerate(optimizer.param_groups):
                if "initial_lr" not in group:
                    raise KeyError(f"param 'initial_lr' is not specified in param_groups[{i}] when resuming an optimizer")
        self.base_lrs = [group["initial_lr"] for group in optimizer.param_groups]
        self.lr = _value(optimizer.param_groups[-1]["lr"])
        self.step(last_epoch)

    def state_dict(self):
        return {key: (list(value) if key == "milestones" else value) for key, value in self.__dict__.items() if key != "optimizer"}

    def load_state_dict(self, state_dict):
        self.__dict__.update(copy.deepcopy(state_dict))

    def get_lr(self):
        return [self.lr]

    def step(self, epoch=None):
        if epoch is None:
            epoch = self.last_epoch + 1
        self.last_epoch = epoch
        if self.milestones and self.last_epoch == self.milestones[0]:
            self.lr *= self.gamma
            for group in self.optimizer.param_groups:
                if torch.is_tensor(group["lr"]):
                    group["lr"].fill_(self.lr)          # the tensor a captured launch reads: keep it, change its value
                else:
                    group["lr"] = self.lr
            if len(self.milestones) > 1:
                self.milestones.pop(0)


SCHEDULERS = {"multi": lr_scheduler.MultiStepLR, "reduce_lr_on_plateau": lr_scheduler.ReduceLROnPlateau, "custom": CustomScheduler}


def build(train_config, optimizer, logger=None):
    """The reference's ``scheduler_builder.build``: None when ``train_config`` has no ``lr_schedule``; otherwise
    ``lr_schedule["name"]`` (default ``multi``) picks the class and the other keys are its arguments.  An unknown name raises
    ``KeyError`` (the reference logs and exits).  The caller's config is left as it is."""
    if "lr_schedule" not in train_config:
        if logger is not None:
            logger.warn("No scheduler is specified.")
        return None
    config = copy.deepcopy(dict(train_config["lr_schedule"]))
    name = config.pop("name", "multi")
    if name not in SCHEDULERS:
        raise KeyError(f"unknown scheduler '{name}': specify one of {sorted(SCHEDULERS)}")
    scheduler = SCHEDULERS[name](optimizer, **config)
    if logger is not None:
        logger.infov(f"scheduler built: {name.upper()}")
    return scheduler
