#!/usr/bin/env python3
"""Generate tests/golden/custom_scheduler.json by RUNNING THE REFERENCE'S OWN ``src/core/schedulers.CustomScheduler`` in this
container.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_scheduler_golden.py

The reference tree is imported read-only (the recipe of make_eval_golden.py).  Only OUTPUT DATA is written: per case the
learning rates after each of 12 ``step()`` calls (``get_lr()[0]`` and the optimizer group's ``lr``), and for the resume case the
``state_dict()`` taken after 6 epochs and the rates of a second scheduler that loaded it.  tests/test_schedulers.py reads the JSON."""
import copy
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
EPOCHS = 12

# name -> (lr, milestones, gamma)
CASES = {"one_milestone": (1e-3, [4], 0.1), "three_milestones": (1e-2, [2, 5, 9], 0.5)}
RESUME = {"lr": 1e-2, "milestones": [2, 5, 9], "gamma": 0.5, "saved_after": 6}


def main():
    import torch
    sys.path.insert(0, REF)
    from src.core.schedulers import CustomScheduler       # reference code, executed not copied

    def optimizer(lr):
        return torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)

    def run(sched, opt, epochs):
        out = []
        for _ in range(epochs):
            sched.step()
            out.append({"epoch": sched.last_epoch, "get_lr": sched.get_lr(), "group_lr": opt.param_groups[0]["lr"]})
        return out

    record = {"epochs": EPOCHS, "cases": {}}
    for name, (lr, milestones, gamma) in CASES.items():
        opt = optimizer(lr)
        sched = CustomScheduler(opt, list(milestones), gamma)
        record["cases"][name] = {"lr": lr, "milestones": milestones, "gamma": gamma, "after_construction": sched.get_lr(),
                                 "steps": run(sched, opt, EPOCHS)}
    r = RESUME
    opt = optimizer(r["lr"])
    sched = CustomScheduler(opt, list(r["milestones"]), r["gamma"])
    first = run(sched, opt, r["saved_after"])
    saved = copy.deepcopy(sched.state_dict())
    opt2 = optimizer(saved["lr"])                          # a resumed run restores the optimizer's lr with the optimizer's own state
    sched2 = CustomScheduler(opt2, list(r["milestones"]), r["gamma"])
    sched2.load_state_dict(copy.deepcopy(saved))
    record["resume"] = dict(r, first=first, state_dict=saved, steps=run(sched2, opt2, EPOCHS - r["saved_after"]))
    with open(os.path.join(HERE, "custom_scheduler.json"), "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps(record)[:400])


if __name__ == "__main__":
    main()
