"""The bits of the one-launch optimizers (echoglad_amd.optim: Adam, SGD, RMSprop on csrc/multi_tensor.h): one sha256 per configuration
over the parameters, the state tensors and the step counts after five steps on seeded inputs.  Two builds that print the same lines
compute the same updates, operation for operation (a contraction or an order that moved shows as another digest).

    python tools/optim_bits.py            (GPU box; ECHOGLAD_LIB picks the library: bash tools/lib_ab.sh <tag> 1 "python tools/optim_bits.py" base <variant>)

Tensors of 1, 1023, 1024, 1025 and 2049 elements (the edges of the 1024-element chunk of a workgroup) and 100 of 300: 105 tensors, two
launches for Adam (96 per launch) and RMSprop (84).  The second step leaves one gradient out: that tensor's count falls behind."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from echoglad_amd import optim  # noqa: E402

SIZES = [1, 1023, 1024, 1025, 2049] + [300] * 100
STEPS, LEFT_OUT = 5, 3
CONFIGS = [
    ("adam", optim.Adam, dict(lr=1e-3)),
    ("adam weight_decay", optim.Adam, dict(lr=1e-3, weight_decay=0.01)),
    ("adam maximize", optim.Adam, dict(lr=1e-3, maximize=True)),
    ("adam tensor lr", optim.Adam, dict(lr="tensor")),
    ("sgd", optim.SGD, dict(lr=0.01)),
    ("sgd momentum", optim.SGD, dict(lr=0.01, momentum=0.9)),
    ("sgd nesterov", optim.SGD, dict(lr=0.01, momentum=0.9, nesterov=True)),
    ("sgd dampening weight_decay", optim.SGD, dict(lr=0.01, momentum=0.9, dampening=0.1, weight_decay=0.01)),
    ("rmsprop", optim.RMSprop, dict(lr=0.01)),
    ("rmsprop centered", optim.RMSprop, dict(lr=0.01, centered=True)),
    ("rmsprop momentum", optim.RMSprop, dict(lr=0.01, momentum=0.9)),
    ("rmsprop centered momentum", optim.RMSprop, dict(lr=0.01, centered=True, momentum=0.9)),
]


def digest(opt, ps):
    h = hashlib.sha256()
    for p in ps:
        h.update(p.detach().cpu().numpy().tobytes())
        for key, t in sorted(opt.state[p].items()):
            h.update(key.encode())
            h.update(torch.as_tensor(t).detach().cpu().numpy().tobytes())
    return h.hexdigest()


def main():
    assert torch.cuda.is_available(), "optim_bits.py runs the kernels: it needs a GPU"
    dev = torch.device("cuda", 0)
    for name, cls, kw in CONFIGS:
        gen = torch.Generator().manual_seed(1234)
        ps = [torch.nn.Parameter(torch.randn(n, generator=gen).to(dev)) for n in SIZES]
        if kw.get("lr") == "tensor":
            kw = dict(kw, lr=torch.tensor(1e-3, dtype=torch.float32, device=dev))
        opt = cls(ps, **kw)
        for step in range(STEPS):
            for k, p in enumerate(ps):
                g = torch.randn(p.shape, generator=gen).to(dev)
                p.grad = None if (step == 1 and k == LEFT_OUT) else g
            opt.step()
        torch.cuda.synchronize()
        counts = sorted({float(opt.state[p]["step"]) for p in ps})
        print(f"{name}: {digest(opt, ps)}  (step counts {counts})", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
